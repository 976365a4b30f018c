// fasta_io.hpp - FASTA alignments on the host (no GPU involved).  imc::read_fasta is the C++ statement of
// imcoalhmm_amd.prepare.read_fasta for ASCII files: the specification the device parser (align_tiles.hpp,
// kernels_align.hpp) is held to by tests/align_tiles_check.cpp, and the reader of every file that parser declines.
//
//  * Lines end at "\n", "\r\n" or a lone "\r" (Python's universal newlines).
//  * A line is stripped at both ends of the ASCII whitespace str.strip() removes - \t \n \v \f \r, space and 0x1c-0x1f -
//    and skipped when nothing is left.
//  * A stripped line that begins with '>' starts a record, named by the first whitespace-separated word behind the '>'.
//  * Every other stripped line is appended to the current record as it is (interior whitespace stays); lines in front of
//    the first header are ignored.
//  * A repeated name keeps its first position and its last sequence (a Python dict).
// Two deliberate deviations from Python, both IMC_ERR_IO (-5):
//  * a header without a name (Python raises IndexError);
//  * a byte >= 0x80 (what Python makes of it depends on the locale).
// Errors are reported in file order, a byte >= 0x80 when the line that holds it ends.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "obs_io.hpp"

namespace imc {

inline bool fasta_space(uint8_t c) { return (c >= 0x09 && c <= 0x0d) || c == ' ' || (c >= 0x1c && c <= 0x1f); }

struct FastaRecords {
    std::vector<std::string> names, seqs;     // in file order (a repeated name: at its first position)
};

// The first whitespace-separated word of s[0..n) ("" when there is none): the name of a header line without its '>'.
inline std::string fasta_first_word(const uint8_t *s, size_t n)
{
    size_t a = 0;
    while (a < n && fasta_space(s[a])) ++a;
    size_t b = a;
    while (b < n && !fasta_space(s[b])) ++b;
    return std::string(reinterpret_cast<const char *>(s) + a, b - a);
}

// The line loop of read_fasta, fed buffer by buffer.
struct FastaParser {
    std::string line;             // the unfinished line
    bool after_cr = false;        // the last byte was a '\r' that ended a line: a '\n' now belongs to it
    long current = -1;            // record that sequence lines go to
    std::map<std::string, size_t> index;

    IoResult end_line(const char *path, FastaRecords &out)
    {
        size_t a = 0, b = line.size();
        for (size_t i = 0; i < b; ++i)
            if ((uint8_t)line[i] >= 0x80) return io_fail(-5, std::string("non-ASCII byte in ") + path);
        while (a < b && fasta_space((uint8_t)line[a])) ++a;
        while (b > a && fasta_space((uint8_t)line[b - 1])) --b;
        if (a < b && line[a] == '>') {
            const std::string name = fasta_first_word(reinterpret_cast<const uint8_t *>(line.data()) + a + 1, b - a - 1);
            if (name.empty()) return io_fail(-5, std::string("header without a name in ") + path);
            auto it = index.find(name);
            if (it == index.end()) {
                it = index.emplace(name, out.names.size()).first;
                out.names.push_back(name);
                out.seqs.emplace_back();
            }
            current = (long)it->second;
            out.seqs[it->second].clear();
        } else if (a < b && current >= 0)
            out.seqs[(size_t)current].append(line, a, b - a);
        line.clear();
        return IoResult();
    }

    IoResult feed(const uint8_t *buf, size_t n, const char *path, FastaRecords &out)
    {
        for (size_t i = 0; i < n; ++i) {
            const uint8_t ch = buf[i];
            const bool skip = after_cr && ch == '\n';
            after_cr = false;
            if (skip) continue;
            if (ch == '\n' || ch == '\r') {
                after_cr = ch == '\r';
                const IoResult r = end_line(path, out);
                if (r.code) return r;
            } else
                line.push_back((char)ch);
        }
        return IoResult();
    }

    IoResult finish(const char *path, FastaRecords &out) { return end_line(path, out); }
};

inline IoResult read_fasta_bytes(const uint8_t *data, size_t n, const char *path, FastaRecords &out)
{
    out.names.clear();
    out.seqs.clear();
    FastaParser p;
    const IoResult r = p.feed(data, n, path, out);
    return r.code ? r : p.finish(path, out);
}

inline IoResult read_fasta(const char *path, FastaRecords &out)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return io_fail(-5, std::string("cannot open ") + path + ": " + std::strerror(errno));
    out.names.clear();
    out.seqs.clear();
    std::vector<uint8_t> buf(1 << 22);
    FastaParser p;
    IoResult r;
    for (size_t n; !r.code && (n = std::fread(buf.data(), 1, buf.size(), fp)) > 0;) r = p.feed(buf.data(), n, path, out);
    std::fclose(fp);
    return r.code ? r : p.finish(path, out);
}

// The triplet rule of scripts/prepare-alignments.py:134-146: i1 + 4 i2 + 16 i3 with A, C, G, T -> 0..3 (either case),
// 64 when any of the three bases is not in ACGT.
inline void encode_triplet(const char *s1, const char *s2, const char *s3, size_t L, uint8_t *out)
{
    int8_t code[256];
    std::memset(code, -1, sizeof code);
    const char *bases = "ACGTacgt";
    for (int k = 0; k < 8; ++k) code[(unsigned char)bases[k]] = (int8_t)(k & 3);
    for (size_t t = 0; t < L; ++t) {
        const int a = code[(unsigned char)s1[t]], b = code[(unsigned char)s2[t]], c = code[(unsigned char)s3[t]];
        out[t] = (a < 0 || b < 0 || c < 0) ? 64 : (uint8_t)(a + 4 * b + 16 * c);
    }
}

}  // namespace imc
