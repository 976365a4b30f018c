// phylip_io.hpp - PHYLIP alignments on the host (no GPU involved).  imc::read_phylip is the C++ statement of
// imcoalhmm_amd.prepare.read_phylip for ASCII files - that function, not the PHYLIP standard, is the specification: the
// device parser (phylip_tiles.hpp, kernels_phylip.hpp) is held to this reader by tests/phylip_tiles_check.cpp, and this
// reader reads every file that parser declines and words every error.
//
//  * Lines end at "\n", "\r\n" or a lone "\r" (Python's universal newlines).
//  * A line that is empty once the ASCII whitespace str.strip() removes - \t \n \v \f \r, space and 0x1c-0x1f - is taken
//    from both its ends is dropped, wherever it stands.  The other lines are kept AS THEY ARE (not stripped).
//  * The first kept line is the header: its first two whitespace-separated words are n and length; further words are
//    ignored.
//  * The next n kept lines are name lines.  The name is the first word; the sequence part is what stands behind the name
//    and the whitespace after it, with every ' ' removed - only ' ': a tab or another control byte stays, and so does
//    trailing whitespace other than spaces.  A name line may hold a name only.
//  * Every later kept line k (from 0) is appended, every ' ' removed, to record k % n: one line per record and
//    interleaved blocks both work, blocks may differ in width, and so may the records of one block.
// Deliberate deviations from Python, each IMC_ERR_IO (-5) with a message that names the file:
//  * a byte >= 0x80 (what Python makes of it depends on the locale);
//  * an empty file, or one without a kept line (Python: IndexError);
//  * fewer than two header words (Python: ValueError from the unpacking);
//  * a header word that is not made of decimal digits only (Python's int() also takes "+2", "1_0", " 2 ");
//  * a value that does not fit: n beyond 2^31 - 1, length beyond 2^64 - 1;
//  * n == 0 (Python: ZeroDivisionError, or an empty dict);
//  * fewer than n name lines (Python silently returns fewer records);
//  * a repeated name (Python's dict(zip()) silently keeps one);
//  * every record whose length differs from the header's (Python: ValueError); the message gives the record's name, its
//    length and the header's length, for the first such record in file order.
// Errors are reported in file order, a byte >= 0x80 when the line that holds it ends; the last four when the file ends, in
// the order above.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "fasta_io.hpp"

namespace imc {

struct PhylipHeader {
    uint64_t n = 0, length = 0;
    uint32_t words = 0;           // words on the header line
};

// The header line s[0..len) (no line break in it): n and length.  The device parser parses the header with this function
// too, from the first slab's staged bytes.
inline IoResult phylip_header(const uint8_t *s, size_t len, const char *path, PhylipHeader &h)
{
    uint64_t v[2] = {0, 0};
    h.words = 0;
    for (size_t a = 0; a < len;) {
        while (a < len && fasta_space(s[a])) ++a;
        size_t b = a;
        while (b < len && !fasta_space(s[b])) ++b;
        if (b == a) break;
        if (h.words < 2) {
            uint64_t x = 0;
            for (size_t i = a; i < b; ++i) {
                if (s[i] < '0' || s[i] > '9')
                    return io_fail(-5, "PHYLIP header word '" + std::string(reinterpret_cast<const char *>(s) + a, b - a) + "' is not a decimal number in " + path);
                const uint64_t d = (uint64_t)(s[i] - '0');
                if (x > (UINT64_MAX - d) / 10) return io_fail(-5, std::string("PHYLIP header value does not fit in ") + path);
                x = 10 * x + d;
            }
            v[h.words] = x;
        }
        ++h.words;
        a = b;
    }
    if (h.words < 2) return io_fail(-5, std::string("PHYLIP header needs two numbers in ") + path);
    if (v[0] > 0x7fffffffu) return io_fail(-5, std::string("PHYLIP header value does not fit in ") + path);
    if (v[0] == 0) return io_fail(-5, std::string("PHYLIP header says 0 sequences in ") + path);
    h.n = v[0];
    h.length = v[1];
    return IoResult();
}

// The line loop of read_phylip, fed buffer by buffer.
struct PhylipParser {
    std::string line;             // the unfinished line
    bool after_cr = false;        // the last byte was a '\r' that ended a line: a '\n' now belongs to it
    bool have_header = false;
    PhylipHeader header;
    uint64_t kept = 0;            // kept lines behind the header

    static void append_without_spaces(std::string &to, const std::string &from, size_t a)
    {
        for (size_t i = a; i < from.size(); ++i)
            if (from[i] != ' ') to.push_back(from[i]);
    }

    IoResult end_line(const char *path, FastaRecords &out)
    {
        const size_t n = line.size();
        const uint8_t *s = reinterpret_cast<const uint8_t *>(line.data());
        bool blank = true;
        for (size_t i = 0; i < n; ++i) {
            if (s[i] >= 0x80) return io_fail(-5, std::string("non-ASCII byte in ") + path);
            if (!fasta_space(s[i])) blank = false;
        }
        IoResult r;
        if (blank) {
        } else if (!have_header) {
            r = phylip_header(s, n, path, header);
            have_header = true;
        } else {
            if (kept < header.n) {                    // a name line: str.split(None, 1)
                size_t a = 0;
                while (a < n && fasta_space(s[a])) ++a;
                size_t b = a;
                while (b < n && !fasta_space(s[b])) ++b;
                out.names.emplace_back(line, a, b - a);
                out.seqs.emplace_back();
                while (b < n && fasta_space(s[b])) ++b;
                append_without_spaces(out.seqs.back(), line, b);
            } else
                append_without_spaces(out.seqs[(size_t)(kept % header.n)], line, 0);
            ++kept;
        }
        line.clear();
        return r;
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

    IoResult finish(const char *path, FastaRecords &out)
    {
        const IoResult r = end_line(path, out);
        if (r.code) return r;
        if (!have_header) return io_fail(-5, std::string("no PHYLIP header in ") + path);
        if (out.names.size() < header.n)
            return io_fail(-5, "PHYLIP header says " + std::to_string(header.n) + " sequences, " + std::to_string(out.names.size()) + " name lines in " + path);
        std::set<std::string> seen;
        for (const std::string &name : out.names)
            if (!seen.insert(name).second) return io_fail(-5, "PHYLIP sequence name " + name + " is repeated in " + path);
        for (size_t k = 0; k < out.names.size(); ++k)
            if (out.seqs[k].size() != header.length)
                return io_fail(-5, "PHYLIP sequence " + out.names[k] + " has " + std::to_string(out.seqs[k].size()) + " columns, header says " + std::to_string(header.length) +
                                       " in " + path);
        return IoResult();
    }
};

inline IoResult read_phylip_bytes(const uint8_t *data, size_t n, const char *path, FastaRecords &out)
{
    out.names.clear();
    out.seqs.clear();
    PhylipParser p;
    const IoResult r = p.feed(data, n, path, out);
    return r.code ? r : p.finish(path, out);
}

inline IoResult read_phylip(const char *path, FastaRecords &out)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return io_fail(-5, std::string("cannot open ") + path + ": " + std::strerror(errno));
    out.names.clear();
    out.seqs.clear();
    std::vector<uint8_t> buf(1 << 22);
    PhylipParser p;
    IoResult r;
    for (size_t n; !r.code && (n = std::fread(buf.data(), 1, buf.size(), fp)) > 0;) r = p.feed(buf.data(), n, path, out);
    std::fclose(fp);
    return r.code ? r : p.finish(path, out);
}

}  // namespace imc
