// obs_io.hpp - host-side observation ingestion (no GPU involved).  Included by imcoal_fwd.hip only.
//
//  * read_observation_file: the reference's text format (whitespace-separated decimal symbols, written by
//    scripts/prepare-alignments.py:92-105 and read at src/IMCoalHMM/hmm.py:13-14) or this library's packed
//    cache ("IMCOBS1\n" magic; 2 bits per column when nsym <= 4, 1 byte up to 256 symbols, 2 bytes beyond);
//    templated on the symbol type: uint8_t for alphabets up to 256, uint16_t beyond (the ILS quartet alphabet of
//    scripts/prepare-alignments.py:186-190 has 257 symbols);
//  * encode_pairwise: the pairwise symbol rule of scripts/prepare-alignments.py:99-105
//    (2 = either base not in ACGT, 0 = equal, 1 = different; case-insensitive);
//  * write_cache.
// The cache header (read_cache_header) and the text loop (TextParser) are pieces of their own: the device ingestion of
// imcoal_fwd.hip checks headers with the first, and tests/ingest_tiles_check.cpp holds csrc/ingest_tiles.hpp to the second.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace imc {

static const char kCacheMagic[8] = {'I', 'M', 'C', 'O', 'B', 'S', '1', '\n'};

struct IoResult {
    int code = 0;          // 0 ok, -2 symbol, -5 io, -1 arg (values of include/imcoal_fwd.h)
    std::string msg;
};

inline IoResult io_fail(int code, const std::string &m)
{
    IoResult r;
    r.code = code;
    r.msg = m;
    return r;
}

// What follows the magic of a cache file: alphabet size, bits per column (2, 8 or 16), columns; the payload comes next.
struct CacheHeader {
    uint32_t fs = 0, bits = 0;
    uint64_t L = 0;
};

// fp stands behind the magic; the checks a cache header must pass, in the order their errors are reported.
inline IoResult read_cache_header(FILE *fp, const char *path, int nsym, CacheHeader &h)
{
    if (std::fread(&h.fs, 4, 1, fp) != 1 || std::fread(&h.bits, 4, 1, fp) != 1 || std::fread(&h.L, 8, 1, fp) != 1)
        return io_fail(-5, std::string("truncated cache header in ") + path);
    if ((h.bits != 2 && h.bits != 8 && h.bits != 16) || h.fs < 1 || h.fs > 65536 || (h.bits == 2 && h.fs > 4) || (h.bits == 8 && h.fs > 256))
        return io_fail(-5, std::string("bad cache header in ") + path);
    if ((int)h.fs > nsym) return io_fail(-2, "cache holds an alphabet of " + std::to_string(h.fs) + " symbols, more than nsym");
    return IoResult();
}

// The text loop of read_observation_file, fed buffer by buffer: a token is accumulated across feeds (values beyond
// 1000000 read as 1000000), checked against nsym and appended at the whitespace that ends it - or by finish() at the end
// of the file; any byte that is neither digit nor whitespace is an error where it stands.
template <typename T>
struct TextParser {
    long cur = -1;   // token being accumulated, -1 = none

    IoResult feed(const char *buf, size_t n, int nsym, const char *path, std::vector<T> &sym)
    {
        for (size_t i = 0; i < n; ++i) {
            const unsigned char ch = (unsigned char)buf[i];
            if (ch >= '0' && ch <= '9') {
                cur = (cur < 0 ? 0 : cur) * 10 + (ch - '0');
                if (cur > 1000000) cur = 1000000;
            } else if (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r' || ch == '\f' || ch == '\v') {
                if (cur >= 0) {
                    if (cur >= nsym) return io_fail(-2, "symbol " + std::to_string(cur) + " at column " + std::to_string(sym.size()) + " >= nsym");
                    sym.push_back((T)cur);
                    cur = -1;
                }
            } else {
                return io_fail(-5, std::string("unexpected character in ") + path);   // int() would raise ValueError (hmm.py:14)
            }
        }
        return IoResult();
    }

    IoResult finish(int nsym, std::vector<T> &sym)
    {
        if (cur >= 0) {
            if (cur >= nsym) return io_fail(-2, "symbol " + std::to_string(cur) + " >= nsym");
            sym.push_back((T)cur);
            cur = -1;
        }
        return IoResult();
    }
};

template <typename T>
inline IoResult read_observation_file(const char *path, int nsym, std::vector<T> &sym)
{
    if (nsym > (sizeof(T) == 1 ? 256 : 65536)) return io_fail(-1, "alphabet too large for this symbol type");
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return io_fail(-5, std::string("cannot open ") + path + ": " + std::strerror(errno));
    sym.clear();
    char head[8];
    const size_t nh = std::fread(head, 1, 8, fp);
    if (nh == 8 && std::memcmp(head, kCacheMagic, 8) == 0) {
        // ---- packed cache ----
        CacheHeader h;
        const IoResult hr = read_cache_header(fp, path, nsym, h);
        if (hr.code) {
            std::fclose(fp);
            return hr;
        }
        const uint32_t bits = h.bits;
        const uint64_t L = h.L;
        sym.resize(L);
        if (bits == 8 || bits == 16) {
            const size_t w = bits / 8;
            std::vector<uint8_t> raw(L * w);
            if (L && std::fread(raw.data(), 1, raw.size(), fp) != raw.size()) { std::fclose(fp); return io_fail(-5, std::string("truncated cache ") + path); }
            for (uint64_t t = 0; t < L; ++t) sym[t] = (T)(w == 1 ? raw[t] : (uint16_t)(raw[2 * t] | raw[2 * t + 1] << 8));
        } else {
            std::vector<uint8_t> pk((L + 3) / 4);
            if (!pk.empty() && std::fread(pk.data(), 1, pk.size(), fp) != pk.size()) { std::fclose(fp); return io_fail(-5, std::string("truncated cache ") + path); }
            for (uint64_t t = 0; t < L; ++t) sym[t] = (pk[t >> 2] >> (2 * (t & 3))) & 3u;
        }
        std::fclose(fp);
        for (uint64_t t = 0; t < L; ++t)
            if (sym[t] >= nsym) return io_fail(-2, "symbol " + std::to_string(sym[t]) + " at column " + std::to_string(t) + " >= nsym");
        return IoResult();
    }
    // ---- text ----
    std::vector<char> buf(1 << 22);
    TextParser<T> text;
    size_t n = nh;
    std::memcpy(buf.data(), head, nh);
    while (n > 0) {
        const IoResult rc = text.feed(buf.data(), n, nsym, path, sym);
        if (rc.code) {
            std::fclose(fp);
            return rc;
        }
        n = std::fread(buf.data(), 1, buf.size(), fp);
    }
    std::fclose(fp);
    return text.finish(nsym, sym);
}

template <typename T>
inline IoResult write_cache(const char *path, const T *sym, uint64_t L, int nsym)
{
    for (uint64_t t = 0; t < L; ++t)
        if (sym[t] >= nsym) return io_fail(-2, "symbol " + std::to_string(sym[t]) + " at column " + std::to_string(t) + " >= nsym");
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return io_fail(-5, std::string("cannot create ") + path + ": " + std::strerror(errno));
    const uint32_t fs = (uint32_t)nsym, bits = nsym <= 4 ? 2u : nsym <= 256 ? 8u : 16u;
    bool ok = std::fwrite(kCacheMagic, 1, 8, fp) == 8 && std::fwrite(&fs, 4, 1, fp) == 1 && std::fwrite(&bits, 4, 1, fp) == 1 &&
              std::fwrite(&L, 8, 1, fp) == 1;
    if (ok && bits >= 8 && L) {
        std::vector<uint8_t> raw(L * (bits / 8));
        for (uint64_t t = 0; t < L; ++t) {
            if (bits == 8) raw[t] = (uint8_t)sym[t];
            else { raw[2 * t] = (uint8_t)(sym[t] & 0xff); raw[2 * t + 1] = (uint8_t)((uint32_t)sym[t] >> 8); }
        }
        ok = std::fwrite(raw.data(), 1, raw.size(), fp) == raw.size();
    }
    if (ok && bits == 2) {
        std::vector<uint8_t> pk((L + 3) / 4, 0);
        for (uint64_t t = 0; t < L; ++t) pk[t >> 2] |= (uint8_t)(sym[t] << (2 * (t & 3)));
        if (!pk.empty()) ok = std::fwrite(pk.data(), 1, pk.size(), fp) == pk.size();
    }
    ok = (std::fclose(fp) == 0) && ok;
    return ok ? IoResult() : io_fail(-5, std::string("write failed: ") + path);
}

inline void encode_pairwise(const char *s1, const char *s2, size_t L, uint8_t *out)
{
    bool clean[256] = {false};
    for (const char *p = "ACGTacgt"; *p; ++p) clean[(unsigned char)*p] = true;
    for (size_t t = 0; t < L; ++t) {
        const unsigned char a = (unsigned char)s1[t], b = (unsigned char)s2[t];
        if (!clean[a] || !clean[b]) out[t] = 2;
        else out[t] = ((a & 0xdf) == (b & 0xdf)) ? 0 : 1;   // ASCII upper-casing of letters
    }
}

}  // namespace imc
