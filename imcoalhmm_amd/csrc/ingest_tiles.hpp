// ingest_tiles.hpp - the parallel form of observation ingestion (obs_io.hpp), host-only: the text parse of
// read_observation_file, the 2-bit cache unpack and the pairwise symbol rule as functions of single positions, so that
// the kernels (kernels_ingest.hpp) and the CPU check (tests/ingest_tiles_check.cpp) call the same code.
//
// The text format is whitespace-separated decimal tokens.  Nothing in its parse is serial: byte i starts a token exactly
// when it is a digit and byte i - 1 is not, the token's value is a function of the at most kMaxTokenDigits bytes from
// there on, and its column is the number of token starts before it.  The host loop reports the FIRST error its byte walk
// meets: a byte that is neither digit nor whitespace where it stands, a token that is not below nsym at the byte that
// ends its digit run (its DETECTION OFFSET; the size of the file for a token that runs to the end of it).  So a range of
// bytes is summarised (IngestSummary) by its token count, the offset of its first bad byte, and the first too-large
// token that starts in it with detection offset, value and column; summaries of adjacent ranges combine associatively
// (ingest_combine), and the summary of everything decides (ingest_verdict): a bad byte at or before the detection offset
// wins.  A digit run longer than kMaxTokenDigits is not evaluated: the summary says `declined` and the file goes to the
// host parser.
//
// A file reaches the device in SLABS of bounded size.  A slab is cut after its last whitespace byte (slab_cut), so no
// token crosses a slab boundary and the byte before a slab is never a digit; the last slab ends where the file ends.
// Offsets are 32-bit within a slab.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "obs_io.hpp"
#include "slab_stream.hpp"

#if defined(__HIPCC__)
#define IMC_ING_HD __host__ __device__
#else
#define IMC_ING_HD
#endif

namespace imc {

// ---- byte classes (exactly those of read_observation_file) ----------------------------------------------
enum ByteClass { kByteDigit = 0, kByteSpace = 1, kByteOther = 2 };

IMC_ING_HD inline ByteClass byte_class(uint8_t ch)
{
    if (ch >= '0' && ch <= '9') return kByteDigit;
    if (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r' || ch == '\f' || ch == '\v') return kByteSpace;
    return kByteOther;
}

// byte i of a slab starts a token (prev: the byte before it; anything but a digit at the start of a slab)
IMC_ING_HD inline bool token_start(uint8_t prev, uint8_t ch) { return byte_class(ch) == kByteDigit && byte_class(prev) != kByteDigit; }

// ---- token value ------------------------------------------------------------------------------------
constexpr uint32_t kMaxTokenDigits = 16;
constexpr uint32_t kTokenCap = 1000000;      // the host loop's cap: every larger value reads as this one

struct TokenRead {
    uint32_t value;      // min(decimal value, kTokenCap)
    uint32_t digits;     // length of the digit run, at most kMaxTokenDigits
    bool declined;       // the run goes on beyond kMaxTokenDigits
};

// The token whose first digit is p[0]; `avail` bytes are readable from p on (the rest of the slab).
IMC_ING_HD inline TokenRead token_read(const uint8_t *p, uint32_t avail)
{
    TokenRead r{0u, 0u, false};
    for (uint32_t j = 0; j <= kMaxTokenDigits; ++j) {
        if (j >= avail || byte_class(p[j]) != kByteDigit) break;
        if (j == kMaxTokenDigits) { r.declined = true; break; }
        r.value = r.value * 10u + (uint32_t)(p[j] - '0');
        if (r.value > kTokenCap) r.value = kTokenCap;
        r.digits = j + 1;
    }
    return r;
}

// ---- summary of a range of bytes -----------------------------------------------------------------------
constexpr uint32_t kNoOffset = 0xffffffffu;

struct IngestSummary {
    uint32_t count;      // token starts in the range
    uint32_t bad;        // slab offset of the first byte of class kByteOther, or kNoOffset
    uint32_t big_det;    // detection offset of the first token >= nsym that starts in the range, or kNoOffset
    uint32_t big_col;    // ... the token starts of the range before it
    uint32_t big_val;    // ... its value
    uint32_t declined;   // a digit run longer than kMaxTokenDigits starts in the range
};

IMC_ING_HD inline IngestSummary ingest_identity() { return IngestSummary{0u, kNoOffset, kNoOffset, 0u, 0u, 0u}; }

// The summary of byte i of a slab of n bytes (i < n); prev is the byte before it (pass a space at i == 0).
IMC_ING_HD inline IngestSummary ingest_position(const uint8_t *at, uint8_t prev, uint32_t i, uint32_t n, uint32_t nsym)
{
    IngestSummary s = ingest_identity();
    const ByteClass c = byte_class(at[0]);
    if (c == kByteOther) s.bad = i;
    if (c == kByteDigit && byte_class(prev) != kByteDigit) {
        s.count = 1u;
        const TokenRead t = token_read(at, n - i);
        if (t.declined) s.declined = 1u;
        else if (t.value >= nsym) { s.big_det = i + t.digits; s.big_val = t.value; }
    }
    return s;
}

// a followed by b.  Tokens that start later are detected later, so a's candidate - if it has one - is the first.
IMC_ING_HD inline IngestSummary ingest_combine(const IngestSummary &a, const IngestSummary &b)
{
    IngestSummary r;
    const bool from_a = a.big_det != kNoOffset;
    r.count = a.count + b.count;
    r.bad = a.bad < b.bad ? a.bad : b.bad;
    r.big_det = from_a ? a.big_det : b.big_det;
    r.big_col = from_a ? a.big_col : a.count + b.big_col;
    r.big_val = from_a ? a.big_val : b.big_val;
    r.declined = a.declined | b.declined;
    return r;
}

// ---- what a slab's summary means ---------------------------------------------------------------------
enum IngestKind { kIngestOk = 0, kIngestBadByte = 1, kIngestSymbol = 2, kIngestDeclined = 3 };
struct IngestVerdict {
    IngestKind kind;
    uint32_t value, column;   // kIngestSymbol: the token and its column within the slab
    bool at_end;              // ... detected at the end of the file (the host's message then names no column)
};

// s: the summary of a whole slab of n bytes.  (Only the last slab can hold a token that runs to its end.)
IMC_ING_HD inline IngestVerdict ingest_verdict(const IngestSummary &s, uint32_t n)
{
    if (s.declined) return IngestVerdict{kIngestDeclined, 0u, 0u, false};
    if (s.bad != kNoOffset && (s.big_det == kNoOffset || s.bad <= s.big_det)) return IngestVerdict{kIngestBadByte, 0u, 0u, false};
    if (s.big_det != kNoOffset) return IngestVerdict{kIngestSymbol, s.big_val, s.big_col, s.big_det >= n};
    return IngestVerdict{kIngestOk, 0u, 0u, false};
}

// The host parser's message for a token that is not below nsym (column: within the whole file).
inline std::string symbol_error_text(uint32_t value, uint64_t column, bool at_end)
{
    if (at_end) return "symbol " + std::to_string(value) + " >= nsym";
    return "symbol " + std::to_string(value) + " at column " + std::to_string(column) + " >= nsym";
}

// ---- slabs -------------------------------------------------------------------------------------------
constexpr size_t kMinSlabBytes = 4096;
constexpr size_t kMaxSlabBytes = (size_t)1 << 30;

// How many of the n buffered bytes form the next slab: all of them at the end of the file, else everything up to and
// including the last whitespace byte.  0 with n > 0: no whitespace in the buffer, the device parser declines the file.
inline size_t slab_cut(const uint8_t *buf, size_t n, bool at_eof)
{
    if (at_eof) return n;
    while (n > 0 && byte_class(buf[n - 1]) != kByteSpace) --n;
    return n;
}

// The slab size a setting asks for (IMC_INGEST_SLAB_BYTES; null or unparsable: the default), within the limits.
inline size_t slab_bytes_setting(const char *text, size_t deflt)
{
    size_t v = deflt;
    if (text && *text) {
        char *end = nullptr;
        const unsigned long long u = std::strtoull(text, &end, 10);
        if (end && end != text) v = (size_t)u;
    }
    return v < kMinSlabBytes ? kMinSlabBytes : v > kMaxSlabBytes ? kMaxSlabBytes : v;
}

// Upper bound of the tokens in `bytes` bytes of text (every token needs a separator but the last).
inline uint64_t max_tokens_in(uint64_t bytes) { return (bytes + 1) / 2; }

// ---- what the host decides ------------------------------------------------------------------------------------
// A rule's answer about a slab or a file is an IoResult: code 0 goes on, kSlabDeclined hands the file to the host parser
// (no text), every other code is an error of include/imcoal_fwd.h with its text.  The engine (imcoal_fwd.hip: slab_pass)
// and the CPU checks call the same rules with the same arguments.
constexpr int kRuleSymbol = -2, kRuleHip = -3, kRuleIo = -5;   // IMC_ERR_SYMBOL, IMC_ERR_HIP, IMC_ERR_IO

inline IoResult rule_declines() { return io_fail(kSlabDeclined, std::string()); }

// A text file's pass: what the host carries from slab to slab, and every rule that looks at it.
struct TextSession {
    uint64_t room;           // tokens the symbol buffer holds: the upper bound for the file's bytes
    uint64_t cols = 0;       // tokens of the slabs accepted so far

    explicit TextSession(uint64_t file_bytes) : room(max_tokens_in(file_bytes)) {}

    size_t cut(const uint8_t *buf, size_t fill, bool last) const { return slab_cut(buf, fill, last); }

    // all: the summary of the whole slab of n bytes behind the accepted ones.  Errors are the host parser's, in file order.
    IoResult accept(const IngestSummary &all, size_t n, const char *path)
    {
        const IngestVerdict v = ingest_verdict(all, (uint32_t)n);
        if (v.kind == kIngestDeclined) return rule_declines();
        if (v.kind == kIngestBadByte) return io_fail(kRuleIo, std::string("unexpected character in ") + path);
        if (v.kind == kIngestSymbol) return io_fail(kRuleSymbol, symbol_error_text(v.value, cols + v.column, v.at_end));
        cols += all.count;
        if (cols > room) return io_fail(kRuleHip, "ingest: more tokens than the file can hold");
        return IoResult();
    }
};

// ---- 2-bit cache and pairwise rule ---------------------------------------------------------------------
IMC_ING_HD inline uint32_t unpack2(const uint8_t *pk, uint32_t t) { return (pk[t >> 2] >> (2 * (t & 3))) & 3u; }

IMC_ING_HD inline bool pairwise_clean(uint8_t c)
{
    const uint8_t u = c & 0xdf;                       // ASCII upper-casing of letters
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

// scripts/prepare-alignments.py:99-105: 2 = either base not in ACGT (either case), 0 = equal, 1 = different
IMC_ING_HD inline uint32_t pairwise_symbol(uint8_t a, uint8_t b)
{
    if (!pairwise_clean(a) || !pairwise_clean(b)) return 2u;
    return ((a & 0xdf) == (b & 0xdf)) ? 0u : 1u;
}

}  // namespace imc
