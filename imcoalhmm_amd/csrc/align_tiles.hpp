// align_tiles.hpp - the parallel form of reading a FASTA alignment (fasta_io.hpp), host-only: the parse as a function of
// single bytes plus an associative combine, the slab rule, and the column rules that turn resident sequences into a
// chunk's symbols, so that the kernels (kernels_align.hpp) and the CPU check (tests/align_tiles_check.cpp) call the same
// code.
//
// What a byte is - a line break, a header byte, a sequence byte that is kept, or a byte that is dropped - depends on the
// byte, on the byte before it (a '\r' must be followed by '\n') and on one small STATE: at the start of a line, inside a
// header line, inside a sequence line; before the first header the same two line states exist once more (lines in front
// of the first header are ignored), which makes five.  A '\n' resets the state, so only the bytes of a range before its
// first '\n' depend on the state the range is entered in.  A range of bytes is summarised (AlnSummary) as a function of
// that entry state: the state it is left in, the sequence bytes it keeps, the headers that start in it and whether it
// asks to DECLINE the file; summaries of adjacent ranges combine associatively (aln_combine), like any transducer.
//
// The device parser takes: lines that end in "\n" or "\r\n" (the last one may end with the file), '>' at column 0
// followed by tabs and printable ASCII, sequence lines of the bytes 0x21-0x7e only, empty lines anywhere.  Everything
// else only raises the decline flag - any other whitespace or control byte in a sequence line, a lone '\r', whitespace in
// front of a '>', a byte >= 0x80 - and the file is then read by imc::read_fasta from its start, which also words every
// error.  The host adds three declines of its own from what the device reports: a header whose name is empty, more than
// kMaxAlnRecords records, a repeated name.  For a file that is not declined the kept bytes, record by record, are
// read_fasta's sequences.
//
// SLABS.  The file goes up in slabs (ingest_tiles.hpp: the slab size setting).  A slab may end anywhere in a sequence
// line - the state, the record count and the base count at its end are read back and passed to the next slab - but not
// inside a header line, whose name the host takes from the slab's bytes: aln_slab_cut cuts in front of that header's '>'
// and the tail is carried into the next slab.  A header line longer than a slab is declined.
#pragma once

#include <cstddef>
#include <cstdint>
#include <set>
#include <string>
#include <vector>

#include "fasta_io.hpp"
#include "ingest_tiles.hpp"

// the smallest helpers are inlined at every optimisation level (the CPU check is built with -O1 under sanitizers)
#define IMC_ALN_FLAT __attribute__((always_inline))

namespace imc {

// ---- the state machine -----------------------------------------------------------------------------------
enum AlnState : uint32_t {
    kAlnStart0 = 0,      // at the start of a line, no header seen yet
    kAlnJunk = 1,        // inside a line in front of the first header (ignored)
    kAlnStart = 2,       // at the start of a line
    kAlnHeader = 3,      // inside a header line
    kAlnSeq = 4          // inside a sequence line
};
constexpr uint32_t kAlnStates = 5;
enum AlnClass : uint32_t { kAlnBreak = 0, kAlnHeaderStart = 1, kAlnHeaderByte = 2, kAlnKept = 3, kAlnDropped = 4 };
constexpr uint32_t kMaxAlnRecords = 4096;

struct AlnStep {
    uint32_t next;       // state behind the byte
    uint32_t cls;        // AlnClass
    uint32_t decline;    // the device parser does not take this byte where it stands
};

IMC_ING_HD IMC_ALN_FLAT inline bool aln_base_byte(uint8_t ch) { return ch >= 0x21 && ch <= 0x7e; }

// Byte ch in `state`, prev the byte before it ('\n' in front of the file).
IMC_ING_HD IMC_ALN_FLAT inline AlnStep aln_step(uint32_t state, uint8_t prev, uint8_t ch)
{
    const uint32_t lone_cr = prev == '\r' && ch != '\n' ? 1u : 0u;
    const bool early = state == kAlnStart0 || state == kAlnJunk;
    if (ch == '\n') return AlnStep{early ? (uint32_t)kAlnStart0 : (uint32_t)kAlnStart, kAlnBreak, 0u};
    if (ch == '\r') return AlnStep{state, kAlnDropped, lone_cr};
    if (state == kAlnHeader) return AlnStep{kAlnHeader, kAlnHeaderByte, lone_cr | ((ch == '\t' || (ch >= 0x20 && ch <= 0x7e)) ? 0u : 1u)};
    if ((state == kAlnStart0 || state == kAlnStart) && ch == '>') return AlnStep{kAlnHeader, kAlnHeaderStart, lone_cr};
    const uint32_t bad = lone_cr | (aln_base_byte(ch) ? 0u : 1u);
    if (early) return AlnStep{kAlnJunk, kAlnDropped, bad};
    return AlnStep{kAlnSeq, kAlnKept, bad};
}

// ---- summary of a range of bytes, as a function of the state it is entered in ---------------------------------
struct AlnSummary {
    uint32_t map;                 // bits 3 e .. 3 e + 2: the state behind the range; bit 16 + e: it asks to decline
    uint32_t seq[kAlnStates];     // sequence bytes it keeps
    uint32_t hdr[kAlnStates];     // headers that start in it
};

constexpr uint32_t kAlnIdentityMap = 0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12;

IMC_ING_HD IMC_ALN_FLAT inline uint32_t aln_exit(uint32_t map, uint32_t entry) { return (map >> (3u * entry)) & 7u; }
IMC_ING_HD IMC_ALN_FLAT inline uint32_t aln_declines(uint32_t map, uint32_t entry) { return (map >> (16u + entry)) & 1u; }

// v[x] without indexing a register array by a run-time value
IMC_ING_HD IMC_ALN_FLAT inline uint32_t aln_pick(const uint32_t (&v)[kAlnStates], uint32_t x)
{
    return x == 0 ? v[0] : x == 1 ? v[1] : x == 2 ? v[2] : x == 3 ? v[3] : v[4];
}

IMC_ING_HD inline AlnSummary aln_identity()
{
    AlnSummary s;
    s.map = kAlnIdentityMap;
    for (uint32_t e = 0; e < kAlnStates; ++e) s.seq[e] = s.hdr[e] = 0u;
    return s;
}

// a followed by b, the maps alone
IMC_ING_HD inline uint32_t aln_compose(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (uint32_t e = 0; e < kAlnStates; ++e) {
        const uint32_t x = aln_exit(a, e);
        r |= aln_exit(b, x) << (3u * e) | (aln_declines(a, e) | aln_declines(b, x)) << (16u + e);
    }
    return r;
}

// a followed by b
IMC_ING_HD inline AlnSummary aln_combine(const AlnSummary &a, const AlnSummary &b)
{
    AlnSummary r;
    r.map = aln_compose(a.map, b.map);
    for (uint32_t e = 0; e < kAlnStates; ++e) {
        const uint32_t x = aln_exit(a.map, e);
        r.seq[e] = a.seq[e] + aln_pick(b.seq, x);
        r.hdr[e] = a.hdr[e] + aln_pick(b.hdr, x);
    }
    return r;
}

// The summary of the n bytes at p; prev is the byte before them.
IMC_ING_HD inline AlnSummary aln_range(const uint8_t *p, uint8_t prev, uint32_t n)
{
    AlnSummary s;
    s.map = 0u;
    for (uint32_t e = 0; e < kAlnStates; ++e) {
        uint32_t state = e, seq = 0, hdr = 0, decline = 0;
        uint8_t before = prev;
        for (uint32_t i = 0; i < n; ++i) {
            const AlnStep st = aln_step(state, before, p[i]);
            seq += st.cls == kAlnKept ? 1u : 0u;
            hdr += st.cls == kAlnHeaderStart ? 1u : 0u;
            decline |= st.decline;
            state = st.next;
            before = p[i];
        }
        s.map |= state << (3u * e) | decline << (16u + e);
        s.seq[e] = seq;
        s.hdr[e] = hdr;
    }
    return s;
}

// What a slab's summary says once the state it was entered in is known.
struct AlnTotal {
    uint32_t exit, seq, hdr, decline;
};

IMC_ING_HD inline AlnTotal aln_resolve(const AlnSummary &s, uint32_t entry)
{
    return AlnTotal{aln_exit(s.map, entry), aln_pick(s.seq, entry), aln_pick(s.hdr, entry), aln_declines(s.map, entry)};
}

// One record of the table the scatter writes: where its '>' stands in the slab, and the kept bytes in front of it.
struct AlnRecord {
    uint32_t slab_offset;
    uint32_t pad;
    uint64_t start;
};

// ---- slabs -------------------------------------------------------------------------------------------
// How many of the n buffered bytes form the next slab, entered in state `entry`: all of them at the end of the file or
// when the last line of the buffer is no header line, else everything in front of that header's '>'.  0 with n > 0: a
// header line longer than the buffer, the device parser declines the file.
inline size_t aln_slab_cut(const uint8_t *buf, size_t n, bool at_eof, uint32_t entry)
{
    if (at_eof || n == 0) return n;
    size_t line = n;
    while (line > 0 && buf[line - 1] != '\n') --line;
    if (line == n) return n;                                                        // the buffer ends with a line
    if (line == 0 && entry != kAlnStart0 && entry != kAlnStart) return n;           // one long line goes on
    return buf[line] == '>' ? line : n;
}

// ---- column rules --------------------------------------------------------------------------------------
// 0..3 for A, C, G, T in either case, 4 for every other byte
IMC_ING_HD inline uint32_t base_code(uint8_t c)
{
    const uint8_t u = c & 0xdf;                       // ASCII upper-casing of letters
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// scripts/prepare-alignments.py:134-146: i1 + 4 i2 + 16 i3, 64 when any of the three bases is not in ACGT (either case)
IMC_ING_HD inline uint32_t triplet_symbol(uint8_t a, uint8_t b, uint8_t c)
{
    const uint32_t i1 = base_code(a), i2 = base_code(b), i3 = base_code(c);
    return (i1 | i2 | i3) & 4u ? 64u : i1 + 4u * i2 + 16u * i3;
}

// Four columns from the aligned words lo and hi (hi: the word behind lo) of a sequence that starts `shift` bytes
// (0..3) into lo.
IMC_ING_HD inline uint32_t aln_unaligned_word(uint32_t lo, uint32_t hi, uint32_t shift)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift));
}

IMC_ING_HD inline uint32_t aln_load_word(const uint8_t *p)          // p is word aligned
{
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
    return w;
}

constexpr uint32_t kAlnColumns = 16;     // columns one thread of the column kernel makes: one 16-byte store

// Columns col0 .. col0 + 15 (col0 a multiple of 16, below L) of the sequence of L bytes that starts at bases + start, as
// four words; bases is word aligned, start is not.  Only aligned words are loaded, and only those whose first byte lies
// in front of the sequence's end: what a word holds beyond that end is never used by the callers (aln_symbols).
IMC_ING_HD inline void aln_gather(const uint8_t *bases, uint64_t start, uint32_t col0, uint32_t L, uint32_t (&out)[4])
{
    const uint64_t off = start + col0, end = start + L;
    const uint32_t shift = (uint32_t)(off & 3u);
    const uint64_t word0 = off - shift;
    uint32_t wd[5];
    for (uint32_t j = 0; j < 5; ++j) wd[j] = word0 + 4u * j < end ? aln_load_word(bases + word0 + 4u * j) : 0u;
    for (uint32_t j = 0; j < 4; ++j) out[j] = aln_unaligned_word(wd[j], wd[j + 1], shift);
}

// The symbols of four columns (the first `valid` of them exist; the others are written as zeros) of K = 2 or 3 sequences.
template <int K>
IMC_ING_HD inline uint32_t aln_symbols(uint32_t a, uint32_t b, uint32_t c, uint32_t valid)
{
    static_assert(K == 2 || K == 3, "pairs and triplets");
    uint32_t word = 0;
    for (uint32_t k = 0; k < 4; ++k)
        if (k < valid) {
            const uint8_t x = (uint8_t)(a >> 8 * k), y = (uint8_t)(b >> 8 * k), z = (uint8_t)(c >> 8 * k);
            word |= (K == 2 ? pairwise_symbol(x, y) : triplet_symbol(x, y, z)) << 8 * k;
        }
    return word;
}

// The name of the header whose '>' stands at slab[at] (n: the slab's bytes), as the host takes it from the staged slab.
inline std::string aln_header_name(const uint8_t *slab, size_t n, size_t at)
{
    size_t end = ++at;
    while (end < n && slab[end] != '\n' && slab[end] != '\r') ++end;
    return fasta_first_word(slab + at, end - at);
}

// ---- what the host decides ------------------------------------------------------------------------------------
// A FASTA file's pass: what the host carries from slab to slab, and every rule that looks at it (answers: ingest_tiles.hpp).
struct AlnSession {
    uint32_t state = kAlnStart0;     // the next slab is entered in it
    uint32_t prev = '\n';            // the byte in front of the next slab
    uint64_t kept = 0;               // bases of the slabs accepted so far
    std::vector<std::string> names;  // of the records so far
    std::vector<uint64_t> start;     // ... and the kept bytes in front of each

    size_t cut(const uint8_t *buf, size_t fill, bool last) const { return aln_slab_cut(buf, fill, last, state); }

    // t: the total of the slab (its `cut` bytes at `slab`) behind the accepted ones; room: the bases the buffer holds.
    // fetch(first, count, recs) points recs at the records first .. first + count - 1 of the scatter's table and answers as a
    // rule does; it is asked only for a slab that is not declined and holds a header.
    template <class Fetch>
    IoResult accept(const AlnTotal &t, Fetch &&fetch, const uint8_t *slab, size_t cut, uint64_t room)
    {
        if (t.decline || (uint64_t)names.size() + t.hdr > kMaxAlnRecords) return rule_declines();
        if (kept + t.seq > room) return io_fail(kRuleHip, "alignment: more bases than the file can hold");
        if (t.hdr) {                                                    // the names, from the slab's bytes
            const AlnRecord *recs = nullptr;
            const IoResult fetched = fetch((uint32_t)names.size(), t.hdr, recs);
            if (fetched.code) return fetched;
            for (uint32_t k = 0; k < t.hdr; ++k) {
                const size_t at = (size_t)recs[k].slab_offset + 1;
                if (at > cut || recs[k].start > kept + t.seq) return io_fail(kRuleHip, "alignment: a header outside its slab");
                std::string name = aln_header_name(slab, cut, at - 1);
                if (name.empty()) return rule_declines();
                names.push_back(std::move(name));
                start.push_back(recs[k].start);
            }
        }
        kept += t.seq;
        state = t.exit;
        prev = slab[cut - 1];
        return IoResult();
    }

    // Behind the last slab: a repeated name declines; else every record's length, from the starts.
    IoResult finish(std::vector<uint64_t> &length) const
    {
        if (std::set<std::string>(names.begin(), names.end()).size() != names.size()) return rule_declines();
        for (size_t k = 0; k < start.size(); ++k) length.push_back((k + 1 < start.size() ? start[k + 1] : kept) - start[k]);
        return IoResult();
    }
};

}  // namespace imc
