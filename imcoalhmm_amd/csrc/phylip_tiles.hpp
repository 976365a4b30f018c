// phylip_tiles.hpp - the parallel form of reading a PHYLIP alignment (phylip_io.hpp), host-only: the parse as a function of
// single bytes plus an associative combine, the rule that says where a kept byte goes, and the stride-n offsets of the
// line table, so that the kernels (kernels_phylip.hpp) and the CPU check (tests/phylip_tiles_check.cpp) call the same code.
//
// THE MACHINE.  What a byte is depends on the byte, on the byte before it (a '\r' must be followed by '\n') and on where
// its line stands: at column 0, behind spaces only (BLANK), inside the line's first word (WORD), or behind the space that
// ended the first word (REST).  A line COUNTS once it has shown a printable byte - that is what str.strip() would keep -
// and the counted lines are numbered j = 0, 1, ...: j = 0 is the header line (the host parses it, the device drops it),
// 1 <= j <= n are the name lines, and line j belongs to record (j - 1) mod n.  In a name line the first word is the name
// and the printable bytes behind it are kept; in a later line every printable byte is kept; spaces, "\r" and "\n" never
// are.  Which of the three a line is follows from j and n, so it is NOT part of the state: a range of bytes is summarised
// (PhySummary) as a function of the state it is entered in - the state behind it, the lines that start in it, and for
// the line that is open behind it the printable bytes (P) and the first-word bytes (W) it has seen since the range's last
// line break or its start - and summaries of adjacent ranges combine associatively (phy_combine).  Once the scan has
// given a range its cursor (state, counted lines, P and W of the open line), phy_advance says for every byte whether it
// is kept, a name byte or nothing, and at which place of its line's kept bytes (of its name) it stands.
//
// THE LINE TABLE.  cnt[j] = kept bytes of line j, summed by the tiles (integer additions: the order does not matter).
// off[j] = kept bytes of the record in front of line j = off[j - n] + cnt[j - n], 0 for j <= n: a scan with stride n
// (phy_chain_partial, phy_chain_walk), done per slab for the lines that started in it - line j - n has ended by then.  A
// kept byte of line j at place p of its line goes to record (j - 1) mod n at off[j] + p, and only if that is below the
// header's length: nothing is ever written outside the n * length bytes.
//
// The device parser takes: lines that end in "\n" or "\r\n" (the last one may end with the file); a header of two
// digit-only words separated and surrounded by spaces only; name lines that start at column 0 with a name of the bytes
// 0x21-0x7e, followed by nothing or by spaces and then bytes 0x21-0x7e and spaces; later lines of the bytes 0x21-0x7e and
// spaces; empty lines and lines of spaces only anywhere.  It DECLINES - the file is then read by imc::read_phylip from
// its start, which also words every error - a tab or any other control byte, a lone '\r', a byte >= 0x80, a space in
// front of a name, a third header word, a header line that does not end inside the first slab, n == 0, n >
// kMaxAlnRecords, n * length larger than the file, length >= 2^31 (no chunk is that long), a name longer than kPhyNameMax - 1, a repeated name,
// fewer than n name lines, a record whose kept bytes differ from length, and more than kPhyMaxLines counted lines.
//
// SLABS.  A slab may be cut anywhere - inside a name, between '\r' and '\n' - because the name bytes themselves are
// written by the device (n x kPhyNameMax bytes) and the cursor at the end of slab k (PhyTotal) is read back and passed to
// slab k + 1.  Only the header line must end inside the first slab.
#pragma once

#include <cstddef>
#include <cstdint>
#include <set>
#include <string>
#include <vector>

#include "align_tiles.hpp"
#include "phylip_io.hpp"

namespace imc {

enum PhyState : uint32_t { kPhyCol0 = 0, kPhyBlank = 1, kPhyWord = 2, kPhyRest = 3 };
constexpr uint32_t kPhyStates = 4;
enum PhyClass : uint32_t { kPhyBreak = 0, kPhyDropped = 1, kPhyFirst = 2, kPhyLater = 3 };   // First: in the first word
constexpr uint32_t kPhyNameMax = 256;             // bytes of a row of the name table; a name of 256 bytes or more declines
constexpr uint32_t kPhyMaxLines = 1u << 24;       // counted lines the line table holds at most; more declines
enum PhyFlag : uint32_t { kPhyFlagNameSpace = 1, kPhyFlagOutside = 2, kPhyFlagLines = 4 };   // declines the scatter raises

struct PhyStep {
    uint32_t next, cls, decline;
};

// Byte ch in `state`, prev the byte before it ('\n' in front of the file).
IMC_ING_HD IMC_ALN_FLAT inline PhyStep phy_step(uint32_t state, uint8_t prev, uint8_t ch)
{
    const uint32_t lone_cr = prev == '\r' && ch != '\n' ? 1u : 0u;
    if (ch == '\n') return PhyStep{kPhyCol0, kPhyBreak, 0u};
    if (ch == '\r') return PhyStep{state, kPhyDropped, lone_cr};
    if (ch == ' ') return PhyStep{state == kPhyCol0 || state == kPhyBlank ? (uint32_t)kPhyBlank : (uint32_t)kPhyRest, kPhyDropped, lone_cr};
    if (!aln_base_byte(ch)) return PhyStep{state, kPhyDropped, 1u};
    if (state == kPhyRest) return PhyStep{kPhyRest, kPhyLater, lone_cr};
    return PhyStep{kPhyWord, kPhyFirst, lone_cr};
}

// ---- the cursor: what is known in front of a byte once the scan has run -------------------------------------------
struct PhyCursor {
    uint32_t state;
    uint32_t lines;      // counted lines that have started (the open line, if it counts, is line `lines - 1`)
    uint32_t P, W;       // printable bytes and first-word bytes of the open line so far
};

enum PhyKind : uint32_t { kPhyNothing = 0, kPhyKeptByte = 1, kPhyNameByte = 2 };
struct PhyPlace {
    uint32_t kind;       // PhyKind
    uint32_t j;          // the byte's line (kinds 1 and 2)
    uint32_t pos;        // its place among the line's kept bytes (kind 1) or in the name (kind 2)
    uint32_t decline;    // the byte itself is not taken (phy_step)
    uint32_t flag;       // kPhyFlagNameSpace: a name that does not start at column 0
};

// Byte ch at the cursor, which moves behind it; n: the header's record count (0 in a summary, where only the cursor
// counts).
IMC_ING_HD IMC_ALN_FLAT inline PhyPlace phy_advance(PhyCursor &c, uint8_t prev, uint8_t ch, uint32_t n)
{
    const PhyStep st = phy_step(c.state, prev, ch);
    PhyPlace out{kPhyNothing, 0u, 0u, st.decline, 0u};
    if (st.cls == kPhyBreak) {
        c.P = c.W = 0u;
    } else if (st.cls == kPhyFirst || st.cls == kPhyLater) {
        const bool starts = c.state == kPhyCol0 || c.state == kPhyBlank;
        if (starts) ++c.lines;
        const uint32_t j = c.lines - 1u;
        out.j = j;
        if (j >= 1u && j <= n) {
            if (starts && c.state == kPhyBlank) out.flag = kPhyFlagNameSpace;
            out.kind = st.cls == kPhyFirst ? kPhyNameByte : kPhyKeptByte;
            out.pos = st.cls == kPhyFirst ? c.W : c.P - c.W;
        } else if (j > n) {
            out.kind = kPhyKeptByte;
            out.pos = c.P;
        }
        ++c.P;
        c.W += st.cls == kPhyFirst ? 1u : 0u;
    }
    c.state = st.next;
    return out;
}

// ---- summary of a range of bytes, as a function of the state it is entered in -------------------------------------
struct PhySummary {
    uint32_t map;                  // bits 2 e, 2 e + 1: the state behind the range; bit 8: it declines; bit 9: it holds a '\n'
    uint32_t lines[kPhyStates];    // counted lines that start in it
    uint32_t P[kPhyStates];        // of the line open behind it, since the range's last '\n' or its start
    uint32_t W[kPhyStates];
};

constexpr uint32_t kPhyIdentityMap = 0u | 1u << 2 | 2u << 4 | 3u << 6;
constexpr uint32_t kPhyMapDecline = 1u << 8, kPhyMapBreak = 1u << 9;

IMC_ING_HD IMC_ALN_FLAT inline uint32_t phy_exit(uint32_t map, uint32_t entry) { return (map >> (2u * entry)) & 3u; }

// v[x] without indexing a register array by a run-time value
IMC_ING_HD IMC_ALN_FLAT inline uint32_t phy_pick(const uint32_t (&v)[kPhyStates], uint32_t x) { return x == 0 ? v[0] : x == 1 ? v[1] : x == 2 ? v[2] : v[3]; }

IMC_ING_HD inline PhySummary phy_identity()
{
    PhySummary s;
    s.map = kPhyIdentityMap;
    for (uint32_t e = 0; e < kPhyStates; ++e) s.lines[e] = s.P[e] = s.W[e] = 0u;
    return s;
}

// a followed by b, the maps alone
IMC_ING_HD inline uint32_t phy_compose(uint32_t a, uint32_t b)
{
    uint32_t r = (a | b) & (kPhyMapDecline | kPhyMapBreak);
    for (uint32_t e = 0; e < kPhyStates; ++e) r |= phy_exit(b, phy_exit(a, e)) << (2u * e);
    return r;
}

// a followed by b
IMC_ING_HD inline PhySummary phy_combine(const PhySummary &a, const PhySummary &b)
{
    PhySummary r;
    r.map = phy_compose(a.map, b.map);
    const bool cut = (b.map & kPhyMapBreak) != 0u;
    for (uint32_t e = 0; e < kPhyStates; ++e) {
        const uint32_t x = phy_exit(a.map, e);
        r.lines[e] = a.lines[e] + phy_pick(b.lines, x);
        r.P[e] = (cut ? 0u : a.P[e]) + phy_pick(b.P, x);
        r.W[e] = (cut ? 0u : a.W[e]) + phy_pick(b.W, x);
    }
    return r;
}

// The summary of the n bytes at p; prev is the byte before them.
IMC_ING_HD inline PhySummary phy_range(const uint8_t *p, uint8_t prev, uint32_t n)
{
    PhySummary s;
    s.map = 0u;
    for (uint32_t e = 0; e < kPhyStates; ++e) {
        PhyCursor c{e, 0u, 0u, 0u};
        uint32_t flags = 0u;
        uint8_t before = prev;
        for (uint32_t i = 0; i < n; ++i) {
            const PhyPlace pl = phy_advance(c, before, p[i], 0u);
            flags |= (pl.decline ? kPhyMapDecline : 0u) | (p[i] == '\n' ? kPhyMapBreak : 0u);
            before = p[i];
        }
        s.map |= c.state << (2u * e) | flags;
        s.lines[e] = c.lines;
        s.P[e] = c.P;
        s.W[e] = c.W;
    }
    return s;
}

// ---- a run of tiles whose entry states are known: what the one-workgroup scan adds up ------------------------------
struct PhyRun {
    uint32_t lines, P, W;
    uint32_t flags;                // kPhyMapDecline | kPhyMapBreak
};

IMC_ING_HD inline PhyRun phy_run_of(const PhySummary &s, uint32_t entry)
{
    return PhyRun{phy_pick(s.lines, entry), phy_pick(s.P, entry), phy_pick(s.W, entry), s.map & (kPhyMapDecline | kPhyMapBreak)};
}

IMC_ING_HD inline PhyRun phy_run_combine(const PhyRun &a, const PhyRun &b)
{
    const bool cut = (b.flags & kPhyMapBreak) != 0u;
    return PhyRun{a.lines + b.lines, (cut ? 0u : a.P) + b.P, (cut ? 0u : a.W) + b.W, a.flags | b.flags};
}

// The cursor behind a run that is entered at `at` and leaves in `state`.
IMC_ING_HD inline PhyCursor phy_cursor_behind(const PhyCursor &at, const PhyRun &run, uint32_t state)
{
    const bool cut = (run.flags & kPhyMapBreak) != 0u;
    return PhyCursor{state, at.lines + run.lines, (cut ? 0u : at.P) + run.P, (cut ? 0u : at.W) + run.W};
}

// What a slab reports: the cursor behind it and whether a byte of it declines.
struct PhyTotal {
    PhyCursor end;
    uint32_t decline;
    uint32_t flags;                // PhyFlag bits the scatter raised, in this slab or an earlier one
    uint32_t pad[2];
};

// ---- the line table: offsets with stride n -------------------------------------------------------------------------
// The lines j0 .. j0 + m - 1 started in the slab.  Chain c (0 <= c < n) holds the lines j0 + c + k n, k = 0, 1, ...; its
// rows are cut into pieces of `rows` each, and piece q of chain c is one unit of work.
IMC_ING_HD inline uint32_t phy_chain_partial(const uint32_t *cnt, uint32_t j0, uint32_t m, uint32_t n, uint32_t rows, uint32_t q, uint32_t c)
{
    uint32_t sum = 0;
    for (uint32_t k = q * rows; k < (q + 1u) * rows && (uint64_t)c + (uint64_t)k * n < m; ++k) sum += cnt[j0 + c + k * n];
    return sum;
}

// part[q' n + c]: phy_chain_partial of the pieces; writes off[] of piece q of chain c.
IMC_ING_HD inline void phy_chain_walk(const uint32_t *cnt, uint32_t *off, const uint32_t *part, uint32_t j0, uint32_t m, uint32_t n, uint32_t rows, uint32_t q,
                                      uint32_t c)
{
    if ((uint64_t)c + (uint64_t)q * rows * n >= m) return;
    const uint32_t first = j0 + c;                                       // the chain's first line of this slab
    uint32_t acc = first <= n ? 0u : off[first - n] + cnt[first - n];   // (line first - n started in an earlier slab)
    for (uint32_t p = 0; p < q; ++p) acc += part[p * n + c];
    for (uint32_t k = q * rows; k < (q + 1u) * rows && (uint64_t)c + (uint64_t)k * n < m; ++k) {
        const uint32_t j = first + k * n;
        off[j] = acc;
        acc += cnt[j];
    }
}

// Rows per piece for at most m_max lines in n chains: about the square root of the rows, so that the partial sums and
// the walk are equally long.
inline uint32_t phy_chain_rows(uint64_t m_max, uint32_t n)
{
    const uint64_t rows = m_max / n + 1u;
    uint32_t r = 1;
    while ((uint64_t)r * r < rows) ++r;
    return r;
}

inline uint32_t phy_chain_pieces(uint64_t m_max, uint32_t n, uint32_t rows) { return (uint32_t)((m_max / n + 1u + rows - 1u) / rows); }

// ---- what the host decides ----------------------------------------------------------------------------------------
// The header from the first slab's bytes.  false: the device parser declines (no counted line that ends inside these
// bytes - unless the file ends with them - or a header it does not take, or one the host reader calls an error).
inline bool phy_first_slab_header(const uint8_t *buf, size_t n, bool at_eof, uint64_t file_bytes, PhylipHeader &h)
{
    size_t a = 0;
    while (a < n) {                                                       // the first line with a byte that counts
        size_t b = a;
        bool counts = false;
        while (b < n && buf[b] != '\n') counts |= !fasta_space(buf[b++]);
        if (counts) {
            if (b == n && !at_eof) return false;
            if (phylip_header(buf + a, b - a, "", h).code) return false;
            if (h.words != 2 || h.n > kMaxAlnRecords || h.length > 0x7fffffffull) return false;
            return h.length <= file_bytes / h.n;                          // n * length <= file bytes, without overflow
        }
        a = b + 1;
    }
    return false;
}

// The limits of the device parser (the CPU check runs with smaller ones).
struct PhyLimits {
    uint32_t cap_lines = kPhyMaxLines;
    uint32_t name_max = kPhyNameMax;
};

// What is sized from the header: the shape of the offsets' pieces, and the bytes of the four buffers.
struct PhySizes {
    uint32_t rows, pieces;
    size_t bases, names, nlen, part;
};

// A PHYLIP file's pass: what the host carries from slab to slab, and every rule that looks at it (answers: ingest_tiles.hpp).
struct PhySession {
    const PhyLimits lim;
    const uint64_t file_bytes;
    const uint32_t cap;              // lines the line table holds (a counted line behind another takes two bytes)
    PhyCursor at{kPhyCol0, 0u, 0u, 0u};   // the next slab is entered at it
    uint32_t prev = '\n';            // the byte in front of the next slab
    uint32_t nrec = 0, length = 0;   // the header's
    bool begun = false;

    explicit PhySession(uint64_t bytes, const PhyLimits &limits = PhyLimits())
        : lim(limits), file_bytes(bytes), cap((uint32_t)(bytes / 2 + 2 < limits.cap_lines ? bytes / 2 + 2 : limits.cap_lines))
    {
    }

    // The first slab (its `cut` bytes at `first`, of slabs of at most `slab` bytes): the header, and what is sized from it
    // (record r at r * length).
    IoResult begin(const uint8_t *first, size_t cut, bool at_eof, size_t slab, PhySizes &sz)
    {
        const uint64_t lines_max = slab / 2 + 2;                          // lines that can start in one slab
        PhylipHeader header;
        if (!phy_first_slab_header(first, cut, at_eof, file_bytes, header)) return rule_declines();
        begun = true;
        nrec = (uint32_t)header.n;
        length = (uint32_t)header.length;
        sz.rows = phy_chain_rows(lines_max, nrec);
        sz.pieces = phy_chain_pieces(lines_max, nrec, sz.rows);
        const uint64_t all = ((uint64_t)nrec * length + 15) & ~(uint64_t)15;
        sz.bases = (size_t)(all < 16 ? 16 : all);
        sz.names = (size_t)nrec * lim.name_max;
        sz.nlen = (size_t)nrec * sizeof(uint32_t);
        sz.part = (size_t)sz.pieces * nrec * sizeof(uint32_t);
        return IoResult();
    }

    // t: the total of the slab behind the accepted ones, whose last byte is last_byte.
    IoResult accept(const PhyTotal &t, uint8_t last_byte)
    {
        // (an open line far beyond the header's length cannot belong to a record of that length: its counters stay 32-bit)
        if (t.decline || t.flags || t.end.lines > cap || t.end.P > (uint64_t)length + lim.name_max) return rule_declines();
        at = t.end;
        prev = last_byte;
        return IoResult();
    }

    // Behind the last slab: a file without a slab or with fewer than n name lines declines; else `line` is the first of the
    // last n lines of the line table, which hold one line of every record.
    IoResult tail(uint32_t &line) const
    {
        if (!begun || at.lines < (uint64_t)nrec + 1) return rule_declines();
        line = at.lines - nrec;
        return IoResult();
    }

    // name_len[r], the lim.name_max bytes at name_bytes + r * lim.name_max: record r's name as the device wrote it;
    // tail_cnt, tail_off: cnt[] and off[] of the n lines from tail()'s line on.  Every record's kept bytes must be the
    // header's length, every name must fit its row and stand once.
    IoResult finish(const uint32_t *name_len, const char *name_bytes, const uint32_t *tail_cnt, const uint32_t *tail_off, std::vector<std::string> &names,
                    std::vector<uint64_t> &start, std::vector<uint64_t> &lengths) const
    {
        std::set<std::string> seen;
        for (uint32_t r = 0; r < nrec; ++r) {
            if ((uint64_t)tail_off[r] + tail_cnt[r] != length || name_len[r] == 0 || name_len[r] >= lim.name_max) return rule_declines();
            names.emplace_back(name_bytes + (size_t)r * lim.name_max, name_len[r]);
            start.push_back((uint64_t)r * length);
            lengths.push_back(length);
            if (!seen.insert(names.back()).second) return rule_declines();
        }
        return IoResult();
    }
};

}  // namespace imc
