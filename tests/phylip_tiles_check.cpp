// phylip_tiles_check.cpp - the parallel form of reading a PHYLIP alignment (csrc/phylip_tiles.hpp) against the host reader
// imc::read_phylip (csrc/phylip_io.hpp), on the CPU.  The functions the PHYLIP kernels call are driven here sequentially,
// the way the device path runs them: the file goes through the product's own loop (imc::slab_stream, cut anywhere) under
// the product's own rules (imc::PhySession: the header and the sizes from the first slab, the verdict on every slab's
// total, the last n lines and the names behind the last slab), and per slab the six launches - a summary per tile, folded
// from single positions with phy_combine (and equal to phy_range over the tile); one scan that gives every tile its cursor
// from the cursor the slab is entered at; the line counts; the stride-n offsets in pieces of a few rows (phy_chain_partial,
// phy_chain_walk); then every tile (in reverse order here: they are independent) walks its bytes from its own cursor
// alone, compacts its kept bytes line by line the way k_phy_scatter does (first place, count and the place-minus-index of
// every line of the tile) and writes every line's run at its record's offset if it ends inside the record.
//   (a) every string up to length 6 over {'1', 'a', ' ', '\n', '\r', '\t', 0x80}, bare and behind the header "2 1\n" and
//       behind "1 2\nx ": tile sizes 1 and 3, the whole file as one slab and slabs of 1, 2 and 3 bytes
//   (b) generated files of the shapes the device parser takes (one line per record, interleaved at several widths, blocks
//       and records of unequal widths, groups separated by spaces, blank and spaces-only lines, "\r\n", padded names,
//       name-only name lines, no final line break, long names): every slab size from 1 to a few tiles at tile sizes 1, 2,
//       3, 7, 16 and 64 - so every cut inside a name, inside the header's line break and inside "\r\n" occurs - must NOT
//       decline; the same with one byte replaced, inserted or removed must decline or agree
//   (c) hand-written files: each decline is raised for the file it is meant for
//   In every case: not declined implies exactly read_phylip's records (names, order, bases); an error of read_phylip
//   implies declined; no byte is written outside n * length (the buffer is exactly that long, under AddressSanitizer).
// Built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../imcoalhmm_amd/csrc/phylip_tiles.hpp"
#include "../imcoalhmm_amd/csrc/slab_stream.hpp"

static long g_compared = 0, g_declined = 0, g_taken = 0;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 1) {}
    uint32_t next()
    {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        return (uint32_t)(s >> 16);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

typedef std::vector<uint8_t> Bytes;

static Bytes bytes_of(const std::string &s) { return Bytes(s.begin(), s.end()); }

struct Parsed {
    bool declined = false;
    std::vector<std::string> names, seqs;
};

static bool same_summary(const imc::PhySummary &a, const imc::PhySummary &b)
{
    if (a.map != b.map) return false;
    for (uint32_t e = 0; e < imc::kPhyStates; ++e)
        if (a.lines[e] != b.lines[e] || a.P[e] != b.P[e] || a.W[e] != b.W[e]) return false;
    return true;
}

// ---- the device path, sequentially ------------------------------------------------------------------------------
struct Device {
    uint32_t tile;
    const imc::PhySession *ses;      // the product's session: what the launches get as arguments comes from it
    imc::PhySizes sz;                // ... and from what its begin() sized
    Bytes bases, names;
    std::vector<uint32_t> cnt, off, nlen;
    uint32_t flags = 0;
    imc::PhyTotal total;             // what the slab reports

    // one slab
    void slab(const uint8_t *buf, uint32_t len)
    {
        const imc::PhyCursor at = ses->at;
        const uint8_t prev = (uint8_t)ses->prev;
        const uint32_t n = ses->nrec, length = ses->length, cap = ses->cap, name_max = ses->lim.name_max;
        const uint32_t tiles = (len + tile - 1) / tile;
        auto byte_before = [&](uint32_t i) { return i ? buf[i - 1] : prev; };
        // summary
        std::vector<imc::PhySummary> sums(tiles);
        for (uint32_t t = 0; t < tiles; ++t) {
            const uint32_t lo = t * tile, hi = std::min(len, lo + tile);
            imc::PhySummary s = imc::phy_identity();
            for (uint32_t i = lo; i < hi; ++i) s = imc::phy_combine(s, imc::phy_range(buf + i, byte_before(i), 1));
            CHECK(same_summary(s, imc::phy_range(buf + lo, byte_before(lo), hi - lo)));
            sums[t] = s;
        }
        // scan
        std::vector<imc::PhyCursor> tile_in(tiles);
        uint32_t map = imc::kPhyIdentityMap;
        imc::PhyRun run{0u, 0u, 0u, 0u};
        for (uint32_t t = 0; t < tiles; ++t) {
            const uint32_t state = imc::phy_exit(map, at.state);
            tile_in[t] = imc::phy_cursor_behind(at, run, state);
            map = imc::phy_compose(map, sums[t].map);
            run = imc::phy_run_combine(run, imc::phy_run_of(sums[t], state));
        }
        const imc::PhyCursor end = imc::phy_cursor_behind(at, run, imc::phy_exit(map, at.state));
        const bool decline = (run.flags & imc::kPhyMapDecline) != 0u;
        // count (the kernel's cursor knows the state and the lines only)
        for (uint32_t t = tiles; t-- > 0;) {
            imc::PhyCursor c{tile_in[t].state, tile_in[t].lines, 0u, 0u};
            for (uint32_t i = t * tile; i < std::min(len, (t + 1) * tile); ++i) {
                const imc::PhyPlace pl = imc::phy_advance(c, byte_before(i), buf[i], n);
                if (pl.kind == imc::kPhyKeptByte && pl.j < cap) ++cnt[pl.j];
                if (pl.kind == imc::kPhyNameByte) ++nlen[pl.j - 1];
            }
        }
        // offsets of the lines that started in the slab, in pieces of `rows` rows
        const uint32_t j0 = at.lines, j1 = std::min(end.lines, cap), m = j1 > j0 ? j1 - j0 : 0u;
        const uint32_t m_max = len / 2 + 2;
        CHECK(m <= m_max);
        const uint32_t rows = sz.rows, pieces = sz.pieces;
        CHECK((uint64_t)rows * pieces * n >= m_max);
        std::vector<uint32_t> part(sz.part / sizeof(uint32_t));
        for (uint32_t q = 0; q < pieces; ++q)
            for (uint32_t c = 0; c < n; ++c) part[(size_t)q * n + c] = imc::phy_chain_partial(cnt.data(), j0, m, n, rows, q, c);
        for (uint32_t q = pieces; q-- > 0;)
            for (uint32_t c = 0; c < n; ++c) imc::phy_chain_walk(cnt.data(), off.data(), part.data(), j0, m, n, rows, q, c);
        for (uint32_t j = std::max(j0, 1u); j < j1; ++j) CHECK(off[j] == (j <= n ? 0u : off[j - n] + cnt[j - n]));
        // scatter
        for (uint32_t t = tiles; t-- > 0;) {
            const imc::PhyCursor in = tile_in[t];
            imc::PhyCursor c = in;
            const uint32_t nseg = tile / 2 + 2;
            std::vector<uint32_t> seg_start(nseg, 0xffffffffu), seg_cnt(nseg, 0u), seg_rel(nseg, 0u);
            Bytes stage(tile);
            uint32_t k = 0;
            for (uint32_t i = t * tile; i < std::min(len, (t + 1) * tile); ++i) {
                const imc::PhyPlace pl = imc::phy_advance(c, byte_before(i), buf[i], n);
                flags |= pl.flag;
                if (pl.kind == imc::kPhyNameByte) {
                    if (pl.pos < name_max) names[(size_t)(pl.j - 1) * name_max + pl.pos] = buf[i];
                } else if (pl.kind == imc::kPhyKeptByte) {
                    const uint32_t s = pl.j + 1u - in.lines;
                    CHECK(s < nseg && k < tile);
                    stage[k] = buf[i];
                    if (seg_cnt[s]) CHECK(seg_rel[s] == pl.pos - k);
                    seg_start[s] = std::min(seg_start[s], k);
                    seg_rel[s] = pl.pos - k;
                    ++seg_cnt[s];
                    ++k;
                }
            }
            CHECK(c.lines - in.lines + 1u <= nseg);
            for (uint32_t s = 0; s < nseg; ++s) {
                if (!seg_cnt[s]) continue;
                CHECK(in.lines + s >= 2u);
                const uint32_t j = in.lines + s - 1u;
                if (j >= cap) { flags |= imc::kPhyFlagLines; continue; }
                const uint64_t first = (uint64_t)off[j] + (uint32_t)(seg_rel[s] + seg_start[s]);
                if (first + seg_cnt[s] > length) { flags |= imc::kPhyFlagOutside; continue; }
                const uint64_t dest0 = (uint64_t)((j - 1u) % n) * length + first;
                for (uint32_t b = 0; b < seg_cnt[s]; ++b) bases.at((size_t)(dest0 + b)) = stage[seg_start[s] + b];
            }
        }
        total = imc::PhyTotal{end, decline ? 1u : 0u, flags, {0u, 0u}};
    }
};

static Parsed device_parse(const Bytes &d, size_t slab_bytes, uint32_t tile, uint32_t cap_lines = 1u << 20, uint32_t name_max = imc::kPhyNameMax)
{
    Parsed out;
    imc::PhySession ses(d.size(), imc::PhyLimits{cap_lines, name_max});    // the product's rules, with the arguments the engine passes
    Device dev;
    dev.tile = tile;
    dev.ses = &ses;
    Bytes h0(slab_bytes), h1(slab_bytes);
    uint8_t *const host[2] = {h0.data(), h1.data()};
    size_t pos = 0;
    bool at_eof = false;
    uint64_t slabs = 0;
    const int end = imc::slab_stream(
        host, slab_bytes,
        [&](uint8_t *dst, size_t want, bool &eof) {
            const size_t got = std::min(want, d.size() - pos);
            if (got) std::memcpy(dst, d.data() + pos, got);
            pos += got;
            if (pos == d.size()) eof = true;
            return got;
        },
        [&](const uint8_t *, size_t fill, bool last) { at_eof = last; return fill; },
        [&](int cur, size_t cut) -> int {
            if (!slabs) {
                if (ses.begin(host[cur], cut, at_eof, slab_bytes, dev.sz).code) return imc::kSlabDeclined;
                CHECK(dev.sz.bases >= (size_t)ses.nrec * ses.length && dev.sz.bases % 16 == 0);
                dev.bases.assign((size_t)ses.nrec * ses.length, 0);       // exactly n * length: any write outside is caught
                dev.names.assign(dev.sz.names, 0);
                dev.nlen.assign(dev.sz.nlen / sizeof(uint32_t), 0);
                dev.cnt.assign(ses.cap, 0);
                dev.off.assign(ses.cap, 0xdeadbeefu);
            }
            ++slabs;
            dev.slab(host[cur], (uint32_t)cut);
            return imc::kSlabDone;
        },
        [&](int cur, size_t cut) -> int { return ses.accept(dev.total, host[cur][cut - 1]).code; });
    uint32_t line = 0;
    if (end == imc::kSlabDeclined || ses.tail(line).code) { out.declined = true; return out; }
    CHECK(end == imc::kSlabDone && slabs > 0);
    std::vector<uint64_t> start, length;
    if (ses.finish(dev.nlen.data(), reinterpret_cast<const char *>(dev.names.data()), dev.cnt.data() + line, dev.off.data() + line, out.names, start, length).code) {
        out.declined = true;
        return out;
    }
    for (uint32_t r = 0; r < ses.nrec; ++r) out.seqs.emplace_back(reinterpret_cast<const char *>(dev.bases.data()) + start[r], length[r]);
    return out;
}

// Device against host on one file at one geometry; returns whether the device took it.
static bool compare(const Bytes &d, size_t slab_bytes, uint32_t tile, uint32_t cap_lines = 1u << 20, uint32_t name_max = imc::kPhyNameMax)
{
    imc::FastaRecords want;
    const imc::IoResult r = imc::read_phylip_bytes(d.data(), d.size(), "file", want);
    const Parsed got = device_parse(d, slab_bytes, tile, cap_lines, name_max);
    ++g_compared;
    if (r.code) CHECK(got.declined);
    if (got.declined) { ++g_declined; return false; }
    ++g_taken;
    CHECK(!r.code);
    CHECK(got.names == want.names);
    CHECK(got.seqs == want.seqs);
    return true;
}

// ---- (a) all short strings -----------------------------------------------------------------------------------------
static void all_short_strings()
{
    const uint8_t alphabet[] = {'1', 'a', ' ', '\n', '\r', '\t', 0x80};
    const char *fronts[] = {"", "2 1\n", "1 2\nx "};
    for (uint32_t len = 0; len <= 6; ++len) {
        uint64_t count = 1;
        for (uint32_t i = 0; i < len; ++i) count *= 7;
        for (uint64_t code = 0; code < count; ++code) {
            Bytes tail(len);
            uint64_t c = code;
            for (uint32_t i = 0; i < len; ++i, c /= 7) tail[i] = alphabet[c % 7];
            for (const char *front : fronts) {
                Bytes d = bytes_of(front);
                d.insert(d.end(), tail.begin(), tail.end());
                if (d.empty()) { compare(d, 4, 1); continue; }
                compare(d, d.size(), 3);
                if (len <= 5 || code % 5 == 0)
                    for (size_t slab = 1; slab <= 3; ++slab) compare(d, slab, slab == 2 ? 1 : 3);
            }
        }
    }
}

// ---- (b) generated files ---------------------------------------------------------------------------------------------
struct Shape {
    uint32_t n, length;
    bool interleaved;
    uint32_t width;          // of a block (interleaved)
    bool vary_blocks, vary_records, blank_between, spaces_line, groups, crlf, final_break, pad_names, name_only, leading_blank;
    uint32_t name_len;
};

static Bytes generate(const Shape &s, Rng &rng)
{
    const std::string eol = s.crlf ? "\r\n" : "\n";
    std::vector<std::string> seqs(s.n), names(s.n);
    for (uint32_t r = 0; r < s.n; ++r) {
        for (uint32_t i = 0; i < s.length; ++i) seqs[r].push_back((char)(0x21 + rng.below(0x5e)));
        names[r] = "s" + std::to_string(r);
        while (names[r].size() < s.name_len) names[r].push_back((char)('A' + rng.below(26)));
    }
    auto grouped = [&](const std::string &x) {
        if (!s.groups) return x;
        std::string y;
        for (size_t i = 0; i < x.size(); ++i) {
            if (i && i % 4 == 0) y.push_back(' ');
            y.push_back(x[i]);
        }
        return y;
    };
    std::string out;
    if (s.leading_blank) out += eol + "   " + eol;
    out += " " + std::to_string(s.n) + " " + std::to_string(s.length) + eol;
    // the blocks: every record has a line in every block, and a line behind the name lines holds at least one base (it
    // must count); widths[r][b] of record r in block b
    std::vector<uint32_t> common;
    if (!s.interleaved) common.push_back(s.length);
    else
        for (uint32_t left = s.length; left;) {
            const uint32_t w = std::min(left, s.vary_blocks ? 1 + rng.below(2 * s.width) : s.width);
            common.push_back(w);
            left -= w;
        }
    const uint32_t blocks = (uint32_t)common.size();
    std::vector<std::vector<uint32_t>> widths(s.n, common);
    if (s.vary_records)
        for (uint32_t r = 0; r < s.n; ++r)
            for (uint32_t m = 0; m < 2 * blocks; ++m) {           // move a base from one block to another
                const uint32_t from = rng.below(blocks), to = rng.below(blocks);
                if (widths[r][from] > 1) { --widths[r][from]; ++widths[r][to]; }
            }
    if (s.name_only && blocks >= 2) { widths[0][1] += widths[0][0]; widths[0][0] = 0; }
    std::vector<uint32_t> done(s.n, 0);
    for (uint32_t block = 0; block < blocks; ++block) {
        if (block && s.blank_between) out += s.spaces_line ? "  " + eol : eol;
        for (uint32_t r = 0; r < s.n; ++r) {
            const uint32_t w = widths[r][block];
            if (block == 0) {
                out += names[r];
                if (w) out += s.pad_names ? std::string(names[r].size() < 10 ? 10 - names[r].size() : 1, ' ') : " ";
            }
            out += grouped(seqs[r].substr(done[r], w)) + eol;
            done[r] += w;
        }
    }
    if (!s.final_break) out.resize(out.size() - eol.size());
    return bytes_of(out);
}

static void generated_files()
{
    Rng rng(2024);
    const uint32_t tiles[] = {1, 2, 3, 7, 16, 64};
    long files = 0;
    for (uint32_t round = 0; round < 60; ++round) {
        Shape s;
        s.n = 1 + rng.below(round % 7 == 0 ? 9 : 4);
        s.length = round % 11 == 0 ? 1 : 1 + rng.below(70);
        s.interleaved = rng.below(3) != 0;
        s.width = 1 + rng.below(round % 5 == 0 ? 2 : 25);
        s.vary_blocks = rng.below(3) == 0;
        s.vary_records = rng.below(4) == 0;
        s.blank_between = rng.below(2) != 0;
        s.spaces_line = rng.below(2) != 0;
        s.groups = rng.below(3) == 0;
        s.crlf = rng.below(3) == 0;
        s.final_break = rng.below(3) != 0;
        s.pad_names = rng.below(2) != 0;
        s.name_only = rng.below(4) == 0;
        s.leading_blank = rng.below(4) == 0;
        s.name_len = round % 9 == 0 ? 40 + rng.below(30) : 1 + rng.below(12);
        const Bytes d = generate(s, rng);
        imc::FastaRecords want;
        CHECK(imc::read_phylip_bytes(d.data(), d.size(), "file", want).code == 0);   // (the generator writes what it means to)
        ++files;
        size_t header_end = 0;                                                      // the header line must end inside the first slab
        while (d[header_end] == '\n' || d[header_end] == '\r' || d[header_end] == ' ') ++header_end;
        while (header_end < d.size() && d[header_end] != '\n') ++header_end;
        for (uint32_t tile : tiles) {
            const size_t top = std::min<size_t>(d.size(), 3 * (size_t)tile + 2);
            for (size_t slab = 1; slab <= top; ++slab) {
                const bool took = compare(d, slab, tile);
                CHECK(took || slab <= header_end);
            }
            CHECK(compare(d, d.size(), tile));
        }
        // one byte replaced, inserted or removed: declines or agrees
        for (uint32_t m = 0; m < 40; ++m) {
            Bytes e = d;
            const uint8_t pool[] = {' ', '\n', '\r', '\t', 'A', '1', 0x80, 0x7f, 0x00};
            const size_t where = rng.below((uint32_t)e.size());
            const uint32_t how = rng.below(3);
            if (how == 0) e[where] = pool[rng.below(9)];
            else if (how == 1) e.insert(e.begin() + where, pool[rng.below(9)]);
            else e.erase(e.begin() + where);
            const uint32_t tile = tiles[rng.below(6)];
            compare(e, 1 + rng.below(3 * tile + 2), tile);
            compare(e, e.size() ? e.size() : 1, tile);
        }
    }
    std::printf("generated files: %ld\n", files);
}

// ---- (c) hand-written files ------------------------------------------------------------------------------------------
static void all_geometries(const std::string &text, bool takes, size_t min_slab = 1)
{
    const Bytes d = bytes_of(text);
    for (uint32_t tile : {1u, 3u, 16u})
        for (size_t slab = min_slab; slab <= d.size(); ++slab) CHECK(compare(d, slab, tile) == takes);
}

static void hand_written()
{
    // taken (the slab sizes start where the header line fits)
    all_geometries(" 2 8\n1         ACGTACGT\n2         ACGTACGA\n", true, 6);
    all_geometries("2 9\na ACG\nb ACGTA\nACGTAC\nACGT\n", true, 4);
    all_geometries("2 6\r\na ACG\r\nb ACG\r\n\r\nACG\r\nACG", true, 5);
    all_geometries("\n  \n2 4\na\nb\n  \nAC GT\n ACGT\n", true, 10);
    all_geometries("1 3\nonly   A C G   \n", true, 4);
    all_geometries("3 0\na\nb\nc\n", true, 4);
    all_geometries("2 2  \nab AC\ncd   GT  ", true, 6);
    // declined, every one also at one slab
    all_geometries("2 4\na\tACGT\nb\tACGT\n", false);                      // a tab separator
    all_geometries("2 4\n a ACGT\nb ACGT\n", false);                       // a space in front of a name
    all_geometries("2 4\ra ACGT\rb ACGT\r", false);                        // lone '\r'
    all_geometries("2 4 x\na ACGT\nb ACGT\n", false);                      // a third header word
    all_geometries("0 4\n", false);                                        // n == 0
    all_geometries("2 40\na ACGT\nb ACGT\n", false);                       // n * length larger than the file
    all_geometries("2 4\na ACGT\na ACGT\n", false);                        // a repeated name
    all_geometries("3 4\na ACGT\nb ACGT\n", false);                        // fewer than n name lines
    all_geometries("2 4\na ACGT\nb ACG\n", false);                         // a short record
    all_geometries("2 4\na ACGT\nb ACG\nA\nAA\n", false);                  // a long first record, a full second one
    all_geometries("2 4\na ACGTA\nb ACG\n", false);                        // equal total, unequal records
    all_geometries("2 4\na AC\xc3GT\nb ACGT\n", false);                    // a byte >= 0x80
    all_geometries("2 4\na AC\x01T\nb ACGT\n", false);                     // a control byte
    all_geometries("+2 4\na ACGT\nb ACGT\n", false);                       // a header word that is not digits
    all_geometries("", false);
    all_geometries("\n\n", false);
    // more records than the device parser takes; a header line that does not end inside the first slab
    {
        std::string big = "4097 1\n";
        for (int r = 0; r < 4097; ++r) big += "n" + std::to_string(r) + " A\n";
        CHECK(!compare(bytes_of(big), big.size(), 64));
        std::string ok = "4096 1\n";
        for (int r = 0; r < 4096; ++r) ok += "n" + std::to_string(r) + " A\n";
        CHECK(compare(bytes_of(ok), ok.size(), 64));
        CHECK(compare(bytes_of(ok), 100, 16));
        const Bytes far = bytes_of("      2 1\na A\nb C\n");
        CHECK(!compare(far, 8, 3) && compare(far, 10, 3));
    }
    // a name of name_max - 1 bytes is taken, one of name_max bytes or more is not; the line cap
    {
        const Bytes d = bytes_of("2 2\nabcdefg AC\nhi GT\n");
        CHECK(compare(d, 5, 3, 1u << 20, 8) && !compare(d, 5, 3, 1u << 20, 7) && !compare(d, d.size(), 3, 1u << 20, 4));
        const Bytes e = bytes_of("2 3\na A\nb C\nC\nG\nT\nA\n");                // seven counted lines
        CHECK(compare(e, 4, 3, 7) && !compare(e, 4, 3, 6) && !compare(e, e.size(), 3, 5) && !compare(e, 4, 1, 3));
    }
}

// The edges of the rules behind the last slab, beside those hand_written() stands on already: "3 0" with its three name
// lines (exactly n name lines and no base: taken), "b ACG" (a last record one base short on its name line), "abcdefg" at
// name_max 8 and 7 (a name of name_max - 1 bytes is taken, one of name_max bytes is not).
static void session_edges()
{
    all_geometries("3 0\na\nb\n", false);                                 // one name line fewer than n, no base
    all_geometries("2 4\na AC\nb AC\nGT\nG\n", false);                     // a last record one base short in the last block
    all_geometries("2 4\na AC\nb AC\nGT\nGT\n", true, 4);                  // ... and whole
    const Bytes d = bytes_of("2 2\nabcdefg AC\nhi GT\n");                   // the name limit with the whole file in one slab and one tile
    CHECK(compare(d, d.size(), 64, 1u << 20, 8) && !compare(d, d.size(), 64, 1u << 20, 7));
}

int main()
{
    all_short_strings();
    generated_files();
    hand_written();
    CHECK(g_taken > 1000 && g_declined > 1000);
    const long compared = g_compared, taken = g_taken, declined = g_declined;      // (the totals name the seeded inputs alone)
    session_edges();
    std::printf("session edges: compared %ld (taken %ld, declined %ld)\n", g_compared - compared, g_taken - taken, g_declined - declined);
    std::printf("compared %ld (taken %ld, declined %ld)\nphylip_tiles ok\n", compared, taken, declined);
    return 0;
}
