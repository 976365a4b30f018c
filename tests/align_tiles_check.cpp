// align_tiles_check.cpp - the parallel form of reading a FASTA alignment (csrc/align_tiles.hpp) against the host reader
// imc::read_fasta (csrc/fasta_io.hpp), on the CPU.  The functions the alignment kernels call are driven here
// sequentially, the way the device path runs them: the file goes through the product's own loop (imc::slab_stream of
// csrc/slab_stream.hpp: aln_slab_cut, what lies behind the cut is carried into the next slab), and per slab the three
// launches - a summary per tile, folded from single positions with aln_combine (and equal to aln_range over the tile),
// one scan that gives every tile its entry state and its offsets from the state the slab is entered in, then every tile
// (in reverse order here: they are independent) walks its bytes from its own entry alone, writes the kept bytes at its
// own offset and reports its headers; the names come from the slab's bytes (aln_header_name).  The first slab that
// declines ends the file.
//   (a) every string up to length 7 over {'>', 'A', 'c', ' ', '\n', '\r', '\t', 0x80}: one slab at tile sizes 1, 2, 3, 4, 7
//       and 64, and every two-slab split the slab rule allows (first slab of 1 .. n - 1 bytes) at tile size 3
//   (b) a few hundred random longer files that conform to what the device parser takes (wrapped and unwrapped lines, "\n"
//       and "\r\n", empty lines, lines in front of the first header, descriptions, empty records, no final line break),
//       and the same with one byte replaced: all tile sizes, every two-slab split
//   The tile scan either declines or yields exactly read_fasta's records (names, lengths, bases); a string that satisfies
//   the separately written predicate conforms() must NOT decline, except where a header line is longer than the slab.
//   (c) pairwise_symbol against encode_pairwise for all 256 x 256 byte pairs; triplet_symbol against a restatement of the
//       reference's rule on all triples over "ACGTacgtNn-" and on every byte in each position; aln_gather / aln_symbols
//       against both encoders at every start residue and lengths around 16, from a buffer that ends where a device buffer
//       ends.
//   (d) the split of a one-workgroup scan among its threads (imc::scan_share) and the fold / scan / walk over it.
// Built with -fsanitize=address,undefined.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../imcoalhmm_amd/csrc/align_tiles.hpp"
#include "../imcoalhmm_amd/csrc/obs_io.hpp"
#include "../imcoalhmm_amd/csrc/slab_stream.hpp"

static long g_compared = 0, g_declined = 0, g_conforming = 0;

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

struct Parsed {
    bool declined = false, slab_declined = false;    // slab_declined: a header line longer than the slab
    std::vector<std::string> names;
    std::vector<uint64_t> start, length;
    Bytes bases;
};

// ---- what the device parser takes, written on its own ------------------------------------------------------
static bool conforms(const Bytes &d)
{
    std::set<std::string> names;
    size_t pos = 0;
    while (pos < d.size()) {
        size_t end = pos;
        while (end < d.size() && d[end] != '\n') ++end;
        size_t stop = end;
        if (stop > pos && d[stop - 1] == '\r') --stop;                       // "\r\n", or "\r" in front of the end of the file
        if (stop > pos && d[pos] == '>') {
            bool in_word = false, have = false;
            std::string name;
            for (size_t i = pos + 1; i < stop; ++i) {
                const uint8_t c = d[i];
                if (!(c == '\t' || (c >= 0x20 && c <= 0x7e))) return false;
                const bool blank = c == '\t' || c == ' ';
                if (!blank && !have) { in_word = true; name.push_back((char)c); }
                if (blank && in_word) { in_word = false; have = true; }
            }
            if (name.empty() || !names.insert(name).second) return false;
        } else
            for (size_t i = pos; i < stop; ++i)
                if (d[i] < 0x21 || d[i] > 0x7e) return false;
        pos = end + 1;
    }
    return names.size() <= imc::kMaxAlnRecords;
}

// ---- the device path, sequentially -------------------------------------------------------------------------
static std::vector<imc::AlnSummary> t_sums, g_position;     // g_position[i]: the summary of byte i of the file (check_file)
static std::vector<uint32_t> t_state, t_seq, t_hdr;
static bool g_scatter_declined = false;                     // run the scatter of a slab that declines as well (the device does)

// first_slab: bytes the first read delivers (0: the whole file in one slab); the second read delivers the rest.  The loop
// is the product's (imc::slab_stream) over two buffers of the file's size, with the three launches as its "queue"; the cut,
// the "judge" and what follows the last slab are the product's too (imc::AlnSession: cut, accept, finish).
static void tiled_parse(const Bytes &data, size_t first_slab, size_t tile, Parsed &out)
{
    out.declined = out.slab_declined = false;
    out.names.clear();
    out.start.clear();
    out.length.clear();
    out.bases.assign(data.size(), 0xee);
    imc::AlnSession ses;                                     // the product's rules, with the arguments the engine passes
    const uint32_t &state = ses.state, &prev = ses.prev;
    const uint64_t &kept = ses.kept, room = (data.size() + 15) & ~(uint64_t)15;
    static Bytes slabs[2];                                   // scratch, kept between calls
    static std::vector<imc::AlnRecord> table;
    const size_t slab = std::max<size_t>(data.size(), 1);
    for (Bytes &b : slabs) b.assign(slab, 0);
    uint8_t *const host[2] = {slabs[0].data(), slabs[1].data()};
    size_t pos = 0, base = 0;                                // base: where the slab's first byte stands in the file
    bool between_slabs = true;                               // false while a slab is judged: a decline is then the verdict's, else the cut's
    imc::AlnTotal total{state, 0, 0, 0};
    const int end = imc::slab_stream(
        host, slab,
        [&](uint8_t *dst, size_t want, bool &eof) {
            const size_t take = std::min(pos == 0 && first_slab ? first_slab : want, data.size() - pos);
            if (take) std::memcpy(dst, data.data() + pos, take);
            pos += take;
            if (pos == data.size()) eof = true;
            return take;
        },
        [&](const uint8_t *buf, size_t fill, bool last) { return ses.cut(buf, fill, last); },
        [&](int cur, size_t cut) -> int {
            const uint8_t *buf = host[cur];
            const uint32_t n = (uint32_t)cut, tiles = (uint32_t)((cut + tile - 1) / tile);
            CHECK(prev == (base ? data[base - 1] : '\n'));        // a byte's summary is the same in every tiling
            // launch 1: tile summaries, from single positions
            if (t_sums.size() < tiles) { t_sums.resize(tiles); t_state.resize(tiles); t_seq.resize(tiles); t_hdr.resize(tiles); }
            for (uint32_t t = 0; t < tiles; ++t) {
                const uint32_t lo = t * (uint32_t)tile, hi = std::min<uint32_t>(lo + (uint32_t)tile, n);
                imc::AlnSummary s = imc::aln_identity();
                for (uint32_t i = lo; i < hi; ++i) s = imc::aln_combine(s, g_position[base + i]);
                if (first_slab == 0 || g_scatter_declined) {             // what a thread computes for its bytes at once
                    const imc::AlnSummary whole = imc::aln_range(buf + lo, lo ? buf[lo - 1] : prev, hi - lo);
                    CHECK(std::memcmp(&s, &whole, sizeof s) == 0);
                }
                t_sums[t] = s;
            }
            // launch 2: the scan - maps first, then the counts in the resolved states
            uint32_t map = imc::kAlnIdentityMap;
            total = imc::AlnTotal{state, 0, 0, 0};
            imc::AlnSummary all = imc::aln_identity();
            for (uint32_t t = 0; t < tiles; ++t) {
                const uint32_t in = imc::aln_exit(map, state);
                CHECK(in == total.exit);
                t_state[t] = in; t_seq[t] = total.seq; t_hdr[t] = total.hdr;
                total.seq += t_sums[t].seq[in];
                total.hdr += t_sums[t].hdr[in];
                total.decline |= imc::aln_declines(t_sums[t].map, in);
                total.exit = imc::aln_exit(t_sums[t].map, in);
                map = imc::aln_compose(map, t_sums[t].map);
                all = imc::aln_combine(all, t_sums[t]);
            }
            const imc::AlnTotal folded = imc::aln_resolve(all, state);
            CHECK(folded.exit == total.exit && folded.seq == total.seq && folded.hdr == total.hdr && folded.decline == total.decline);
            // launch 3: the scatter, tiles in reverse order
            table.assign(total.hdr, imc::AlnRecord{0u, 0u, 0u});
            for (uint32_t t = total.decline && !g_scatter_declined ? 0 : tiles; t-- > 0;) {
                const uint32_t lo = t * (uint32_t)tile, hi = std::min<uint32_t>(lo + (uint32_t)tile, n);
                uint32_t st = t_state[t], at_seq = t_seq[t], at_hdr = t_hdr[t], pre = imc::kAlnIdentityMap;
                for (uint32_t i = lo; i < hi; ++i) {
                    CHECK(st == imc::aln_exit(pre, t_state[t]));                      // the threads' map scan gives the same state
                    const uint8_t before = i ? buf[i - 1] : prev;
                    const imc::AlnStep step = imc::aln_step(st, before, buf[i]);
                    if (step.cls == imc::kAlnKept) {
                        CHECK(kept + at_seq < out.bases.size());
                        out.bases[kept + at_seq++] = buf[i];
                    } else if (step.cls == imc::kAlnHeaderStart) {
                        CHECK(at_hdr < table.size());
                        table[at_hdr++] = imc::AlnRecord{i, 0u, kept + at_seq};
                    }
                    st = step.next;
                    pre = imc::aln_compose(pre, g_position[base + i].map);
                }
                CHECK(at_seq == t_seq[t] + t_sums[t].seq[t_state[t]] && at_hdr == t_hdr[t] + t_sums[t].hdr[t_state[t]]);
            }
            return 0;
        },
        [&](int cur, size_t cut) -> int {
            between_slabs = false;
            const imc::IoResult r = ses.accept(
                total, [&](uint32_t, uint32_t count, const imc::AlnRecord *&recs) { CHECK(count == table.size()); recs = table.data(); return imc::IoResult(); }, host[cur],
                cut, room);
            CHECK(r.code == 0 || r.code == imc::kSlabDeclined);   // the device path has no error of its own to report
            if (r.code) return r.code;
            base += cut;
            between_slabs = true;
            return 0;
        });
    if (end == imc::kSlabDeclined) { out.declined = true; out.slab_declined = between_slabs; return; }
    if (ses.finish(out.length).code) { out.declined = true; return; }
    out.names = ses.names;
    out.start = ses.start;
    out.bases.resize(kept);
}

static void compare(const Bytes &data, size_t first_slab, size_t tile, const imc::IoResult &host_rc, const imc::FastaRecords &host, bool takes)
{
    static Parsed got;
    tiled_parse(data, first_slab, tile, got);
    ++g_compared;
    if (got.declined) {
        ++g_declined;
        CHECK(!takes || got.slab_declined);                   // declining is a way out, not the rule
        return;
    }
    CHECK(host_rc.code == 0);                                 // every error is the host reader's: the tile scan declines
    CHECK(got.names == host.names);
    CHECK(got.length.size() == host.names.size());
    for (size_t k = 0; k < host.names.size(); ++k) {
        CHECK(got.length[k] == host.seqs[k].size() && got.start[k] + got.length[k] <= got.bases.size());
        CHECK(std::memcmp(got.bases.data() + got.start[k], host.seqs[k].data(), host.seqs[k].size()) == 0);
    }
    CHECK(host.names.empty() ? got.bases.empty() : got.start[0] == 0);
}

static const size_t kTiles[] = {1, 2, 3, 4, 7, 64};

static void check_file(const Bytes &data, bool all_tiles_on_splits, bool must_conform)
{
    static imc::FastaRecords host;
    const imc::IoResult rc = imc::read_fasta_bytes(data.data(), data.size(), "f", host);
    const bool takes = conforms(data);
    CHECK(!must_conform || takes);
    CHECK(!takes || rc.code == 0);
    if (takes) ++g_conforming;
    g_position.resize(data.size());
    for (size_t i = 0; i < data.size(); ++i) g_position[i] = imc::aln_range(data.data() + i, i ? data[i - 1] : (uint8_t)'\n', 1);
    for (size_t tile : kTiles) compare(data, 0, tile, rc, host, takes);
    for (size_t first = 1; first < data.size(); ++first) {
        if (all_tiles_on_splits)
            for (size_t tile : kTiles) compare(data, first, tile, rc, host, takes);
        else
            compare(data, first, 3, rc, host, takes);
    }
}

// ---- (b) random files ---------------------------------------------------------------------------------------
static Bytes random_conforming(Rng &rng)
{
    static const char bases[] = "ACGTacgtNn-*>.";
    Bytes d;
    const std::string eol = rng.below(2) ? "\r\n" : "\n";
    auto put = [&](const std::string &s) { d.insert(d.end(), s.begin(), s.end()); };
    for (uint32_t k = rng.below(3); k > 0; --k) put((rng.below(2) ? std::string("#junk") : std::string("")) + eol);   // in front of the first header
    const uint32_t records = rng.below(5);
    for (uint32_t r = 0; r < records; ++r) {
        put(">s" + std::to_string(r));
        if (rng.below(3) == 0) put(std::string(rng.below(2) ? " " : "\t") + "some description");
        put(eol);
        const uint32_t length = rng.below(4) == 0 ? 0 : rng.below(90), wrap = rng.below(3) == 0 ? 1000 : 1 + rng.below(20);
        for (uint32_t i = 0; i < length; ++i) {
            uint8_t c = (uint8_t)bases[rng.below(sizeof bases - 1)];
            if (i % wrap == 0 && c == '>') c = 'A';                              // '>' at column 0 is a header
            d.push_back(c);
            if ((i + 1) % wrap == 0 && i + 1 < length) put(eol);
        }
        if (length) put(eol);
        if (rng.below(4) == 0) put(eol);                                          // an empty line between records
    }
    if (!d.empty() && rng.below(3) == 0) d.resize(d.size() - eol.size());        // no final line break
    return d;
}

// ---- the record cap by hand -----------------------------------------------------------------------------------
// Exactly kMaxAlnRecords records are taken and one more is declined, in one slab and with the last header alone in a
// second slab (the first slab then holds kMaxAlnRecords headers, and the cap is met by the names of an earlier slab).
static void check_record_cap()
{
    for (uint32_t records : {imc::kMaxAlnRecords, imc::kMaxAlnRecords + 1}) {
        Bytes d;
        size_t last_header = 0;
        for (uint32_t r = 0; r < records; ++r) {
            const std::string rec = ">r" + std::to_string(r) + "\nAC\n";
            last_header = d.size();
            d.insert(d.end(), rec.begin(), rec.end());
        }
        static imc::FastaRecords host;
        const imc::IoResult rc = imc::read_fasta_bytes(d.data(), d.size(), "f", host);
        const bool takes = conforms(d);
        CHECK(rc.code == 0 && host.names.size() == records && takes == (records <= imc::kMaxAlnRecords));
        g_position.resize(d.size());
        for (size_t i = 0; i < d.size(); ++i) g_position[i] = imc::aln_range(d.data() + i, i ? d[i - 1] : (uint8_t)'\n', 1);
        for (size_t first : {(size_t)0, last_header, d.size() / 2}) {
            const long declined = g_declined;
            compare(d, first, 64, rc, host, takes);
            CHECK((g_declined > declined) == !takes);
        }
    }
}

// ---- (c) column rules ----------------------------------------------------------------------------------------
static uint32_t reference_triplet(uint8_t a, uint8_t b, uint8_t c)
{
    const std::string clean = "ACGT", s{(char)std::toupper(a), (char)std::toupper(b), (char)std::toupper(c)};
    if (a >= 0x80 || b >= 0x80 || c >= 0x80 || clean.find(s[0]) == clean.npos || clean.find(s[1]) == clean.npos || clean.find(s[2]) == clean.npos) return 64;
    return (uint32_t)(clean.find(s[0]) + 4 * clean.find(s[1]) + 16 * clean.find(s[2]));
}

static void check_column_rules()
{
    uint8_t a[256], b[256], want[256];
    for (int x = 0; x < 256; ++x) {
        for (int y = 0; y < 256; ++y) { a[y] = (uint8_t)x; b[y] = (uint8_t)y; }
        imc::encode_pairwise(reinterpret_cast<const char *>(a), reinterpret_cast<const char *>(b), 256, want);
        for (int y = 0; y < 256; ++y) CHECK(imc::pairwise_symbol((uint8_t)x, (uint8_t)y) == want[y]);
    }
    const std::string common = "ACGTacgtNn-";
    for (char x : common)
        for (char y : common)
            for (char z : common) {
                const uint32_t s = imc::triplet_symbol((uint8_t)x, (uint8_t)y, (uint8_t)z);
                CHECK(s == reference_triplet((uint8_t)x, (uint8_t)y, (uint8_t)z) && s <= 64);
                uint8_t one;
                imc::encode_triplet(&x, &y, &z, 1, &one);
                CHECK(one == s);
            }
    for (int v = 0; v < 256; ++v)
        for (char o : std::string("AcT-")) {
            const uint8_t u = (uint8_t)v, w = (uint8_t)o;
            CHECK(imc::triplet_symbol(u, w, 'g') == reference_triplet(u, w, 'g'));
            CHECK(imc::triplet_symbol(w, u, 'C') == reference_triplet(w, u, 'C'));
            CHECK(imc::triplet_symbol('t', w, u) == reference_triplet('t', w, u));
        }
    // the column kernel's thread: sequences back to back at every residue, the buffer ends as a device buffer does
    Rng rng(99);
    for (uint32_t L : {1u, 3u, 15u, 16u, 17u, 31u, 32u, 33u, 70u})
        for (uint32_t lead = 0; lead < 4; ++lead) {
            const uint64_t start[3] = {lead, lead + L, lead + 2 * (uint64_t)L};
            Bytes bases((lead + 3 * L + 15) / 16 * 16, 0xee);
            for (uint64_t i = lead; i < lead + 3 * (uint64_t)L; ++i) bases[i] = rng.below(8) ? (uint8_t)"ACGTacgtNn-"[rng.below(11)] : (uint8_t)rng.below(256);
            Bytes want2(L), want3(L), got2((L + 15) / 16 * 16, 0xee), got3(got2);
            const char *p = reinterpret_cast<const char *>(bases.data());
            for (int order = 0; order < 2; ++order) {
                const uint64_t o0 = start[order ? 2 : 0], o1 = start[1], o2 = start[order ? 0 : 2];
                imc::encode_pairwise(p + o0, p + o1, L, want2.data());
                imc::encode_triplet(p + o0, p + o1, p + o2, L, want3.data());
                for (uint32_t col0 = 0; col0 < L; col0 += imc::kAlnColumns) {
                    uint32_t x[4], y[4], z[4];
                    imc::aln_gather(bases.data(), o0, col0, L, x);
                    imc::aln_gather(bases.data(), o1, col0, L, y);
                    imc::aln_gather(bases.data(), o2, col0, L, z);
                    for (uint32_t j = 0; j < 4; ++j) {
                        const uint32_t valid = L - col0 > 4 * j ? L - col0 - 4 * j : 0u;
                        const uint32_t w2 = imc::aln_symbols<2>(x[j], y[j], 0u, valid), w3 = imc::aln_symbols<3>(x[j], y[j], z[j], valid);
                        std::memcpy(got2.data() + col0 + 4 * j, &w2, 4);
                        std::memcpy(got3.data() + col0 + 4 * j, &w3, 4);
                    }
                }
                CHECK(std::memcmp(got2.data(), want2.data(), L) == 0 && std::memcmp(got3.data(), want3.data(), L) == 0);
                for (size_t i = L; i < got2.size(); ++i) CHECK(got2[i] == 0 && got3[i] == 0);      // the padding stays zero
            }
        }
}

// ---- (d) the shares of the one-workgroup scan ---------------------------------------------------------------
// imc::scan_share with 1024 threads: consecutive shares in thread order that cover [0, n) once; and the scan the kernels
// run over them (tile_scan.hpp: every thread folds its share, the folds are scanned Hillis-Steele, every thread walks its
// share from its prefix) under map composition, which is not commutative, against the plain left-to-right prefix.
static void check_scan_shares()
{
    const uint32_t threads = 1024;
    Rng rng(5);
    std::vector<uint32_t> sizes = {0, 1, 1023, 1024, 1025, 2049};
    for (uint32_t k = 1; k <= 3; ++k) { sizes.push_back(2050 * k - 1); sizes.push_back(2050 * k + 1); }
    for (uint32_t n : sizes) {
        uint32_t next = 0;
        for (uint32_t t = 0; t < threads; ++t) {
            const imc::ScanShare own = imc::scan_share(n, threads, t);
            CHECK(own.lo == next && own.hi >= own.lo && own.hi <= n);
            CHECK(own.hi - own.lo <= (n + threads - 1) / threads);
            CHECK(own.hi > own.lo || own.lo == n);               // no empty share in front of a non-empty one
            next = own.hi;
        }
        CHECK(next == n);
        std::vector<uint32_t> maps(n), want(n), got(n, 0xffffffffu), fold(threads), step(threads);
        for (uint32_t &m : maps) {                               // random maps: an exit state and a decline bit per entry state
            m = 0;
            for (uint32_t e = 0; e < imc::kAlnStates; ++e) m |= rng.below(imc::kAlnStates) << (3u * e) | rng.below(2) << (16u + e);
        }
        uint32_t run = imc::kAlnIdentityMap;
        for (uint32_t i = 0; i < n; ++i) { want[i] = run; run = imc::aln_compose(run, maps[i]); }
        for (uint32_t t = 0; t < threads; ++t) {
            const imc::ScanShare own = imc::scan_share(n, threads, t);
            fold[t] = imc::kAlnIdentityMap;
            for (uint32_t i = own.lo; i < own.hi; ++i) fold[t] = imc::aln_compose(fold[t], maps[i]);
        }
        for (uint32_t d = 1; d < threads; d <<= 1) {
            for (uint32_t t = 0; t < threads; ++t) step[t] = t >= d ? imc::aln_compose(fold[t - d], fold[t]) : fold[t];
            fold.swap(step);
        }
        for (uint32_t t = 0; t < threads; ++t) {
            const imc::ScanShare own = imc::scan_share(n, threads, t);
            uint32_t before = t ? fold[t - 1] : imc::kAlnIdentityMap;
            for (uint32_t i = own.lo; i < own.hi; ++i) { got[i] = before; before = imc::aln_compose(before, maps[i]); }
        }
        CHECK(got == want && fold[threads - 1] == run);
    }
}

int main()
{
    // (a) every short string
    static const uint8_t alphabet[8] = {'>', 'A', 'c', ' ', '\n', '\r', '\t', 0x80};
    for (size_t len = 0; len <= 7; ++len) {
        size_t combos = 1;
        for (size_t i = 0; i < len; ++i) combos *= 8;
        Bytes s(len);
        for (size_t code = 0; code < combos; ++code) {
            size_t c = code;
            for (size_t i = 0; i < len; ++i) { s[i] = alphabet[c % 8]; c /= 8; }
            check_file(s, false, false);
        }
    }
    const long short_conforming = g_conforming;
    CHECK(short_conforming > 1000);
    // (b) random longer files: conforming as they are, then with one byte replaced
    Rng rng(7);
    long random_files = 0;
    g_scatter_declined = true;
    for (int k = 0; k < 300; ++k) {
        Bytes d = random_conforming(rng);
        check_file(d, true, true);
        ++random_files;
        if (d.empty()) continue;
        static const uint8_t spoil[] = {' ', '\t', '\r', '\n', '>', 0x80, 0x0b, 0x7f, 0x1c, 'A'};
        d[rng.below((uint32_t)d.size())] = spoil[rng.below(sizeof spoil)];
        check_file(d, false, false);
    }
    CHECK(g_conforming - short_conforming >= random_files);
    // the slab rule by hand
    const uint8_t two[] = ">a\nACGT\n>bb\nAC";
    CHECK(imc::aln_slab_cut(two, 10, false, imc::kAlnStart0) == 8);      // cut in front of ">b"
    CHECK(imc::aln_slab_cut(two, 6, false, imc::kAlnStart0) == 6);       // a sequence line may be cut anywhere
    CHECK(imc::aln_slab_cut(two, 2, false, imc::kAlnStart0) == 0);       // a header line longer than the buffer
    CHECK(imc::aln_slab_cut(two, 2, false, imc::kAlnSeq) == 2);          // ... is a '>' inside a sequence line when entered in one
    CHECK(imc::aln_slab_cut(two, 10, true, imc::kAlnStart0) == 10);
    check_column_rules();
    check_scan_shares();
    const long compared = g_compared, declined = g_declined;     // (the totals name the seeded inputs alone)
    check_record_cap();
    std::printf("record cap: %ld parses compared, %ld declined\n", g_compared - compared, g_declined - declined);
    std::printf("align_tiles ok: %ld parses compared, %ld declined, %ld conforming files\n", compared, declined, g_conforming);
    return 0;
}
