// train_tiles.hpp - the parallel form of dictionary training (pair_dict.hpp: train_dict, train_dict_wide,
// train_dictionary), host/device.
//
// The host trainer is the specification: its dictionary, entry for entry.  What it does per merge or round splits into a
// COUNT (order-free: integer adds), a CHOICE (a total order on (count, key)) and a REPLACEMENT pass (the encoder's pass,
// encode_tiles.hpp, already exact).  So the device needs no new proof obligation beyond "the counts are the host's
// counts and the choice is the host's choice":
//   byte phase   counts of a * A + b over adjacent pairs, summed per tile in any order; the winner is the maximum of
//                (count, -key) over the eligible bins - the host's row-major scan with `>` keeps the FIRST maximum, which
//                is the smallest key among equal counts, so the maximum is an associative and commutative combine
//   rounds       counts per distinct key a << 16 | b in an open-addressing table, inserted in any order; the keys at or
//                above the threshold are listed in any order and ranked on the host by pair_dict.hpp's own comparator
// The kernels (kernels_train.hpp) and the CPU check (tests/train_tiles_check.cpp) call the functions below; the sequence
// of decisions around them (which sample, which thresholds, when to stop) is train_with(), which runs on any backend
// that can load, count and replace: the device (imcoal_fwd.hip) and the CPU check's tile emulation.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "encode_tiles.hpp"
#include "pair_dict.hpp"

namespace imc {

// ---- byte phase: bins and the winner -----------------------------------------------------------------
constexpr uint32_t kTrnLdsBins = 16384;        // A * A bins of 4 bytes are kept in LDS up to here (64 KB: A <= 128)

IMC_ENC_HD inline uint32_t pair_bin(uint32_t a, uint32_t b, uint32_t A) { return a * A + b; }
IMC_ENC_HD inline bool pair_bins_in_lds(uint32_t A) { return A * A <= kTrnLdsBins; }

struct PairBest {
    uint32_t count;    // 0: no eligible pair
    uint32_t key;      // its bin a * A + b
};
constexpr uint32_t kNoBin = 0xffffffffu;

IMC_ENC_HD inline PairBest best_identity() { return PairBest{0u, kNoBin}; }

// a pair can win only with a count and, under a cap, while both halves are shallower than the cap
IMC_ENC_HD inline bool pair_eligible(uint32_t count, int depth_a, int depth_b, int max_depth)
{
    return count > 0 && (max_depth <= 0 || (depth_a > depth_b ? depth_a : depth_b) < max_depth);
}

// larger count first, then smaller key: (count, -key) compared lexicographically.  Associative and commutative.
IMC_ENC_HD inline PairBest best_combine(const PairBest &x, const PairBest &y)
{
    const bool first = x.count != y.count ? x.count > y.count : x.key <= y.key;   // (selects on the fields: they stay in registers)
    return PairBest{first ? x.count : y.count, first ? x.key : y.key};
}

// ---- rounds: the counting table ----------------------------------------------------------------------
// Open addressing with linear probing over `capacity` slots (a power of two, at least twice the stream length, so it
// never fills); kNoKey (encode_tiles.hpp) marks an empty slot.
inline uint32_t count_table_capacity(size_t n)
{
    uint32_t cap = 16;
    while ((size_t)cap < 2 * n) cap <<= 1;
    return cap;
}
IMC_ENC_HD inline uint32_t count_slot(uint32_t key, uint32_t capacity) { return ((key * 2654435761u) >> 5) & (capacity - 1); }

// host form of one insertion (the kernel claims the slot with a compare-and-swap and adds with an atomic instead);
// false: no free slot within `capacity` probes
inline bool count_table_add(std::vector<uint32_t> &keys, std::vector<uint32_t> &counts, uint32_t key, uint32_t c)
{
    const uint32_t cap = (uint32_t)keys.size();
    uint32_t s = count_slot(key, cap);
    for (uint32_t probe = 0; probe < cap; ++probe) {
        if (keys[s] == kNoKey) keys[s] = key;
        if (keys[s] == key) { counts[s] += c; return true; }
        s = (s + 1) & (cap - 1);
    }
    return false;
}

// ---- the sample ----------------------------------------------------------------------------------------
// A training sample is the concatenation of pieces (one chunk's symbols, or the heads of many: recompress_share); the
// part [first, first + count) of it is these ranges of the pieces, in order.
struct SampleRange {
    size_t piece, src_first, count, dst_first;
};

inline std::vector<SampleRange> sample_ranges(const std::vector<size_t> &piece_len, size_t first, size_t count)
{
    std::vector<SampleRange> r;
    size_t at = 0;
    for (size_t k = 0; k < piece_len.size() && count; ++k) {
        const size_t end = at + piece_len[k];
        if (first < end) {
            const size_t lo = std::max(first, at), c = std::min(end - lo, count - (lo - first));
            if (c) r.push_back({k, lo - at, c, lo - first});
        }
        at = end;
        if (at >= first + count) break;
    }
    return r;
}

// ---- the sequence of decisions -------------------------------------------------------------------------
// What a backend does (every call returns 0 or an error code that train_with hands on):
//   load(first, count)                  the stream becomes symbols [first, first + count) of the sample
//   byte_step(A, max_depth, &s)         counts the stream's adjacent pairs over alphabet A, finds the winner (s.count == 0:
//                                       none), names it token A and runs its replacement pass into the spare stream
//   accept()                            the spare stream becomes the stream (length s.new_n)
//   count_round(threshold, &cand)       (count, key) of every distinct adjacent key that occurs >= threshold times, any order
//   apply(d, z0, nz, &new_n)            one replacement pass for tokens z0 .. z0 + nz - 1 of d; the stream is its output
//   truncate(n)                         the stream keeps its first n elements
struct ByteStep {
    uint32_t a, b, count, new_n;
};

template <class Backend>
int train_rounds_with(Backend &be, PairDict &d, size_t n, size_t min_count, int max_depth, TrainStats &st)
{
    if (d.alphabet < wide_base(d.nsym)) return 0;
    std::vector<int> depth = dict_depths(d);
    std::vector<RoundCandidate> found, cand;
    while (d.alphabet < kMaxAlphabet && n >= 2) {
        found.clear();
        if (int rc = be.count_round(min_count, found)) return rc;
        cand.clear();
        for (const RoundCandidate &c : found)
            if (c.first >= min_count && (max_depth <= 0 || std::max(depth[c.second >> 16], depth[c.second & 0xffffu]) < max_depth)) cand.push_back(c);
        if (cand.empty()) break;
        std::sort(cand.begin(), cand.end(), round_candidate_before);
        const size_t round = (size_t)round_size(d.alphabet), take = round_take(cand.size(), d.alphabet);
        const int z0 = d.alphabet;
        ++st.rounds;
        for (size_t q = 0; q < take; ++q) {
            const int a = (int)(cand[q].second >> 16), b = (int)(cand[q].second & 0xffffu);
            d.add(a, b);
            depth.push_back(1 + std::max(depth[a], depth[b]));
        }
        size_t new_n = 0;
        if (int rc = be.apply(d, z0, (int)take, &new_n)) return rc;
        n = new_n;
        if (take < round) break;
    }
    return 0;
}

// train_dictionary() on a backend: the same dictionary from the same sample of L symbols.  The byte phase is ONE greedy
// run: where the host starts again with the next lower threshold it continues - a threshold only decides where the run
// stops, never what it picks, so the restarted run would repeat every merge made so far.
template <class Backend>
int train_with(Backend &be, size_t L, int nsym, size_t forced_min_count, int max_depth, const TrainLimits &lim, TrainedDict &t, TrainStats &st)
{
    const bool wide_raw = nsym > kByteAlphabet;
    st = TrainStats{training_head(L, wide_raw, lim), 0, 0};
    init_dict(t.dict, nsym);
    if (wide_raw) {
        const size_t nt = std::min(L - 1, lim.wide_train_tokens * 8);
        if (int rc = be.load(1, nt)) return rc;
        if (int rc = train_rounds_with(be, t.dict, nt, lim.wide_min_count, max_depth, st)) return rc;
    } else {
        const size_t n0 = std::min(L - 1, lim.train_max);
        size_t n = n0;
        if (int rc = be.load(1, n0)) return rc;
        std::vector<int> depth((size_t)nsym, 0);
        for (int attempt = 0;; ++attempt) {
            st.attempts = (uint64_t)attempt + 1;
            while (t.dict.alphabet < kByteAlphabet && n >= 2) {
                ByteStep s{};
                if (int rc = be.byte_step(t.dict.alphabet, max_depth, &s)) return rc;
                if (s.count == 0 || s.count < kByteThresholds[attempt]) break;
                t.dict.add((int)s.a, (int)s.b);
                depth.push_back(1 + std::max(depth[s.a], depth[s.b]));
                be.accept();
                n = s.new_n;
            }
            if (attempt == 2 || !byte_phase_retry(t.dict.alphabet, n0, lim)) break;
        }
        if (t.dict.alphabet >= kByteAlphabet) {
            const size_t cols = std::min(L, lim.wide_train_tokens * 96);
            if (cols - 1 != n0) {                    // the rounds look further than the byte phase did: encode that head
                n = cols - 1;
                if (int rc = be.load(1, n)) return rc;
                for (int z = nsym; z < kByteAlphabet && n >= 2; ++z)
                    if (int rc = be.apply(t.dict, z, 1, &n)) return rc;
            }
            const size_t nt = std::min(n, lim.wide_train_tokens);
            be.truncate(nt);
            if (int rc = train_rounds_with(be, t.dict, nt, wide_min_count(nt, forced_min_count, lim), max_depth, st)) return rc;
        }
    }
    t.depth = dict_depths(t.dict);
    t.order = dict_order(t.dict, t.depth);
    return 0;
}

}  // namespace imc
