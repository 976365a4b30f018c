// encode_tiles.hpp - the parallel form of one pass of the pair-dictionary encoder (pair_dict.hpp), host-only.
//
// A pass of replace_pair / replace_round walks the stream left to right and replaces every pair of this pass it meets,
// skipping the pair's second element.  With m[t] = 1 where (seq[t], seq[t+1]) is a pair of the pass (0 at the last
// position), the walk is the one-bit recurrence
//     taken[t] = m[t] && !taken[t-1]            (taken[-1] = 0)
// i.e. position t is taken iff m[t] and t - s is even, s being the start of the maximal run of ones that contains t.
// A taken position emits the pair's token, the position after a taken one emits nothing, every other position emits
// itself.  The only thing that crosses a tile boundary is that one bit (the parity of the run of ones ending just
// before the tile) - and it has to: (0,0) is the first merge of every alignment dictionary and runs of symbol 0 are
// thousands of columns long, far beyond any tile.
//
// A tile is therefore summarised as a function of the incoming bit: how many elements it emits and which bit it hands
// on, for both values of the bit (TileSummary).  Summaries compose associatively (tile_combine), so the carries and the
// output offsets of all tiles come from one scan, and every tile then writes its part of the output independently.
// The kernels (kernels_encode.hpp) and the CPU check (tests/encode_tiles_check.cpp) call the functions below.
// The pass schedule (encode_schedule) and the rule for how a chunk stores each level (level_rules) are at the end;
// tests/chunk_policy_check.cpp checks the rule against encode_levels().
//
// The stream the passes run on is 16-bit throughout.  Bit 15 (kChunkMark) marks the first element of a chunk; token
// ids stay below kMaxAlphabet = 2^14, so a marked element compares unequal to every pair half.  That is the rule
// "position 0 of a chunk is never merged" (pair_dict.hpp), and it lets K concatenated chunks go through one run of
// passes: no pair forms across a chunk boundary, because its second element would be the marked one.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

#include "pair_dict.hpp"

#if defined(__HIPCC__)
#define IMC_ENC_HD __host__ __device__
#else
#define IMC_ENC_HD
#endif

namespace imc {

constexpr tok_t kChunkMark = 0x8000;   // bit 15 of a stream element: first element of a chunk
static_assert(kMaxAlphabet <= kChunkMark, "token ids must leave bit 15 free");

// ---- tile summary -----------------------------------------------------------------------------------
struct TileSummary {
    uint32_t cnt[2];   // elements emitted when the position before the tile was not taken [0] / taken [1]
    uint32_t out[2];   // whether the tile's last position is taken, for the same two cases
};

IMC_ENC_HD inline TileSummary tile_identity() { return TileSummary{{0u, 0u}, {0u, 1u}}; }

// the summary of `s` followed by one more position whose pair flag is m
IMC_ENC_HD inline TileSummary tile_step(TileSummary s, bool m)
{
    for (int p = 0; p < 2; ++p) {
        const uint32_t before = s.out[p];
        s.cnt[p] += before ? 0u : 1u;             // the position after a taken one emits nothing
        s.out[p] = (m && !before) ? 1u : 0u;
    }
    return s;
}

// the summary of tile a followed by tile b (function composition on the carried bit: associative)
IMC_ENC_HD inline TileSummary tile_combine(const TileSummary &a, const TileSummary &b)
{
    TileSummary r;
    for (int p = 0; p < 2; ++p) {
        r.cnt[p] = a.cnt[p] + (a.out[p] ? b.cnt[1] : b.cnt[0]);   // (selects, not indexed: the fields stay in registers)
        r.out[p] = a.out[p] ? b.out[1] : b.out[0];
    }
    return r;
}

// One 32-bit word for summaries whose counts stay below 2^14 (the summaries inside a workgroup's tile).
constexpr uint32_t kPackedCountLimit = 1u << 14;
IMC_ENC_HD inline uint32_t tile_pack(const TileSummary &s) { return s.cnt[0] | s.cnt[1] << 14 | s.out[0] << 28 | s.out[1] << 29; }
IMC_ENC_HD inline TileSummary tile_unpack(uint32_t w)
{
    return TileSummary{{w & 0x3fffu, (w >> 14) & 0x3fffu}, {(w >> 28) & 1u, (w >> 29) & 1u}};
}

// ---- emit rule --------------------------------------------------------------------------------------
enum EmitKind { kEmitNothing = 0, kEmitSelf = 1, kEmitToken = 2 };

// What a position with pair flag m emits when `carry` says whether the position before it was taken; updates carry.
IMC_ENC_HD inline EmitKind emit_step(bool m, uint32_t &carry)
{
    if (carry) { carry = 0u; return kEmitNothing; }
    if (m) { carry = 1u; return kEmitToken; }
    return kEmitSelf;
}

// ---- the pairs of a pass ----------------------------------------------------------------------------
// A byte pass has one pair; a round has up to 256 keys (a << 16 | b), kept in an open-addressing set of kKeySlots
// slots.  Any exact lookup gives the same parse, so the set's layout is free; this one is shared by host and device.
constexpr uint32_t kKeySlots = 1024;           // >= 4 x the largest round
constexpr uint32_t kNoKey = 0xffffffffu;       // never a key: both halves of a key are below kMaxAlphabet
constexpr tok_t kNoToken = 0xffff;
static_assert(kKeySlots >= 4 * 256, "the key set must stay sparse");

IMC_ENC_HD inline uint32_t key_of(tok_t a, tok_t b) { return (uint32_t)a << 16 | b; }
IMC_ENC_HD inline uint32_t key_slot(uint32_t k) { return ((k * 2654435761u) >> 7) & (kKeySlots - 1); }

// token of key k, or kNoToken (at most kKeySlots probes: the set always has empty slots)
IMC_ENC_HD inline tok_t key_lookup(const uint32_t *hk, const tok_t *hv, uint32_t k)
{
    uint32_t s = key_slot(k);
    for (uint32_t probe = 0; probe < kKeySlots; ++probe) {
        const uint32_t have = hk[s];
        if (have == k) return hv[s];
        if (have == kNoKey) return kNoToken;
        s = (s + 1) & (kKeySlots - 1);
    }
    return kNoToken;
}

// host-side build of the set (the kernels insert with an LDS compare-and-swap instead)
inline void key_set_build(const PairDict &d, int z0, int nz, std::vector<uint32_t> &hk, std::vector<tok_t> &hv)
{
    hk.assign(kKeySlots, kNoKey);
    hv.assign(kKeySlots, kNoToken);
    for (int z = z0; z < z0 + nz; ++z) {
        const uint32_t k = key_of(d.left[z], d.right[z]);
        uint32_t s = key_slot(k);
        while (hk[s] != kNoKey) s = (s + 1) & (kKeySlots - 1);
        hk[s] = k;
        hv[s] = (tok_t)z;
    }
}

// ---- which passes, and which level is the stream after how many of them ------------------------------
// The order of encode_levels(): the byte merges one per pass, then the 16-bit rounds; a level is a snapshot of the
// stream between two passes.  alphabet[] and is_wide[] are what encode_levels() reports for the level.
struct EncodeSchedule {
    struct Pass { int z0, nz; };                // the pass replaces the pairs of tokens z0 .. z0 + nz - 1
    std::vector<Pass> passes;
    int after[kNumLevels];                      // level l is the stream after this many passes (0: the raw stream)
    int alphabet[kNumLevels];
    bool is_wide[kNumLevels];
};

inline EncodeSchedule encode_schedule(const PairDict &d)
{
    EncodeSchedule s;
    int lvl = 0;
    auto put = [&](int alphabet, bool wide) {
        s.after[lvl] = (int)s.passes.size();
        s.alphabet[lvl] = alphabet;
        s.is_wide[lvl] = wide;
        ++lvl;
    };
    if (d.nsym > kByteAlphabet) {
        while (lvl < kNumLevels && kLevels[lvl] <= kByteAlphabet) put(d.nsym, true);
    } else {
        auto snapshot = [&](int A) {
            while (lvl < kNumLevels && kLevels[lvl] <= A && kLevels[lvl] <= kByteAlphabet) put(std::max(d.nsym, std::min(kLevels[lvl], d.alphabet)), false);
        };
        snapshot(d.nsym);
        const int top = std::min(d.alphabet, kByteAlphabet);
        for (int z = d.nsym; z < top; ++z) {
            s.passes.push_back({z, 1});
            snapshot(z + 1);
        }
        while (lvl < kNumLevels && kLevels[lvl] <= kByteAlphabet) put(std::max(d.nsym, top), false);
    }
    for (int z0 = wide_base(d.nsym); z0 < d.alphabet; z0 += round_size(z0)) {
        const int z1 = std::min(z0 + round_size(z0), d.alphabet);
        s.passes.push_back({z0, z1 - z0});
        while (lvl < kNumLevels && kLevels[lvl] <= z1) put(z1, true);
    }
    while (lvl < kNumLevels) put(std::max(d.nsym, d.alphabet), d.alphabet > kByteAlphabet);
    return s;
}

// ---- how a chunk stores its levels -------------------------------------------------------------------
// The one rule for both encoders.  A level that repeats the alphabet of the level before it is that level's stream
// (whatever that is); otherwise a level no larger than the raw alphabet is the chunk's raw symbols and any other level
// owns a buffer.  Token occurrences (the hot-set choice of the hybrid table) are kept for the byte levels and for the
// 16-bit levels up to counted_max tokens.
enum LevelKind { kLevelRaw = 0, kLevelSame = 1, kLevelOwn = 2 };
struct LevelRule {
    LevelKind kind;
    int alphabet;
    bool is_wide;
    bool counted;
};

inline std::array<LevelRule, kNumLevels> level_rules(const EncodeSchedule &s, int nsym, int counted_max)
{
    std::array<LevelRule, kNumLevels> r;
    for (int l = 0; l < kNumLevels; ++l) {
        if (l > 0 && s.alphabet[l] == s.alphabet[l - 1]) { r[l] = r[l - 1]; r[l].kind = kLevelSame; continue; }
        const bool own = s.alphabet[l] > nsym;
        r[l] = LevelRule{own ? kLevelOwn : kLevelRaw, s.alphabet[l], s.is_wide[l], own && (!s.is_wide[l] || s.alphabet[l] <= counted_max)};
    }
    return r;
}

}  // namespace imc
