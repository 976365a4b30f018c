// encode_tiles_check.cpp - the parallel form of an encoder pass (csrc/encode_tiles.hpp) against the greedy loops of
// csrc/pair_dict.hpp, on the CPU.  The tile functions the kernels call are driven here sequentially, tile by tile:
// flags and tile summaries first, one scan over the summaries for carries and offsets, then every tile emits from its
// own carry and offset alone - the three launches of a device pass.
//   (a) one pass against replace_pair / replace_round on seq + 1: all strings over 2 and 3 symbols up to length 10, six
//       pair sets (with (a,a), (0,1)+(1,0) and the cycle (0,1),(1,2),(2,0)), and random strings with long runs
//   (b) K = 1, 2, 5 concatenated marked chunks (lengths 1 and 2 among them) against per-chunk results
//   (c) dictionaries trained on a 40k-column sample (3 symbols: byte merges then rounds; 257 symbols: rounds on the raw
//       stream): all 23 levels against encode_levels() at 4096, 4097, 8191 columns and on an all-zero chunk
// Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../imcoalhmm_amd/csrc/encode_tiles.hpp"

using imc::tok_t;

static long g_compared = 0;

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

// the pairs of one pass: tokens z0 .. z0 + nz - 1 of d
struct PassKeys {
    const imc::PairDict &d;
    int z0, nz;
    std::vector<uint32_t> hk;
    std::vector<tok_t> hv;
    PassKeys(const imc::PairDict &dict, int first, int count) : d(dict), z0(first), nz(count) { imc::key_set_build(d, z0, nz, hk, hv); }
};

// One pass over a marked 16-bit stream, tile by tile.
static std::vector<tok_t> tiled_pass(const std::vector<tok_t> &in, size_t tile, const PassKeys &pk)
{
    const size_t n = in.size();
    const imc::PairDict &d = pk.d;
    const int z0 = pk.z0, nz = pk.nz;
    const std::vector<uint32_t> &hk = pk.hk;
    const std::vector<tok_t> &hv = pk.hv;
    auto token = [&](tok_t a, tok_t b) -> tok_t {
        if (nz == 1) return (a == d.left[z0] && b == d.right[z0]) ? (tok_t)z0 : imc::kNoToken;
        return imc::key_lookup(hk.data(), hv.data(), imc::key_of(a, b));
    };
    // launch 1: flags and tile summaries
    std::vector<uint8_t> m(n, 0);
    const size_t ntiles = (n + tile - 1) / tile;
    std::vector<imc::TileSummary> sums(ntiles);
    for (size_t i = 0; i < ntiles; ++i) {
        imc::TileSummary s = imc::tile_identity();
        for (size_t t = i * tile; t < std::min(n, (i + 1) * tile); ++t) {
            m[t] = t + 1 < n && token(in[t], in[t + 1]) != imc::kNoToken;
            s = imc::tile_step(s, m[t]);
        }
        sums[i] = s;
        if (s.cnt[0] < imc::kPackedCountLimit && s.cnt[1] < imc::kPackedCountLimit) {
            const imc::TileSummary r = imc::tile_unpack(imc::tile_pack(s));
            CHECK(r.cnt[0] == s.cnt[0] && r.cnt[1] == s.cnt[1] && r.out[0] == s.out[0] && r.out[1] == s.out[1]);
        }
    }
    // launch 2: carries and offsets
    std::vector<std::pair<uint32_t, uint32_t>> tile_in(ntiles);
    imc::TileSummary run = imc::tile_identity();
    for (size_t i = 0; i < ntiles; ++i) {
        tile_in[i] = {run.cnt[0], run.out[0]};
        run = imc::tile_combine(run, sums[i]);
    }
    // launch 3: every tile on its own
    std::vector<tok_t> out(run.cnt[0]);
    for (size_t i = 0; i < ntiles; ++i) {
        uint32_t w = tile_in[i].first, carry = tile_in[i].second;
        for (size_t t = i * tile; t < std::min(n, (i + 1) * tile); ++t) {
            const imc::EmitKind kind = imc::emit_step(m[t], carry);
            if (kind == imc::kEmitNothing) continue;
            CHECK(w < out.size());
            out[w++] = kind == imc::kEmitToken ? token(in[t], in[t + 1]) : in[t];
        }
        CHECK(w == (i + 1 < ntiles ? tile_in[i + 1].first : run.cnt[0]));
    }
    return out;
}

// the host encoder's pass on one chunk: position 0 is never merged
static void greedy_pass(std::vector<tok_t> &seq, const imc::PairDict &d, int z0, int nz, bool as_round)
{
    size_t n = seq.size();
    if (n > 2) {
        if (!as_round) n = 1 + imc::replace_pair<tok_t>(seq.data() + 1, n - 1, d.left[z0], d.right[z0], (tok_t)z0);
        else {
            std::vector<uint32_t> rk;
            std::vector<tok_t> ri;
            for (int z = z0; z < z0 + nz; ++z) { rk.push_back(imc::key_of(d.left[z], d.right[z])); ri.push_back((tok_t)z); }
            n = 1 + imc::replace_round(seq.data() + 1, n - 1, rk, ri);
        }
    }
    seq.resize(n);
}

static const size_t kTiles[] = {1, 2, 3, 4, 7, 64};

static imc::PairDict small_dict(int nsym, const std::vector<std::pair<int, int>> &pairs)
{
    imc::PairDict d;
    imc::init_dict(d, nsym);
    for (auto &p : pairs) d.add(p.first, p.second);
    return d;
}

static void compare_one_pass(const std::vector<tok_t> &chunk, const PassKeys &pk)
{
    const imc::PairDict &d = pk.d;
    const int nz = pk.nz;
    std::vector<tok_t> marked = chunk;
    marked[0] |= imc::kChunkMark;
    for (int as_round = (nz == 1 ? 0 : 1); as_round < 2; ++as_round) {
        std::vector<tok_t> want = chunk;
        greedy_pass(want, d, d.nsym, nz, as_round != 0);
        want[0] |= imc::kChunkMark;
        for (size_t tile : kTiles) {
            CHECK(tiled_pass(marked, tile, pk) == want);
            ++g_compared;
        }
    }
}

static void part_a()
{
    const std::vector<std::vector<std::pair<int, int>>> sets = {
        {{0, 0}}, {{0, 1}}, {{0, 1}, {1, 0}}, {{0, 1}, {1, 2}, {2, 0}}, {{0, 0}, {0, 1}}, {{1, 1}, {1, 0}, {0, 1}}};
    for (int nsym = 2; nsym <= 3; ++nsym)
        for (auto &set : sets) {
            bool fits = true;
            for (auto &p : set) fits = fits && p.first < nsym && p.second < nsym;
            if (!fits) continue;
            const imc::PairDict d = small_dict(nsym, set);
            const PassKeys pk(d, nsym, (int)set.size());
            for (int len = 1; len <= 10; ++len) {
                size_t count = 1;
                for (int i = 0; i < len; ++i) count *= nsym;
                for (size_t code = 0; code < count; ++code) {
                    std::vector<tok_t> s(len);
                    size_t c = code;
                    for (int i = 0; i < len; ++i) { s[i] = (tok_t)(c % nsym); c /= nsym; }
                    compare_one_pass(s, pk);
                }
            }
            Rng rng(17 + nsym + set.size());
            for (int rep = 0; rep < 200; ++rep) {      // long runs: the carry crosses many tiles
                std::vector<tok_t> s(1 + rng.below(300));
                tok_t cur = 0;
                for (auto &x : s) { if (rng.below(8) == 0) cur = (tok_t)rng.below(nsym); x = cur; }
                compare_one_pass(s, pk);
            }
        }
}

// a few passes in a row on K concatenated chunks against the same passes per chunk
static void part_b()
{
    imc::PairDict d = small_dict(3, {{0, 0}, {3, 3}, {4, 4}, {0, 1}, {1, 0}, {4, 2}});
    const std::vector<PassKeys> passes = {PassKeys(d, 3, 1), PassKeys(d, 4, 1), PassKeys(d, 5, 4)};
    Rng rng(5);
    for (int K : {1, 2, 5})
        for (int rep = 0; rep < 60; ++rep) {
            std::vector<std::vector<tok_t>> chunks(K);
            std::vector<tok_t> stream;
            for (int k = 0; k < K; ++k) {
                const size_t len = (rep + k) % 4 == 0 ? 1 : (rep + k) % 4 == 1 ? 2 : 1 + rng.below(200);
                tok_t cur = 0;
                for (size_t t = 0; t < len; ++t) { if (rng.below(6) == 0) cur = (tok_t)rng.below(3); chunks[k].push_back(cur); }
                stream.insert(stream.end(), chunks[k].begin(), chunks[k].end());
                stream[stream.size() - len] |= imc::kChunkMark;
            }
            for (size_t tile : kTiles) {
                std::vector<tok_t> s = stream;
                std::vector<std::vector<tok_t>> want = chunks;
                for (auto &p : passes) {
                    s = tiled_pass(s, tile, p);
                    for (auto &c : want) greedy_pass(c, d, p.z0, p.nz, p.nz > 1);
                }
                std::vector<std::vector<tok_t>> got;
                for (tok_t x : s) {
                    if (x & imc::kChunkMark) got.emplace_back();
                    CHECK(!got.empty());
                    got.back().push_back(x & (tok_t)~imc::kChunkMark);
                }
                CHECK(got == want);
                ++g_compared;
            }
        }
}

static std::vector<int> sticky(size_t n, int nsym, uint64_t seed, uint32_t keep)
{
    Rng rng(seed);
    std::vector<int> s(n);
    int cur = 0;
    for (auto &x : s) {
        if (rng.below(100) >= keep) cur = rng.below(10) < 7 ? 0 : (int)rng.below(nsym);
        x = cur;
    }
    return s;
}

// mostly symbol 0, the others evenly (the recipe of the GPU tests' compressible())
static std::vector<int> mostly_zero(size_t n, int nsym, uint64_t seed)
{
    Rng rng(seed);
    std::vector<int> s(n);
    for (auto &x : s) x = rng.below(10) ? 0 : 1 + (int)rng.below(nsym - 1);
    return s;
}

static void compare_levels(const imc::PairDict &d, const std::vector<int> &sym, size_t tile)
{
    const size_t L = sym.size();
    const bool raw16 = d.nsym > imc::kByteAlphabet;
    std::vector<uint8_t> b(sym.begin(), sym.end());
    std::vector<tok_t> w(sym.begin(), sym.end());
    imc::EncodedLevels enc;
    imc::encode_levels(d, raw16 ? nullptr : b.data(), raw16 ? w.data() : nullptr, L, enc);
    const imc::EncodeSchedule sch = imc::encode_schedule(d);
    std::vector<tok_t> s = w;
    s[0] |= imc::kChunkMark;
    size_t applied = 0;
    for (int l = 0; l < imc::kNumLevels; ++l) {
        CHECK(sch.after[l] >= (int)applied && sch.after[l] <= (int)sch.passes.size());
        for (; applied < (size_t)sch.after[l]; ++applied) s = tiled_pass(s, tile, PassKeys(d, sch.passes[applied].z0, sch.passes[applied].nz));
        CHECK(sch.alphabet[l] == enc.alphabet[l]);
        CHECK(sch.is_wide[l] == enc.is_wide[l]);
        CHECK(s.size() == enc.length[l]);
        if (raw16 && sch.after[l] == 0) { ++g_compared; continue; }     // encode_levels keeps no copy of the raw 16-bit stream
        CHECK((s[0] & imc::kChunkMark) != 0);
        for (size_t t = 0; t < s.size(); ++t) {
            const tok_t v = s[t] & (tok_t)~imc::kChunkMark;
            CHECK(t == 0 || v == s[t]);                                  // one mark, at position 0
            CHECK(v == (enc.is_wide[l] ? enc.wide[l][t] : (tok_t)enc.bytes[l][t]));
        }
        ++g_compared;
    }
    CHECK(applied == sch.passes.size() || sch.after[imc::kNumLevels - 1] == (int)applied);
}

static void part_c()
{
    {   // 3 symbols: byte merges, then 16-bit rounds
        const std::vector<int> sample = mostly_zero(40000, 3, 11);
        std::vector<uint8_t> host(sample.begin(), sample.end());
        imc::PairDict d;
        imc::train_dict(d, 3, std::vector<uint8_t>(host.begin() + 1, host.end()), 2);
        CHECK(d.alphabet == imc::kByteAlphabet);
        const std::vector<uint8_t> lvl256 = imc::encode_bytes(d, host.data(), host.size(), nullptr);
        imc::train_dict_wide(d, std::vector<tok_t>(lvl256.begin() + 1, lvl256.end()), 2);
        CHECK(d.alphabet >= imc::kByteAlphabet + 2 * 64);          // at least two rounds
        for (size_t L : {(size_t)4096, (size_t)4097, (size_t)8191}) {
            compare_levels(d, mostly_zero(L, 3, 100 + L), 64);
            compare_levels(d, std::vector<int>(sample.begin(), sample.begin() + L), 7);
        }
        compare_levels(d, std::vector<int>(5000, 0), 64);
        compare_levels(d, std::vector<int>(4096, 0), 3);
        // a dictionary that stops inside the byte phase
        imc::PairDict small;
        imc::train_dict(small, 3, std::vector<uint8_t>(host.begin() + 1, host.begin() + 3000), 8);
        CHECK(small.alphabet > 8 && small.alphabet < imc::kByteAlphabet);
        compare_levels(small, sticky(4097, 3, 7, 90), 64);
    }
    {   // 257 symbols: no byte levels, rounds on the raw 16-bit stream
        const std::vector<int> sample = sticky(40000, 257, 12, 60);
        imc::PairDict d;
        imc::init_dict(d, 257);
        imc::train_dict_wide(d, std::vector<tok_t>(sample.begin() + 1, sample.end()), 3);
        CHECK(d.alphabet > 257 + 64);
        for (size_t L : {(size_t)4096, (size_t)4097, (size_t)8191}) compare_levels(d, sticky(L, 257, 200 + L, 60), 64);
        compare_levels(d, std::vector<int>(4500, 0), 64);
    }
}

static void algebra()
{
    // every summary a stream can have, combined three ways
    std::vector<imc::TileSummary> all;
    for (int bits = 0; bits < 32; ++bits)
        for (int len = 0; len <= 5; ++len) {
            imc::TileSummary s = imc::tile_identity();
            for (int i = 0; i < len; ++i) s = imc::tile_step(s, (bits >> i) & 1);
            all.push_back(s);
        }
    auto same = [](const imc::TileSummary &x, const imc::TileSummary &y) {
        return x.cnt[0] == y.cnt[0] && x.cnt[1] == y.cnt[1] && x.out[0] == y.out[0] && x.out[1] == y.out[1];
    };
    for (size_t a = 0; a < all.size(); a += 3)
        for (size_t b = 0; b < all.size(); b += 5)
            for (size_t c = 0; c < all.size(); c += 7) {
                CHECK(same(imc::tile_combine(imc::tile_combine(all[a], all[b]), all[c]), imc::tile_combine(all[a], imc::tile_combine(all[b], all[c]))));
                ++g_compared;
            }
    for (auto &s : all) CHECK(same(imc::tile_combine(imc::tile_identity(), s), s) && same(imc::tile_combine(s, imc::tile_identity()), s));
}

int main()
{
    algebra();
    part_a();
    part_b();
    part_c();
    std::printf("encode_tiles ok (%ld comparisons)\n", g_compared);
    return 0;
}
