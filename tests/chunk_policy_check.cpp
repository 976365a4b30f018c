// chunk_policy_check.cpp - the host-only rules behind chunk creation, on the CPU: how a chunk stores each level
// (csrc/encode_tiles.hpp: level_rules) and what a dictionary is trained on (csrc/pair_dict.hpp: train_dictionary,
// training_head, recompress_share / recompress_sample).  The training limits are scaled down (TrainLimits) so that
// chunks longer than their training head fit a test.
//   (a) level rule: for trained 3-, 65- and 257-symbol dictionaries and untrained ones, all 23 levels against
//       encode_levels() and encode_schedule(): "same as the level before" exactly when the alphabets are equal, the raw
//       stream exactly when the alphabet is at most nsym, width, and whether token counts are kept
//   (b) head claim: a dictionary trained on training_head(L) symbols is the dictionary trained on all L, for L one
//       below, at, one above and far above the head - bytes (byte phase fills 256 entries, then 16-bit rounds) and
//       16-bit raw symbols
//   (c) re-compression sample: heads of min(L_k, share) symbols give the sample the whole chunks give
// Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
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

// independent symbols: 0, 1, 2 "hot" (together 90 %: 0 alone when nsym is 3), the rest uniform
static std::vector<int> skewed(size_t n, int nsym, uint64_t seed)
{
    Rng rng(seed);
    std::vector<int> s(n);
    for (auto &x : s) {
        const uint32_t u = rng.below(100);
        if (nsym == 3) x = u < 90 ? 0 : u < 95 ? 1 : 2;
        else x = u < 90 ? (int)(u % 3) : 3 + (int)rng.below(nsym - 3);
    }
    return s;
}

static imc::TrainedDict train(const std::vector<int> &sym, size_t L, int nsym, const imc::TrainLimits &lim)
{
    if (nsym > imc::kByteAlphabet) {
        const std::vector<tok_t> w(sym.begin(), sym.begin() + L);
        return imc::train_dictionary(nullptr, w.data(), L, nsym, 0, lim.max_depth, lim);
    }
    const std::vector<uint8_t> b(sym.begin(), sym.begin() + L);
    return imc::train_dictionary(b.data(), nullptr, L, nsym, 0, lim.max_depth, lim);
}

// ---- (a) ----
static void check_levels(const imc::PairDict &d, const std::vector<int> &sym, int counted_max)
{
    const int nsym = d.nsym;
    const bool raw16 = nsym > imc::kByteAlphabet;
    const std::vector<uint8_t> b(sym.begin(), sym.end());
    const std::vector<tok_t> w(sym.begin(), sym.end());
    imc::EncodedLevels enc;
    imc::encode_levels(d, raw16 ? nullptr : b.data(), raw16 ? w.data() : nullptr, sym.size(), enc);
    const imc::EncodeSchedule sch = imc::encode_schedule(d);
    const auto rules = imc::level_rules(sch, nsym, counted_max);
    CHECK(rules.size() == (size_t)imc::kNumLevels && imc::kNumLevels == 23);
    for (int l = 0; l < imc::kNumLevels; ++l) {
        const imc::LevelRule &r = rules[l];
        CHECK(r.alphabet == enc.alphabet[l] && r.alphabet == sch.alphabet[l]);
        CHECK(r.is_wide == enc.is_wide[l] && r.is_wide == sch.is_wide[l]);
        const bool same = l > 0 && enc.alphabet[l] == enc.alphabet[l - 1];
        CHECK((r.kind == imc::kLevelSame) == same);
        int root = l;                                                            // the level whose stream this one is
        while (rules[root].kind == imc::kLevelSame) --root;
        CHECK(rules[root].alphabet == r.alphabet && sch.after[root] == sch.after[l]);
        CHECK((rules[root].kind == imc::kLevelRaw) == (enc.alphabet[l] <= nsym));
        CHECK((rules[root].kind == imc::kLevelOwn) == (enc.alphabet[l] > nsym));
        if (rules[root].kind == imc::kLevelRaw) CHECK(enc.length[l] == sym.size() && sch.after[l] == 0);
        CHECK(r.counted == (enc.alphabet[l] > nsym && (!enc.is_wide[l] || enc.alphabet[l] <= counted_max)));
        if (same) {                                                              // ... and it IS the same stream
            CHECK(enc.length[l] == enc.length[l - 1] && enc.is_wide[l] == enc.is_wide[l - 1] && r.counted == rules[l - 1].counted);
            if (rules[root].kind == imc::kLevelOwn) CHECK(enc.bytes[l] == enc.bytes[l - 1] && enc.wide[l] == enc.wide[l - 1]);   // (of raw levels
                                                                                 // encode_levels() keeps a copy of some only)
        }
        if (rules[root].kind == imc::kLevelOwn) {
            CHECK((enc.is_wide[l] ? enc.wide[l].size() : enc.bytes[l].size()) == enc.length[l]);
            for (size_t t = 1; t < enc.length[l]; ++t) CHECK((enc.is_wide[l] ? (int)enc.wide[l][t] : (int)enc.bytes[l][t]) < r.alphabet);
        }
        ++g_compared;
    }
}

static void part_a(const imc::PairDict &d3, const imc::PairDict &d257)
{
    imc::TrainLimits lim;
    lim.train_min = 32768; lim.train_max = 200000; lim.wide_train_tokens = 4000;
    const imc::TrainedDict t65 = train(skewed(200000, 65, 31), 200000, 65, lim);
    CHECK(t65.dict.alphabet > 65 && d3.alphabet > imc::kByteAlphabet && d257.alphabet > 257);
    CHECK(t65.depth == imc::dict_depths(t65.dict) && t65.order == imc::dict_order(t65.dict, t65.depth));
    imc::PairDict bare3, bare257;
    imc::init_dict(bare3, 3);
    imc::init_dict(bare257, 257);
    for (int counted_max : {4096, 384}) {
        check_levels(d3, skewed(5000, 3, 41), counted_max);
        check_levels(t65.dict, skewed(5000, 65, 42), counted_max);
        check_levels(d257, skewed(5000, 257, 43), counted_max);
        check_levels(bare3, skewed(4097, 3, 44), counted_max);
        check_levels(bare257, skewed(4097, 257, 45), counted_max);
    }
}

// ---- (b) ----
static imc::PairDict head_claim(int nsym, const imc::TrainLimits &lim, size_t far, uint64_t seed)
{
    const bool raw16 = nsym > imc::kByteAlphabet;
    const std::vector<int> sym = skewed(far, nsym, seed);
    const size_t head = imc::training_head(far, raw16, lim);
    CHECK(head < far);
    imc::PairDict last;
    for (size_t L : {head - 1, head, head + 1, far}) {
        const size_t h = imc::training_head(L, raw16, lim);
        CHECK(h == std::min(L, head));
        const imc::TrainedDict whole = train(sym, L, nsym, lim), part = train(sym, h, nsym, lim);
        CHECK(whole.dict.alphabet > imc::wide_base(nsym));                       // the 16-bit rounds ran
        CHECK(part.dict.alphabet == whole.dict.alphabet && part.dict.left == whole.dict.left && part.dict.right == whole.dict.right);
        CHECK(part.depth == whole.depth && part.order == whole.order);
        last = whole.dict;
        ++g_compared;
    }
    return last;
}

// ---- (c) ----
static void part_c()
{
    imc::TrainLimits lim;
    lim.train_min = 1000; lim.train_max = 20000; lim.wide_train_tokens = 300;   // budgets: 28800 bytes, 2400 16-bit symbols
    CHECK(imc::recompress_share(1, false, lim) == 28800 && imc::recompress_share(5, false, lim) == 5760 && imc::recompress_share(40, false, lim) == 1000);
    CHECK(imc::recompress_share(2, true, lim) == 1200 && imc::recompress_share(3, true, lim) == 1000);
    CHECK(imc::recompress_share(32, false) == std::max<size_t>((size_t)32768, ((size_t)96 << 19) / 32));
    for (size_t unit : {(size_t)1, (size_t)2}) {
        const std::vector<size_t> lengths = {7000, 999, 1000, 1001, 5760, 5761, 1, 12000, 5759};
        const size_t share = imc::recompress_share(5, unit == 2, lim);
        std::vector<std::vector<uint8_t>> whole, heads;
        std::vector<uint8_t> expect;
        Rng rng(77 + unit);
        for (size_t L : lengths) {
            std::vector<uint8_t> c(L * unit);
            for (auto &x : c) x = (uint8_t)rng.below(251);
            whole.push_back(c);
            heads.push_back(std::vector<uint8_t>(c.begin(), c.begin() + std::min(L, share) * unit));
            expect.insert(expect.end(), heads.back().begin(), heads.back().end());
        }
        CHECK(imc::recompress_sample(heads, share, unit) == expect);
        CHECK(imc::recompress_sample(whole, share, unit) == expect);
        g_compared += 2;
    }
}

int main()
{
    CHECK(imc::TrainLimits().zip_min_columns == 4096 && imc::compressible(4096, 3) && !imc::compressible(4095, 3));
    CHECK(imc::compressible(5000, imc::kMaxAlphabet / 2 - 1) && !imc::compressible(5000, imc::kMaxAlphabet / 2));
    const imc::TrainLimits def;
    CHECK(imc::training_head((size_t)1 << 30, false, def) == (size_t)96 << 19 && imc::training_head((size_t)1 << 30, true, def) == ((size_t)8 << 19) + 1);
    CHECK(imc::wide_min_count(400000, 0) == 6 && imc::wide_min_count(399999, 0) == 4 && imc::wide_min_count(199999, 0) == 3 && imc::wide_min_count(400000, 2) == 2);

    imc::TrainLimits bytes;                       // head: 1 500 001 columns
    bytes.train_min = 32768; bytes.train_max = 1500000; bytes.wide_train_tokens = 12000;
    const imc::PairDict d3 = head_claim(3, bytes, 3000000, 5);
    imc::TrainLimits wide;                        // head: 32 001 columns
    wide.train_min = 32768; wide.wide_train_tokens = 4000;
    const imc::PairDict d257 = head_claim(257, wide, 100000, 6);
    part_a(d3, d257);
    part_c();
    std::printf("chunk_policy ok (%ld comparisons)\n", g_compared);
    return 0;
}
