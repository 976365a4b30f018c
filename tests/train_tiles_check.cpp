// train_tiles_check.cpp - dictionary training in its parallel form (csrc/train_tiles.hpp) against the host trainer
// (csrc/pair_dict.hpp: train_dict, train_dict_wide, train_dictionary), on the CPU.  The backend below does what the
// kernels of csrc/kernels_train.hpp do, with the functions they call, in a deliberately scrambled order:
//   byte phase   per-tile histograms of pair_bin() - every "thread" merges equal consecutive keys of its own items first,
//                bins kept per tile while pair_bins_in_lds() and added directly beyond - summed over the tiles in shuffled
//                order; the winner from per-thread folds combined by best_combine() in shuffled tree order
//   rounds       count_table_add() of the per-thread runs in shuffled order; the slots at or above the threshold listed
//                in shuffled order
// and imc::train_with() drives it exactly as it drives the device.  Tile sizes 1, 2, 3, 4, 7 and 64; the training limits
// are scaled down.  Every dictionary is compared entry for entry (left, right, alphabet, depth, order) and so are the
// statistics of imc_last_training.  The branches the device trainer must reach are counted and printed; the check fails
// if one of them was never reached.
// Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../imcoalhmm_amd/csrc/train_tiles.hpp"

using imc::tok_t;

static long g_dicts = 0, g_steps = 0, g_rounds = 0;
static long g_retry8 = 0, g_retry2 = 0, g_cap_excluded_top = 0, g_short_round = 0, g_full_alphabet = 0, g_joint_only = 0, g_ended_short = 0,
            g_lds_hist = 0, g_global_hist = 0, g_reencoded = 0, g_ties = 0;

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
    template <class T>
    void shuffle(std::vector<T> &v)
    {
        for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[below((uint32_t)i)]);
    }
};

// ---- the backend ------------------------------------------------------------------------------------------
struct TileBackend {
    std::vector<std::vector<tok_t>> pieces;
    size_t tile, items;
    Rng rng;
    std::vector<tok_t> seq, spare;
    std::vector<tok_t> left, right;
    std::vector<int> depth;                       // the "device dictionary": what k_trn_argmax appends to

    TileBackend(std::vector<std::vector<tok_t>> p, int nsym, size_t tile_, uint64_t seed)
        : pieces(std::move(p)), tile(tile_), items(tile_ >= 64 ? 16 : tile_ >= 3 ? 3 : tile_), rng(seed), left(imc::kMaxAlphabet, 0), right(imc::kMaxAlphabet, 0),
          depth(imc::kMaxAlphabet, 0)
    {
        (void)nsym;
    }
    int load(size_t first, size_t count)
    {
        std::vector<size_t> len;
        for (const auto &p : pieces) len.push_back(p.size());
        seq.assign(count, 0xffff);
        size_t covered = 0;
        for (const imc::SampleRange &r : imc::sample_ranges(len, first, count)) {
            CHECK(r.piece < pieces.size() && r.src_first + r.count <= pieces[r.piece].size() && r.dst_first + r.count <= count && r.dst_first == covered);
            for (size_t t = 0; t < r.count; ++t) seq[r.dst_first + t] = pieces[r.piece][r.src_first + t];
            covered += r.count;
        }
        CHECK(covered == count);
        return 0;
    }
    // the runs of one thread's items: (key, count) with equal consecutive keys merged; key(t) for t + 1 < n
    template <class Key, class Emit>
    void thread_runs(size_t base, size_t n, Key key, Emit emit) const
    {
        bool have = false;
        uint32_t run_key = 0, run_n = 0;
        for (size_t i = 0; i < items; ++i) {
            const size_t t = base + i;
            if (t + 1 >= n) break;
            const uint32_t k = key(t);
            if (have && k == run_key) { ++run_n; continue; }
            if (have) emit(run_key, run_n);
            have = true; run_key = k; run_n = 1;
        }
        if (have) emit(run_key, run_n);
    }
    std::vector<uint32_t> pair_counts(uint32_t A)
    {
        const size_t n = seq.size();
        std::vector<uint32_t> counts((size_t)A * A, 0);
        std::vector<size_t> tiles;
        for (size_t b = 0; b < n; b += tile) tiles.push_back(b);
        rng.shuffle(tiles);
        const bool lds = imc::pair_bins_in_lds(A);
        ++(lds ? g_lds_hist : g_global_hist);
        for (size_t b : tiles) {
            std::vector<uint32_t> bins(lds ? (size_t)A * A : 0, 0);
            for (size_t th = b; th < std::min(b + tile, n); th += items) {
                // (a thread's items end with its tile: the pair that straddles the edge belongs to the tile of its first element)
                const size_t hi = std::min(b + tile, n);
                bool have = false;
                uint32_t run_key = 0, run_n = 0;
                for (size_t t = th; t < std::min(th + items, hi); ++t) {
                    if (t + 1 >= n) break;
                    const uint32_t k = imc::pair_bin(seq[t], seq[t + 1], A);
                    if (have && k == run_key) { ++run_n; continue; }
                    if (have) (lds ? bins : counts)[run_key] += run_n;
                    have = true; run_key = k; run_n = 1;
                }
                if (have) (lds ? bins : counts)[run_key] += run_n;
            }
            for (size_t k = 0; k < bins.size(); ++k)
                if (bins[k]) counts[k] += bins[k];
        }
        return counts;
    }
    imc::PairBest winner(const std::vector<uint32_t> &counts, uint32_t A, int max_depth)
    {
        const size_t threads = 37;
        std::vector<imc::PairBest> leaf(threads, imc::best_identity());
        for (size_t th = 0; th < threads; ++th)
            for (size_t bin = th; bin < counts.size(); bin += threads) {
                const uint32_t a = (uint32_t)bin / A, b = (uint32_t)bin % A;
                if (imc::pair_eligible(counts[bin], depth[a], depth[b], max_depth)) leaf[th] = imc::best_combine(leaf[th], imc::PairBest{counts[bin], (uint32_t)bin});
            }
        rng.shuffle(leaf);
        while (leaf.size() > 1) {                  // a tree over a shuffled order: pairs, then pairs of pairs ...
            std::vector<imc::PairBest> next;
            for (size_t i = 0; i + 1 < leaf.size(); i += 2) next.push_back(rng.below(2) ? imc::best_combine(leaf[i], leaf[i + 1]) : imc::best_combine(leaf[i + 1], leaf[i]));
            if (leaf.size() & 1) next.push_back(leaf.back());
            leaf.swap(next);
        }
        return leaf[0];
    }
    int byte_step(int A, int max_depth, imc::ByteStep *s)
    {
        CHECK(seq.size() >= 2 && A < imc::kByteAlphabet);
        const std::vector<uint32_t> counts = pair_counts((uint32_t)A);
        const imc::PairBest w = winner(counts, (uint32_t)A, max_depth);
        // the host's own scan (train_dict), for this one step
        uint64_t best = 0, free_best = 0, ties = 0;
        int ba = -1, bb = -1;
        for (int a = 0; a < A; ++a)
            for (int b = 0; b < A; ++b) {
                const uint64_t c = counts[(size_t)a * A + b];
                free_best = std::max(free_best, c);
                if (c > best && (max_depth <= 0 || std::max(depth[a], depth[b]) < max_depth)) { best = c; ba = a; bb = b; ties = 0; }
                else if (c == best && c) ++ties;
            }
        CHECK((ba < 0) == (w.count == 0));
        if (ba >= 0) CHECK(w.count == best && w.key == (uint32_t)(ba * A + bb));
        if (free_best > best) ++g_cap_excluded_top;
        if (ties) ++g_ties;
        ++g_steps;
        spare = seq;
        size_t nn = seq.size();
        if (w.count) {
            const uint32_t a = w.key / (uint32_t)A, b = w.key % (uint32_t)A;
            left[A] = (tok_t)a; right[A] = (tok_t)b; depth[A] = 1 + std::max(depth[a], depth[b]);
            nn = imc::replace_pair<tok_t>(spare.data(), spare.size(), (tok_t)a, (tok_t)b, (tok_t)A);
            *s = imc::ByteStep{a, b, w.count, (uint32_t)nn};
        } else
            *s = imc::ByteStep{0, 0, 0, (uint32_t)nn};
        spare.resize(nn);
        return 0;
    }
    void accept() { seq.swap(spare); }
    void truncate(size_t keep) { seq.resize(std::min(seq.size(), keep)); }
    int count_round(size_t threshold, std::vector<imc::RoundCandidate> &found)
    {
        const size_t n = seq.size();
        CHECK(n >= 2);
        const uint32_t cap = imc::count_table_capacity(n);
        CHECK((cap & (cap - 1)) == 0 && cap >= 2 * n);
        std::vector<std::pair<uint32_t, uint32_t>> runs;
        for (size_t base = 0; base < n; base += items)
            thread_runs(base, n, [&](size_t t) { return imc::key_of(seq[t], seq[t + 1]); }, [&](uint32_t k, uint32_t c) { runs.push_back({k, c}); });
        rng.shuffle(runs);
        std::vector<uint32_t> keys(cap, imc::kNoKey), counts(cap, 0);
        for (const auto &r : runs) CHECK(imc::count_table_add(keys, counts, r.first, r.second));
        std::vector<uint32_t> slots(cap);
        for (uint32_t s = 0; s < cap; ++s) slots[s] = s;
        rng.shuffle(slots);
        uint64_t sum = 0;
        for (uint32_t s : slots) {
            sum += counts[s];
            if (keys[s] != imc::kNoKey && counts[s] >= threshold) found.push_back({(uint64_t)counts[s], keys[s]});
        }
        CHECK(sum == n - 1);
        ++g_rounds;
        return 0;
    }
    int apply(const imc::PairDict &d, int z0, int nz, size_t *new_n)
    {
        CHECK(nz >= 1 && nz <= 256 && z0 + nz <= d.alphabet && !seq.empty());
        if (z0 >= imc::wide_base(d.nsym) && nz < imc::round_size(z0)) ++g_short_round;
        if (nz == 1) seq.resize(imc::replace_pair<tok_t>(seq.data(), seq.size(), d.left[z0], d.right[z0], (tok_t)z0));
        else {
            std::vector<uint32_t> rk;
            std::vector<tok_t> ri;
            for (int z = z0; z < z0 + nz; ++z) { rk.push_back(imc::key_of(d.left[z], d.right[z])); ri.push_back((tok_t)z); }
            seq.resize(imc::replace_round(seq.data(), seq.size(), rk, ri));
        }
        if (z0 < imc::wide_base(d.nsym)) ++g_reencoded;
        *new_n = seq.size();
        return 0;
    }
};

// ---- comparison ---------------------------------------------------------------------------------------------
static std::vector<tok_t> concat(const std::vector<std::vector<tok_t>> &pieces)
{
    std::vector<tok_t> all;
    for (const auto &p : pieces) all.insert(all.end(), p.begin(), p.end());
    return all;
}

struct Outcome {
    imc::TrainedDict t;
    imc::TrainStats st;
};

static Outcome compare(const std::vector<std::vector<tok_t>> &pieces, int nsym, size_t forced, int max_depth, const imc::TrainLimits &lim, const char *what)
{
    const std::vector<tok_t> all = concat(pieces);
    const size_t L = all.size();
    CHECK(L >= 2);
    for (tok_t x : all) CHECK((int)x < nsym);
    Outcome host;
    if (nsym > imc::kByteAlphabet) host.t = imc::train_dictionary(nullptr, all.data(), L, nsym, forced, max_depth, lim, &host.st);
    else {
        const std::vector<uint8_t> b(all.begin(), all.end());
        host.t = imc::train_dictionary(b.data(), nullptr, L, nsym, forced, max_depth, lim, &host.st);
    }
    uint64_t seed = 1;
    for (size_t tile : {(size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)7, (size_t)64}) {
        if ((tile < 7 && L > 5000) || (tile < 64 && L > 100000)) continue;   // (the smallest tiles on the short streams only: the check runs under sanitizers)
        TileBackend be(pieces, nsym, tile, 977 * seed++ + L);
        imc::TrainedDict t;
        imc::TrainStats st;
        CHECK(imc::train_with(be, L, nsym, forced, max_depth, lim, t, st) == 0);
        if (!(t.dict.alphabet == host.t.dict.alphabet && t.dict.left == host.t.dict.left && t.dict.right == host.t.dict.right)) {
            std::printf("FAILED %s, tile %zu: alphabet %d against the host's %d\n", what, tile, t.dict.alphabet, host.t.dict.alphabet);
            std::exit(1);
        }
        CHECK(t.dict.nsym == host.t.dict.nsym && t.dict.span == host.t.dict.span);
        CHECK(t.depth == host.t.depth && t.order == host.t.order);
        CHECK(st.sample == host.st.sample && st.attempts == host.st.attempts && st.rounds == host.st.rounds);
        ++g_dicts;
    }
    // (n < 2 ends a phase only before its first merge: a merge needs two occurrences at the least in the byte phase, and a round
    // that leaves one element was a short round, which is the last one anyway)
    if (L - 1 < 2) ++g_ended_short;
    if (host.st.attempts >= 2) ++g_retry8;
    if (host.st.attempts >= 3) ++g_retry2;
    if (host.t.dict.alphabet == imc::kMaxAlphabet) ++g_full_alphabet;
    return host;
}

static Outcome compare1(const std::vector<tok_t> &sym, int nsym, size_t forced, int max_depth, const imc::TrainLimits &lim, const char *what)
{
    return compare(std::vector<std::vector<tok_t>>{sym}, nsym, forced, max_depth, lim, what);
}

// ---- streams --------------------------------------------------------------------------------------------------
static std::vector<tok_t> uniform(size_t n, int nsym, uint64_t seed)
{
    Rng rng(seed);
    std::vector<tok_t> s(n);
    for (auto &x : s) x = (tok_t)rng.below((uint32_t)nsym);
    return s;
}
static std::vector<tok_t> skewed(size_t n, int nsym, uint64_t seed)   // symbol 0 at 90 %
{
    Rng rng(seed);
    std::vector<tok_t> s(n);
    for (auto &x : s) x = (tok_t)(rng.below(100) < 90 || nsym < 2 ? 0 : 1 + rng.below((uint32_t)nsym - 1));
    return s;
}
static std::vector<tok_t> sticky(size_t n, int nsym, uint64_t seed)   // long runs: the symbol changes with probability 1 / 50
{
    Rng rng(seed);
    std::vector<tok_t> s(n);
    tok_t cur = 0;
    for (auto &x : s) {
        if (rng.below(50) == 0) cur = (tok_t)rng.below((uint32_t)nsym);
        x = cur;
    }
    return s;
}
static std::vector<tok_t> periodic(size_t n, int period)
{
    std::vector<tok_t> s(n, 0);
    for (size_t t = 0; t < n; ++t) s[t] = (tok_t)(period > 1 && t % period == (size_t)period - 1 ? 1 : 0);
    return s;
}
// every ordered pair of distinct symbols equally often: (x, y) blocks in rotation, so that many bins tie
static std::vector<tok_t> many_ties(size_t n, int nsym)
{
    std::vector<tok_t> s;
    while (s.size() + 2 <= n)
        for (int a = 0; a < nsym && s.size() + 2 <= n; ++a)
            for (int b = 0; b < nsym && s.size() + 2 <= n; ++b)
                if (a != b) { s.push_back((tok_t)a); s.push_back((tok_t)b); }
    return s;
}

static imc::TrainLimits scaled(size_t train_min, size_t train_max, size_t wide_tokens, size_t wide_min)
{
    imc::TrainLimits lim;
    lim.zip_min_columns = 64; lim.train_min = train_min; lim.train_max = train_max; lim.wide_train_tokens = wide_tokens; lim.wide_min_count = wide_min;
    return lim;
}

// the raw expansion of token z
static void expand(const imc::PairDict &d, int z, std::vector<tok_t> &out)
{
    if (z < d.nsym) { out.push_back((tok_t)z); return; }
    expand(d, d.left[z], out);
    expand(d, d.right[z], out);
}

int main()
{
    const imc::TrainLimits lim = scaled(2000, 20000, 600, 6), lim_long = scaled(2000, 6000, 300, 6);
    // ---- sample_ranges on its own ----
    {
        const std::vector<size_t> len = {5, 0, 3, 7};
        for (size_t first = 0; first <= 15; ++first)
            for (size_t count = 0; first + count <= 15; ++count) {
                size_t covered = 0;
                for (const imc::SampleRange &r : imc::sample_ranges(len, first, count)) {
                    CHECK(r.count > 0 && r.dst_first == covered && r.src_first + r.count <= len[r.piece]);
                    size_t at = 0;
                    for (size_t k = 0; k < r.piece; ++k) at += len[k];
                    CHECK(at + r.src_first == first + covered);
                    covered += r.count;
                }
                CHECK(covered == count);
            }
    }
    // ---- alphabets x stream kinds ----
    for (int nsym : {2, 3, 4, 65, 257, 1000}) {
        for (size_t n : {(size_t)2, (size_t)3, (size_t)65, (size_t)2000, (size_t)9001}) {
            const std::string tag = "nsym " + std::to_string(nsym) + ", n " + std::to_string(n);
            compare1(uniform(n, nsym, 11 + n), nsym, 0, 0, lim, ("uniform, " + tag).c_str());
            compare1(skewed(n, nsym, 12 + n), nsym, 0, 0, lim, ("skewed, " + tag).c_str());
            compare1(sticky(n, nsym, 13 + n), nsym, 0, 0, lim, ("sticky, " + tag).c_str());
            compare1(skewed(n, nsym, 14 + n), nsym, 0, 0, lim_long, ("skewed, longer than the byte sample, " + tag).c_str());
        }
        // all equal, alternating, period 3: the stream collapses and a phase ends by n < 2
        for (size_t n : {(size_t)2, (size_t)5, (size_t)64, (size_t)4097, (size_t)16385}) {
            for (int period : {1, 2, 3}) {
                const Outcome o = compare1(periodic(n, period), nsym, 0, 0, lim, "periodic");
                (void)o;
            }
        }
        if (nsym <= 65) compare1(many_ties(8000, nsym), nsym, 0, 0, lim, "ties");
        // forced count and depth cap
        compare1(skewed(12000, nsym, 77), nsym, 2, 0, lim, "forced count 2");
        for (int cap : {1, 3}) compare1(skewed(12000, nsym, 78), nsym, 0, cap, lim, "depth cap");
        compare1(sticky(12000, nsym, 79), nsym, 2, 3, lim, "forced count and depth cap");
    }
    // ---- rounds that look further than the byte phase did: the head is encoded again with the byte dictionary ----
    {
        const long before = g_reencoded;
        int wide = 0;
        for (int nsym : {2, 3, 4, 65}) {      // (byte sample 20000 symbols, the rounds' head 30011)
            wide += compare1(uniform(30011, nsym, 14), nsym, 0, 0, lim, "uniform, longer than the byte sample").t.dict.alphabet > imc::kByteAlphabet;
            wide += compare1(sticky(30011, nsym, 15), nsym, 0, 0, lim, "sticky, longer than the byte sample").t.dict.alphabet > imc::kByteAlphabet;
            wide += compare1(skewed(30011, nsym, 16), nsym, 0, 0, lim, "skewed, longer than the byte sample").t.dict.alphabet > imc::kByteAlphabet;
        }
        CHECK(wide > 0 && g_reencoded > before);
    }
    // ---- the retry loop: a byte phase that stops at 192..255 tokens with threshold 64 ----
    for (int nsym : {170, 190, 230})
        for (size_t n : {(size_t)2500, (size_t)8000})
            for (uint64_t seed : {1}) {
                Rng rng(seed * 1000 + n + nsym);
                std::vector<tok_t> s(n);
                for (auto &x : s) x = (tok_t)(rng.below(100) < 80 ? rng.below(4) : rng.below((uint32_t)nsym));
                compare1(s, nsym, 0, 0, lim, "retry");
                compare1(s, nsym, 0, 4, lim, "retry under a depth cap");
            }
    // ---- the full alphabet: 16384 tokens under scaled limits ----
    {
        const imc::TrainLimits big = scaled(2000, 20000, 40000, 2);
        const Outcome o = compare1(uniform(200000, 600, 5), 600, 0, 0, big, "full alphabet");
        std::printf("full alphabet: %d tokens after %llu rounds\n", o.t.dict.alphabet, (unsigned long long)o.st.rounds);
    }
    // ---- a recompression sample: a pair that exists only across the joints of the chunks' heads ----
    {
        std::vector<std::vector<tok_t>> pieces;
        Rng rng(99);
        for (int k = 0; k < 220; ++k) {
            std::vector<tok_t> p(30 + rng.below(20));
            for (auto &x : p) x = (tok_t)(rng.below(10) ? 0 : 3);
            p.front() = 2;                          // 2 only ever starts a piece, 1 only ever ends one
            p.back() = 1;
            pieces.push_back(p);
        }
        const Outcome o = compare(pieces, 4, 0, 0, lim, "joints");
        for (int z = 4; z < o.t.dict.alphabet; ++z) {
            std::vector<tok_t> raw;
            expand(o.t.dict, z, raw);
            for (size_t t = 0; t + 1 < raw.size(); ++t)
                if (raw[t] == 1 && raw[t + 1] == 2) { ++g_joint_only; break; }
        }
        // 16-bit raw pieces
        std::vector<std::vector<tok_t>> wide;
        for (int k = 0; k < 60; ++k) wide.push_back(skewed(100 + k, 300, 500 + k));
        compare(wide, 300, 0, 0, lim, "joints, 16-bit raw");
    }
    std::printf("dictionaries compared %ld, byte steps %ld, rounds %ld\n", g_dicts, g_steps, g_rounds);
    std::printf("branches: retry with threshold 8 %ld, with threshold 2 %ld, depth cap excluded the top pair %ld, short last round %ld, "
                "alphabet 16384 %ld, joint-only pair merged %ld, phase ended by n < 2 %ld, LDS histograms %ld, global histograms %ld, "
                "re-encoded heads (passes) %ld, steps with tied counts %ld\n",
                g_retry8, g_retry2, g_cap_excluded_top, g_short_round, g_full_alphabet, g_joint_only, g_ended_short, g_lds_hist, g_global_hist,
                g_reencoded, g_ties);
    CHECK(g_retry8 > 0 && g_retry2 > 0 && g_cap_excluded_top > 0 && g_short_round > 0 && g_full_alphabet > 0 && g_joint_only > 0);
    CHECK(g_ended_short > 0 && g_lds_hist > 0 && g_global_hist > 0 && g_reencoded > 0 && g_ties > 0);
    std::printf("train_tiles ok\n");
    return 0;
}
