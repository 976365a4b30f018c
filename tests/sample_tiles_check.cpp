// The parallel form of the HMM sampler (imcoalhmm_amd/csrc/sample_tiles.hpp) against its sequential specification, on the
// CPU under AddressSanitizer + UBSan (tests/test_sample_tiles_cpu.py builds and runs this file).  The functions the kernels
// call - the summary step, the combine and the tile walk - are driven tile by tile at tile lengths 1, 2, 3, 7, 64 and 4096
// against sample_sequential(): N in {1, 2, 3, 20, 65, 256}, one and three replicates whose starts fall inside tiles,
// sticky / fast-mixing / sparse / cyclic-permutation / absorbing / banded (leading and trailing zeros) / unnormalised T.
// Also: the Philox known answers, the threshold rules, associativity of the combine on random maps.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../imcoalhmm_amd/csrc/sample_tiles.hpp"

namespace {

long g_compared = 0;

#define CHECK(cond, ...)                                                                \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                \
            std::printf(__VA_ARGS__);                                                   \
            std::printf("\n");                                                          \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

struct Rng {   // splitmix64: the test's own generator, unrelated to the sampler's
    uint64_t x;
    explicit Rng(uint64_t seed) : x(seed) {}
    uint64_t next()
    {
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double unit() { return (double)(next() >> 11) * 0x1.0p-53; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

enum Kind { kSticky, kFast, kSparse, kCyclic, kAbsorbing, kBanded, kUnnormalised, kKinds };
const char *kind_name[kKinds] = {"sticky", "fast-mixing", "sparse", "cyclic", "absorbing", "banded", "unnormalised"};

std::vector<double> transitions(Kind kind, int N, Rng &rng)
{
    std::vector<double> T((size_t)N * N, 0.0);
    for (int i = 0; i < N; ++i) {
        double *row = &T[(size_t)i * N];
        switch (kind) {
        case kSticky:
            for (int j = 0; j < N; ++j) row[j] = 0.001 * rng.unit() / N;
            row[i] += 0.999;
            break;
        case kFast:
            for (int j = 0; j < N; ++j) row[j] = rng.unit() + 1e-3;
            break;
        case kSparse:
            for (int k = 0; k < 3; ++k) row[rng.below(N)] += rng.unit() + 0.05;
            break;
        case kCyclic:
            row[(i + 1) % N] = 1.0;
            break;
        case kAbsorbing:
            if (i == N / 2) row[i] = 1.0;
            else for (int j = 0; j < N; ++j) row[j] = rng.unit() + 1e-3;
            break;
        case kBanded:   // zeros before N/4 and from 3N/4 on
            for (int j = N / 4; j < std::max(N / 4 + 1, 3 * N / 4); ++j) row[j] = rng.unit() + 1e-3;
            break;
        case kUnnormalised: {
            const double scale = 0.1 + 50.0 * rng.unit();
            for (int j = 0; j < N; ++j) row[j] = scale * (rng.unit() + 1e-3);
            break;
        }
        default: break;
        }
    }
    return T;
}

template <class Sym>
void run_case(Kind kind, int N, int S, int emit, int R, uint64_t L, uint64_t seed, uint32_t tag)
{
    Rng rng(seed * 1000003u + (uint64_t)N * 131u + (uint64_t)kind);
    const std::vector<double> T = transitions(kind, N, rng);
    std::vector<double> pi(N), E((size_t)N * S);
    for (double &v : pi) v = rng.unit() + 1e-3;
    if (N > 2) pi[0] = 0.0, pi[N - 1] = 0.0;               // leading and trailing zero
    for (double &v : E) v = rng.unit() + 0.05;
    imc::SampleTables tb;
    std::string err;
    CHECK(imc::build_tables(N, S, emit, pi.data(), T.data(), E.data(), &tb, &err), "%s", err.c_str());

    const uint64_t total = (uint64_t)R * L;
    std::vector<Sym> want_sym(total), got_sym(total);
    std::vector<uint8_t> want_st(total), got_st(total);
    imc::sample_sequential(tb, seed, tag, R, L, want_sym.data(), want_st.data());
    for (uint64_t g = 0; g < total; ++g) {
        CHECK(want_st[g] < N && (int)want_sym[g] < emit, "%s N=%d column %llu out of range", kind_name[kind], N, (unsigned long long)g);
        if (g % L) CHECK(T[(size_t)want_st[g - 1] * N + want_st[g]] > 0.0, "%s N=%d: a transition of probability zero at column %llu", kind_name[kind], N, (unsigned long long)g);
        else CHECK(pi[want_st[g]] > 0.0, "a start state of probability zero");
    }
    {   // without the states
        std::vector<Sym> again(total);
        imc::sample_sequential(tb, seed, tag, R, L, again.data(), (uint8_t *)nullptr);
        CHECK(again == want_sym, "symbols depend on whether states are asked for");
    }

    for (uint64_t tile : {1u, 2u, 3u, 7u, 64u, 4096u}) {
        const uint64_t M = imc::sample_tile_count(total, tile);
        std::vector<uint8_t> maps(M * N), enter(M);
        for (uint64_t j = 0; j < M; ++j)
            imc::summarise_tile(j * tile, std::min(total, (j + 1) * tile), L, seed, tag, tb.T(), N, &maps[j * N]);
        // entering states: blocks of five tiles combined first, then block to block - another association than the walk's
        std::vector<uint8_t> block(N);   // (what enters tile 0 is irrelevant: start from N - 1)
        int s = N - 1;
        for (uint64_t j0 = 0; j0 < M; j0 += 5) {
            const uint64_t j1 = std::min(M, j0 + 5);
            imc::map_identity(block.data(), N);
            int inner = s;
            for (uint64_t j = j0; j < j1; ++j) {
                enter[j] = (uint8_t)inner;
                inner = maps[j * N + inner];
                imc::map_combine(block.data(), &maps[j * N], block.data(), N);
            }
            CHECK(block[s] == inner, "block map disagrees with tile-by-tile application");
            s = block[s];
        }
        std::fill(got_sym.begin(), got_sym.end(), (Sym)0xEE);
        std::fill(got_st.begin(), got_st.end(), (uint8_t)0xEE);
        for (uint64_t j = 0; j < M; ++j) {
            const int out = imc::walk_tile(enter[j], j * tile, std::min(total, (j + 1) * tile), L, seed, tag, tb.T(), tb.E(), N, emit, got_sym.data(), got_st.data());
            CHECK(out == maps[j * N + enter[j]], "%s N=%d tile %llu: walk and summary disagree", kind_name[kind], N, (unsigned long long)j);
        }
        for (uint64_t g = 0; g < total; ++g)
            CHECK(got_sym[g] == want_sym[g] && got_st[g] == want_st[g], "%s N=%d R=%d L=%llu tile=%llu: column %llu differs", kind_name[kind], N, R,
                  (unsigned long long)L, (unsigned long long)tile, (unsigned long long)g);
        g_compared += (long)total;
        if (kind == kCyclic)                                // every map is a bijection: the entering state matters everywhere
            for (uint64_t j = 0; j < M; ++j)
                if ((j * tile) % L != 0 && (j * tile) / L == ((j + 1) * tile - 1) / L && (j + 1) * tile <= total) {
                    std::vector<bool> seen(N, false);
                    for (int i = 0; i < N; ++i) seen[maps[j * N + i]] = true;
                    for (int i = 0; i < N; ++i) CHECK(seen[i], "cyclic N=%d: the map of tile %llu is not a bijection", N, (unsigned long long)j);
                }
    }
}

void check_philox()
{
    struct { uint32_t ctr[4], key[2], out[4]; } kat[3] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    for (auto &k : kat) {
        uint32_t w[4];
        imc::philox4x32_10(k.ctr, k.key, w);
        CHECK(std::memcmp(w, k.out, sizeof w) == 0, "Philox known answer: %08x %08x %08x %08x", w[0], w[1], w[2], w[3]);
    }
    // counter and key layout, and the two uniforms
    const uint64_t seed = 0x299f31d0a4093822ull, t = 0x85a308d3243f6a88ull;
    double us, uy;
    imc::column_uniforms(seed, 0x03707344u, 0x13198a2eu, t, &us, &uy);
    CHECK(us == (double)((0x94fdccebd16cfe09ull) >> 11) * 0x1.0p-53 && uy == (double)((0x24126ea15001e420ull) >> 11) * 0x1.0p-53, "uniforms from the third known answer");
    CHECK(imc::unit_from_words(0xffffffffu, 0xffffffffu) < 1.0 && imc::unit_from_words(0, 0) == 0.0, "uniforms lie in [0, 1)");
}

void check_thresholds()
{
    double cdf[6];
    const double r[6] = {0.0, 2.0, 0.0, 6.0, 0.0, 0.0};
    CHECK(imc::threshold_row(r, 6, cdf) == 0, "a valid row");
    CHECK(cdf[0] == 0.0 && cdf[1] == 0.25 && cdf[2] == 0.25 && cdf[3] == 1.0 && cdf[4] == 1.0 && cdf[5] == 1.0, "running sum over its last value, ones from the last positive entry");
    CHECK(imc::pick(cdf, 6, 0.0) == 1 && imc::pick(cdf, 6, 0.2499999) == 1 && imc::pick(cdf, 6, 0.25) == 3 && imc::pick(cdf, 6, 0x1.fffffffffffffp-1) == 3, "smallest j with u < cdf[j]");
    const double third[3] = {0.1, 0.2, 0.3};            // the last running sum is the total, so the last threshold is 1.0 by construction too
    CHECK(imc::threshold_row(third, 3, cdf) == 0 && cdf[0] == 0.1 / (0.1 + 0.2 + 0.3) && cdf[2] == 1.0, "unnormalised row");
    const double neg[2] = {0.5, -0.1}, zero[2] = {0.0, 0.0};
    const double inf_row[2] = {1.0, std::numeric_limits<double>::infinity()}, nan_row[2] = {std::numeric_limits<double>::quiet_NaN(), 1.0};
    CHECK(imc::threshold_row(neg, 2, cdf) == 1 && imc::threshold_row(inf_row, 2, cdf) == 1 && imc::threshold_row(nan_row, 2, cdf) == 1, "negative and non-finite entries");
    CHECK(imc::threshold_row(zero, 2, cdf) == 2, "a row without mass");
    imc::SampleTables tb;
    std::string err;
    const double pi[2] = {1, 1}, T[4] = {1, 0, 0, 0}, E[4] = {1, 1, 1, 1};
    CHECK(!imc::build_tables(2, 2, 2, pi, T, E, &tb, &err) && err.find("T row 1") != std::string::npos, "the message names the matrix and the row: %s", err.c_str());
    for (int n = 1; n <= 70; ++n) {                      // the bisection against the linear search, thresholds and values between them
        Rng rng(n);
        std::vector<double> row(n), c(n);
        for (double &v : row) v = rng.below(3) ? rng.unit() : 0.0;
        row[rng.below(n)] += 0.5;
        CHECK(imc::threshold_row(row.data(), n, c.data()) == 0, "row");
        for (int k = 0; k < 400; ++k) {
            const double u = k < n ? c[k] * (c[k] < 1.0) : rng.unit();
            int lin = 0;
            while (!(u < c[lin])) ++lin;
            CHECK(imc::pick(c.data(), n, u) == lin && row[lin] > 0.0, "pick n=%d u=%.17g", n, u);
        }
    }
    CHECK(imc::tile_setting(nullptr, 512) == 512 && imc::tile_setting("", 512) == 512 && imc::tile_setting("1", 512) == 1 && imc::tile_setting("65536", 512) == 65536, "tile setting");
    CHECK(imc::tile_setting("0", 512) == 0 && imc::tile_setting("65537", 512) == 0 && imc::tile_setting("12x", 512) == 0 && imc::tile_setting("-3", 512) == 0, "tile setting refusals");
}

void check_combine()
{
    Rng rng(7);
    for (int N : {1, 2, 3, 20, 65, 256})
        for (int rep = 0; rep < 50; ++rep) {
            std::vector<uint8_t> a(N), b(N), c(N), ab(N), bc(N), l(N), r(N), id(N);
            for (int i = 0; i < N; ++i) a[i] = (uint8_t)rng.below(N), b[i] = (uint8_t)rng.below(N), c[i] = (uint8_t)rng.below(N);
            imc::map_combine(a.data(), b.data(), ab.data(), N);
            imc::map_combine(b.data(), c.data(), bc.data(), N);
            imc::map_combine(ab.data(), c.data(), l.data(), N);
            imc::map_combine(a.data(), bc.data(), r.data(), N);
            CHECK(l == r, "combine is not associative at N=%d", N);
            imc::map_identity(id.data(), N);
            imc::map_combine(id.data(), a.data(), l.data(), N);
            imc::map_combine(a.data(), id.data(), r.data(), N);
            CHECK(l == a && r == a, "identity");
            std::vector<uint8_t> in_place = a;
            imc::map_combine(in_place.data(), b.data(), in_place.data(), N);
            CHECK(in_place == ab, "combine into its first argument");
        }
}

}  // namespace

int main()
{
    check_philox();
    check_thresholds();
    check_combine();
    for (int N : {1, 2, 3, 20, 65, 256})
        for (int k = 0; k < kKinds; ++k) {
            run_case<uint8_t>((Kind)k, N, 3, 2, 1, N >= 65 ? 4201 : 4999, 20240917u + k, 0);
            run_case<uint8_t>((Kind)k, N, 5, 5, 3, 1409, 77u + k, 1);
        }
    run_case<uint16_t>(kFast, 20, 300, 300, 3, 1409, 5, 2);       // 16-bit symbols
    run_case<uint8_t>(kFast, 3, 3, 2, 3, 1, 5, 0);                 // one-column replicates: every column is a start
    run_case<uint8_t>(kCyclic, 20, 3, 3, 3, 2, 5, 0);
    std::printf("sample_tiles ok (%ld columns compared)\n", g_compared);
    return 0;
}
