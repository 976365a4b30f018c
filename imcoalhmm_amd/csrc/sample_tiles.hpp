// sample_tiles.hpp - drawing hidden paths and symbols from an HMM (pi, T, E): the specification and its parallel form,
// host-only.  The sequential loop sample_sequential() below IS the definition of the sampler's output; the kernels
// (kernels_sample.hpp) and the CPU check (tests/sample_tiles_check.cpp) call the tile functions and must reproduce it bit
// for bit.
//
// Uniforms.  Counter based, so any column is drawn independently of every other: Philox4x32-10 with key
// (seed & 0xffffffff, seed >> 32) and counter (t & 0xffffffff, t >> 32, replicate, tag), t the column index within the
// replicate.  Of the four output words w0..w3, u_state = ((w1 << 32 | w0) >> 11) * 2^-53 draws the column's state and
// u_sym = ((w3 << 32 | w2) >> 11) * 2^-53 its symbol: both in [0, 1) and exact in fp64.
//
// Threshold tables.  Built once per call on the host in fp64 by build_tables() - the one function both paths use.  For a
// row r[0..n): acc += r[j] from left to right, total = the last acc, cdf[j] = acc_j / total, and every entry from the last
// strictly positive r[j] onward is exactly 1.0.  pick(cdf, n, u) is the smallest j with u < cdf[j]; an entry of
// probability zero is never picked (its threshold equals its left neighbour's), rows need not be normalised.  The table
// is non-decreasing, so the order of the search is free; pick() bisects.
//
// Chain.  x_0 = pick(cdf_pi, u_state(0)), x_t = pick(cdf_T[x_{t-1}], u_state(t)), o_t = pick(cdf_E[x_t], u_sym(t)).
//
// Parallel form.  Column t with its uniform is a map [N] -> [N], i -> pick(cdf_T[i], u_state(t)); column 0 of a replicate
// is the constant map to x_0.  The stream is the R replicates of L columns back to back; a tile of consecutive stream
// columns is summarised as the composition of its maps - N bytes, since N <= 256.  Composition is associative with the
// identity i -> i (map_combine), so every tile's entering state comes from one scan over the summaries, and every tile
// is then walked from its entering state on its own (walk_tile).  A replicate's first column forgets the entering state,
// so replicate boundaries need no handling wherever they fall inside a tile, and the state entering tile 0 is irrelevant.
// N walks per tile is the price of the summary (one per possible entering state); all of them share the tile's uniforms.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define IMC_SMP_HD __host__ __device__
#else
#define IMC_SMP_HD
#endif

namespace imc {

constexpr int kSampleMaxStates = 256;      // a state is a byte
constexpr int kSampleMaxSymbols = 4096;
constexpr int kSampleMaxReplicates = 65536;
constexpr int kSampleMaxTile = 65536;      // IMC_SAMPLE_TILE: 1 .. this

// ---- uniforms ---------------------------------------------------------------------------------------
IMC_SMP_HD inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

IMC_SMP_HD inline double unit_from_words(uint32_t lo, uint32_t hi)
{
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1.0p-53;   // 53 bits: exact
}

// the two uniforms of column t of a replicate
IMC_SMP_HD inline void column_uniforms(uint64_t seed, uint32_t tag, uint32_t replicate, uint64_t t, double *u_state, double *u_sym)
{
    const uint32_t ctr[4] = {(uint32_t)t, (uint32_t)(t >> 32), replicate, tag};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    *u_state = unit_from_words(w[0], w[1]);
    *u_sym = unit_from_words(w[2], w[3]);
}

// ---- threshold tables -------------------------------------------------------------------------------
// cdf[0..n) of the row r[0..n).  0 = fine, 1 = an entry is negative or not finite, 2 = the total is not positive.
inline int threshold_row(const double *r, int n, double *cdf)
{
    double acc = 0.0;
    int last_positive = -1;
    for (int j = 0; j < n; ++j) {
        if (!(r[j] >= 0.0) || !std::isfinite(r[j])) return 1;
        acc += r[j];
        cdf[j] = acc;
        if (r[j] > 0.0) last_positive = j;
    }
    const double total = acc;
    if (!(total > 0.0) || !std::isfinite(total)) return 2;
    for (int j = 0; j < n; ++j) cdf[j] = j >= last_positive ? 1.0 : cdf[j] / total;
    return 0;
}

// The tables of one call, in the layout the kernels read: N rows of cdf_T (N entries each), then cdf_pi as row N, then N
// rows of cdf_E (emit entries each).
struct SampleTables {
    int N = 0, emit = 0;
    std::vector<double> cdf;
    const double *T() const { return cdf.data(); }
    const double *pi() const { return cdf.data() + (size_t)N * N; }
    const double *E() const { return cdf.data() + (size_t)(N + 1) * N; }
    size_t transition_doubles() const { return (size_t)(N + 1) * N; }   // cdf_T and cdf_pi
};

// false with a message that names the matrix and the row
inline bool build_tables(int N, int S, int emit, const double *pi, const double *T, const double *E, SampleTables *out, std::string *err)
{
    out->N = N;
    out->emit = emit;
    out->cdf.assign((size_t)(N + 1) * N + (size_t)N * emit, 0.0);
    auto row = [&](const char *matrix, int r, const double *src, int n, double *dst) {
        const int bad = threshold_row(src, n, dst);
        if (bad) *err = std::string(matrix) + " row " + std::to_string(r) + (bad == 1 ? ": an entry is negative or not finite" : ": the total is not positive");
        return bad == 0;
    };
    double *cdf = out->cdf.data();
    if (!row("pi", 0, pi, N, cdf + (size_t)N * N)) return false;
    for (int i = 0; i < N; ++i)
        if (!row("T", i, T + (size_t)i * N, N, cdf + (size_t)i * N)) return false;
    for (int i = 0; i < N; ++i)
        if (!row("E", i, E + (size_t)i * S, emit, cdf + (size_t)(N + 1) * N + (size_t)i * emit)) return false;
    return true;
}

// smallest j with u < cdf[j]; cdf is non-decreasing and ends in 1.0 > u
IMC_SMP_HD inline int pick(const double *cdf, int n, double u)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ---- the three functions the kernels call -------------------------------------------------------------
// One walk stepped by one column: the state after column t (of its replicate) for a walk in state s before it.
// cdf_T holds the N rows and cdf_pi as row N (SampleTables), so the choice of the row is the only thing t == 0 changes.
IMC_SMP_HD inline int walk_step(int s, bool first_column, double u_state, const double *cdf_T, int N)
{
    return pick(cdf_T + (size_t)(first_column ? N : s) * N, N, u_state);
}

// a summary (map[i] = state after the tile so far, entered in state i) stepped by one column
IMC_SMP_HD inline void summary_step(uint8_t *map, int N, bool first_column, double u_state, const double *cdf_T)
{
    for (int i = 0; i < N; ++i) map[i] = (uint8_t)walk_step(map[i], first_column, u_state, cdf_T, N);
}

IMC_SMP_HD inline void map_identity(uint8_t *map, int N)
{
    for (int i = 0; i < N; ++i) map[i] = (uint8_t)i;
}

// out = a then b (out may be a, not b)
IMC_SMP_HD inline void map_combine(const uint8_t *a, const uint8_t *b, uint8_t *out, int N)
{
    for (int i = 0; i < N; ++i) out[i] = b[a[i]];
}

// Stream columns [g0, g1) of R replicates of L columns, walked from the state `enter`; writes the symbols (sym_bytes 1 or
// 2 per symbol) and, unless states is null, the states, both indexed by stream column.  Returns the state after g1 - 1.
template <class Sym>
IMC_SMP_HD inline int walk_tile(int enter, uint64_t g0, uint64_t g1, uint64_t L, uint64_t seed, uint32_t tag, const double *cdf_T,
                                const double *cdf_E, int N, int emit, Sym *sym, uint8_t *states)
{
    uint32_t r = (uint32_t)(g0 / L);
    uint64_t t = g0 % L;
    int s = enter;
    for (uint64_t g = g0; g < g1; ++g) {
        double us, uy;
        column_uniforms(seed, tag, r, t, &us, &uy);
        s = walk_step(s, t == 0, us, cdf_T, N);
        sym[g] = (Sym)pick(cdf_E + (size_t)s * emit, emit, uy);
        if (states) states[g] = (uint8_t)s;
        if (++t == L) { t = 0; ++r; }
    }
    return s;
}

// the summary of stream columns [g0, g1)
inline void summarise_tile(uint64_t g0, uint64_t g1, uint64_t L, uint64_t seed, uint32_t tag, const double *cdf_T, int N, uint8_t *map)
{
    uint32_t r = (uint32_t)(g0 / L);
    uint64_t t = g0 % L;
    map_identity(map, N);
    for (uint64_t g = g0; g < g1; ++g) {
        double us, uy;
        column_uniforms(seed, tag, r, t, &us, &uy);
        summary_step(map, N, t == 0, us, cdf_T);
        if (++t == L) { t = 0; ++r; }
    }
}

inline uint64_t sample_tile_count(uint64_t columns, uint64_t tile) { return (columns + tile - 1) / tile; }

// ---- the sequential specification ---------------------------------------------------------------------
// R replicates of L columns from the tables; outputs laid out [replicate][column].
template <class Sym>
inline void sample_sequential(const SampleTables &tb, uint64_t seed, uint32_t tag, int R, uint64_t L, Sym *sym, uint8_t *states)
{
    for (int r = 0; r < R; ++r) {
        int s = 0;
        for (uint64_t t = 0; t < L; ++t) {
            double us, uy;
            column_uniforms(seed, tag, (uint32_t)r, t, &us, &uy);
            s = t == 0 ? pick(tb.pi(), tb.N, us) : pick(tb.T() + (size_t)s * tb.N, tb.N, us);
            const size_t g = (size_t)r * L + t;
            sym[g] = (Sym)pick(tb.E() + (size_t)s * tb.emit, tb.emit, uy);
            if (states) states[g] = (uint8_t)s;
        }
    }
}

// IMC_SAMPLE_TILE: the tile length a call uses; `text` null or empty = the default.  0 = not a number in 1 .. kSampleMaxTile.
inline int tile_setting(const char *text, int dflt)
{
    if (!text || !*text) return dflt;
    char *end = nullptr;
    const long v = std::strtol(text, &end, 10);
    if (*end || v < 1 || v > kSampleMaxTile) return 0;
    return (int)v;
}

}  // namespace imc
