// kernels_sample.hpp - the HMM sampler on the device: the states and symbols imc::sample_sequential() (sample_tiles.hpp)
// produces on the host, bit for bit, written straight into device memory.  Plain HIP for gfx950; the map formulation is in
// sample_tiles.hpp, whose inline functions (column_uniforms, walk_step, pick) the kernels call.
//
// The stream is the R replicates of L columns back to back, cut into tiles of `tile` columns.  A call is three launches,
// ordered by kernel boundaries only:
//   k_smp_summary   one walk per (tile, entering state): the tile's map, N bytes.  Entering states are lanes.  Up to 64
//                   states a wavefront holds floor(64 / N) tiles side by side (three at 20 states: 60 of 64 lanes walk);
//                   beyond 64 states a tile takes ceil(N / 64) wavefronts.  All walks of a tile need the same uniforms:
//                   the lanes of a tile draw one column each (Philox once per column and tile, not once per walk) and
//                   the walks read them lane to lane, a batch of G = min(N, 64) columns at a time.
//   k_smp_scan      ONE workgroup: every thread composes the maps of a contiguous run of tiles in LDS, the per-thread maps
//                   are scanned there (Kogge-Stone on maps, two buffers), and every thread walks its run again from its
//                   entering state to write the tiles' entering states.  More tiles than threads x SMP_SCAN_RUN: it loops,
//                   handing one state from pass to pass.
//   k_smp_emit      one walk per tile from its entering state, one lane per tile.  A lane's 64 columns go to a padded LDS
//                   row; the wavefront then writes the 64 rows out with 16-byte stores, four (eight for 16-bit symbols)
//                   consecutive lanes per row, so a store instruction covers whole 64- or 128-byte pieces of the output.
//                   Rows that are short or whose destination is not 16-byte aligned go out element by element, lane = column.
//
// Tables: cdf_T with cdf_pi as row N - (N + 1) N doubles - is what every step of every walk reads.  The summary keeps it in
// LDS while it fits the workgroup's budget (it has no other LDS use: up to 142 states) and reads global memory, i.e. L2,
// beyond; emit needs 34 to 50 KiB of staging for its four wavefronts and keeps the tables, cdf_E included, in LDS only while
// they are small (SMP_EMIT_TABLE_LDS), since its rows are chosen by the state and differ from lane to lane anyway.
//
// No workgroup waits for another one; every loop has a bound that is a launch argument.  Stream columns are 64-bit, tile
// indices 32-bit (the host refuses 2^31 tiles or more).
#pragma once
#include <hip/hip_runtime.h>

#include "sample_tiles.hpp"

constexpr int SMP_THREADS = 256;
constexpr int SMP_SUMMARY_WIDE_THREADS = 1024;        // summary workgroups whose table takes most of a CU's LDS: 16 wavefronts share it
constexpr size_t SMP_SUMMARY_WIDE_FROM = 40 * 1024;   // ... from this table size on
constexpr size_t SMP_EMIT_TABLE_LDS = 12 * 1024;      // emit: tables up to this size beside the staging rows (both within 64 KiB)
constexpr int SMP_SCAN_RUN = 64;                      // tiles per thread and pass of the scan
constexpr int SMP_SCAN_LDS = 64 * 1024;               // the scan's two map buffers
constexpr int SMP_ROW_PAD = 4;                        // bytes after a staging row: lanes writing column k of their rows hit 64 banks

struct SmpArgs {
    const double *tab;       // cdf_T rows, cdf_pi, cdf_E rows (imc::SampleTables)
    int N, emit;
    uint64_t seed;
    uint32_t tag;
    uint64_t L, total;       // columns per replicate, columns of the stream
    uint32_t tile, ntiles;
};

inline int smp_scan_threads(int N) { return std::min(1024, std::max(64, SMP_SCAN_LDS / 2 / N / 64 * 64)); }
inline size_t smp_emit_stage_bytes(int sym_bytes) { return (size_t)(SMP_THREADS / 64) * 64 * ((64 * sym_bytes + SMP_ROW_PAD) + (64 + SMP_ROW_PAD)); }

__device__ inline void smp_advance(uint64_t &t, uint32_t &r, uint64_t by, uint64_t L)
{
    t += by;
    if (t >= L) {
        const uint64_t q = t / L;
        r += (uint32_t)q;
        t -= q * L;
    }
}

template <bool TLDS>
__global__ __launch_bounds__(SMP_SUMMARY_WIDE_THREADS) void k_smp_summary(SmpArgs a, uint8_t *__restrict__ summ)
{
    extern __shared__ __attribute__((aligned(16))) char smp_lds[];
    const double *cdfT = a.tab;
    if (TLDS) {
        double *l = reinterpret_cast<double *>(smp_lds);
        const int n = (a.N + 1) * a.N;
        for (int i = threadIdx.x; i < n; i += blockDim.x) l[i] = a.tab[i];
        __syncthreads();
        cdfT = l;
    }
    const int lane = threadIdx.x & 63, N = a.N;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    // this lane's walk (tile, entering state), the lane group that shares the tile's uniforms and the lane's place in it
    int G, base, jg, state;
    uint64_t tile;
    bool placed = true;
    if (N <= 64) {
        const int per_wave = 64 / N, grp = lane / N;
        G = N;
        state = jg = lane - grp * N;
        placed = grp < per_wave;
        base = placed ? grp * N : 0;
        tile = wave * per_wave + grp;
    } else {
        const int parts = (N + 63) >> 6;
        G = 64;
        tile = wave / parts;
        state = (int)(wave % parts) * 64 + lane;
        jg = lane;
        base = 0;
    }
    const bool tile_ok = placed && tile < a.ntiles;
    const bool walk_ok = tile_ok && state < N;
    const uint64_t g0 = tile_ok ? tile * a.tile : 0;
    const uint32_t len = tile_ok ? (uint32_t)std::min<uint64_t>(a.tile, a.total - g0) : 0u;
    uint32_t r_gen = (uint32_t)(g0 / a.L);
    uint64_t t_walk = g0 - (uint64_t)r_gen * a.L, t_gen = t_walk;
    smp_advance(t_gen, r_gen, (uint64_t)jg, a.L);      // the column this lane draws in the first batch
    int s = state;
    for (uint32_t b0 = 0; b0 < a.tile; b0 += (uint32_t)G) {
        double u = 0.0, unused;
        if (b0 + (uint32_t)jg < len) imc::column_uniforms(a.seed, a.tag, r_gen, t_gen, &u, &unused);
        smp_advance(t_gen, r_gen, (uint64_t)G, a.L);
        const uint32_t steps = std::min<uint32_t>((uint32_t)G, a.tile - b0);
        for (uint32_t j = 0; j < steps; ++j) {
            const double uj = __shfl(u, base + (int)j, 64);
            if (walk_ok && b0 + j < len) {
                s = imc::walk_step(s, t_walk == 0, uj, cdfT, N);
                if (++t_walk == a.L) t_walk = 0;
            }
        }
    }
    if (walk_ok) summ[tile * (uint64_t)N + state] = (uint8_t)s;
}

// enter[j] = the state in which tile j is entered (tile 0: state 0, which its first column forgets)
// (not tile_scan.hpp's scan: the element is an N-byte map in dynamic LDS, ping-pong buffers, several passes per run)
__global__ __launch_bounds__(1024) void k_smp_scan(const uint8_t *__restrict__ summ, uint32_t ntiles, int N, uint8_t *__restrict__ enter)
{
    extern __shared__ __attribute__((aligned(16))) char smp_lds[];
    const uint32_t k = threadIdx.x, threads = blockDim.x;
    uint8_t *src = reinterpret_cast<uint8_t *>(smp_lds), *dst = src + (size_t)threads * N;
    int carry = 0;
    for (uint32_t done = 0; done < ntiles;) {
        const uint32_t rem = ntiles - done;
        const uint32_t run = std::min<uint32_t>((uint32_t)SMP_SCAN_RUN, (rem + threads - 1) / threads);
        const uint64_t first = std::min<uint64_t>((uint64_t)done + (uint64_t)k * run, ntiles), last = std::min<uint64_t>(first + run, ntiles);
        uint8_t *mine = src + (size_t)k * N;
        imc::map_identity(mine, N);
        for (uint64_t j = first; j < last; ++j) imc::map_combine(mine, summ + j * N, mine, N);
        __syncthreads();
        for (uint32_t d = 1; d < threads; d <<= 1) {      // inclusive scan: thread k ends with the map of runs 0 .. k
            uint8_t *out = dst + (size_t)k * N;
            const uint8_t *own = src + (size_t)k * N;
            if (k >= d) imc::map_combine(src + (size_t)(k - d) * N, own, out, N);
            else for (int i = 0; i < N; ++i) out[i] = own[i];
            __syncthreads();
            uint8_t *sw = src; src = dst; dst = sw;
        }
        int s = k ? src[(size_t)(k - 1) * N + carry] : carry;
        const int next_carry = src[(size_t)(threads - 1) * N + carry];
        __syncthreads();                                   // the maps are read: the next pass may overwrite them
        for (uint64_t j = first; j < last; ++j) {
            enter[j] = (uint8_t)s;
            s = summ[j * N + s];
        }
        carry = next_carry;
        done += (uint32_t)std::min<uint64_t>((uint64_t)threads * run, rem);
    }
}

// The wavefront's 64 staged rows (row q: my_len elements of EB bytes for the output at element my_off, as lane q knows
// them) written out: 16-byte stores where a row is full and its destination aligned, element by element otherwise.
template <int EB>
__device__ inline void smp_flush_rows(const char *stage, int stride, char *out, uint64_t my_off, int my_len, int lane)
{
    constexpr int VPR = 64 * EB / 16;      // 16-byte pieces of a row
    const int my_vec = (my_len == 64 && ((reinterpret_cast<uintptr_t>(out) + my_off * EB) & 15) == 0) ? 1 : 0;
    const uint32_t off_lo = (uint32_t)my_off, off_hi = (uint32_t)(my_off >> 32);
#pragma unroll
    for (int it = 0; it < VPR; ++it) {
        const int idx = it * 64 + lane, q = idx / VPR, piece = idx % VPR;
        const uint64_t off_q = ((uint64_t)__shfl(off_hi, q, 64) << 32) | __shfl(off_lo, q, 64);
        if (__shfl(my_vec, q, 64)) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(stage + q * stride) + piece * 4;
            *reinterpret_cast<uint4 *>(out + off_q * EB + piece * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    unsigned long long rest = __ballot(!my_vec && my_len > 0);
    while (rest) {
        const int q = __builtin_ctzll(rest);
        rest &= rest - 1;
        const uint64_t off_q = ((uint64_t)__shfl(off_hi, q, 64) << 32) | __shfl(off_lo, q, 64);
        const int len_q = __shfl(my_len, q, 64);
        if (lane < len_q) {
            if (EB == 1) out[off_q + lane] = stage[q * stride + lane];
            else *reinterpret_cast<uint16_t *>(out + (off_q + lane) * 2) = *reinterpret_cast<const uint16_t *>(stage + q * stride + lane * 2);
        }
    }
}

template <bool TLDS, class Sym>
__global__ __launch_bounds__(SMP_THREADS) void k_smp_emit(SmpArgs a, const uint8_t *__restrict__ enter, Sym *__restrict__ sym, uint8_t *__restrict__ states)
{
    extern __shared__ __attribute__((aligned(16))) char smp_lds[];
    constexpr int SYM_STRIDE = 64 * (int)sizeof(Sym) + SMP_ROW_PAD, ST_STRIDE = 64 + SMP_ROW_PAD;
    const int N = a.N, emit = a.emit;
    const double *cdfT = a.tab, *cdfE = a.tab + (size_t)(N + 1) * N;
    size_t table_bytes = 0;
    if (TLDS) {
        double *l = reinterpret_cast<double *>(smp_lds);
        const int n = (N + 1) * N + N * emit;
        for (int i = threadIdx.x; i < n; i += SMP_THREADS) l[i] = a.tab[i];
        cdfT = l;
        cdfE = l + (size_t)(N + 1) * N;
        table_bytes = ((size_t)n * sizeof(double) + 15) & ~(size_t)15;
    }
    const int lane = threadIdx.x & 63;
    char *stage_sym = smp_lds + table_bytes + (size_t)(threadIdx.x >> 6) * 64 * (SYM_STRIDE + ST_STRIDE);
    char *stage_st = stage_sym + 64 * SYM_STRIDE;
    const uint64_t tile = (uint64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    const bool ok = tile < a.ntiles;
    const uint64_t g0 = ok ? tile * a.tile : 0;
    const int len = ok ? (int)std::min<uint64_t>(a.tile, a.total - g0) : 0;
    uint32_t r = (uint32_t)(g0 / a.L);
    uint64_t t = g0 - (uint64_t)r * a.L;
    int s = ok ? enter[tile] : 0;
    __syncthreads();
    for (int c0 = 0; c0 < (int)a.tile; c0 += 64) {
        const int here = std::max(0, std::min(64, len - c0));
        for (int k = 0; k < here; ++k) {
            double us, uy;
            imc::column_uniforms(a.seed, a.tag, r, t, &us, &uy);
            s = imc::walk_step(s, t == 0, us, cdfT, N);
            const int o = imc::pick(cdfE + (size_t)s * emit, emit, uy);
            *reinterpret_cast<Sym *>(stage_sym + lane * SYM_STRIDE + k * (int)sizeof(Sym)) = (Sym)o;
            stage_st[lane * ST_STRIDE + k] = (char)s;
            if (++t == a.L) { t = 0; ++r; }
        }
        __syncthreads();
        smp_flush_rows<(int)sizeof(Sym)>(stage_sym, SYM_STRIDE, reinterpret_cast<char *>(sym), g0 + (uint64_t)c0, here, lane);
        if (states) smp_flush_rows<1>(stage_st, ST_STRIDE, reinterpret_cast<char *>(states), g0 + (uint64_t)c0, here, lane);
        __syncthreads();
    }
}
