// tile_scan.hpp - the scaffold of the tiled device pipelines (kernels_encode.hpp, kernels_train.hpp, kernels_ingest.hpp,
// kernels_align.hpp): a stream is cut into tiles, every tile is summarised as an element of a monoid, ONE workgroup scans
// the summaries, and every tile scatters from its scanned prefix.  The monoids are the pipelines' own (encode_tiles.hpp,
// ingest_tiles.hpp, align_tiles.hpp); here are the tile geometry and the three primitives around them, templated on the
// combine - a callable (earlier, later) -> both, associative, NOT assumed commutative - and its identity.  Plain HIP for
// gfx950.  Not served: k_smp_scan (kernels_sample.hpp), whose element is an N-byte map in dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "slab_stream.hpp"

constexpr int TILE_THREADS = 256;
constexpr int TILE_ITEMS = 16;                           // consecutive elements per thread: one 16-bit flag word
constexpr int TILE_SIZE = TILE_THREADS * TILE_ITEMS;     // 4096 elements per workgroup
constexpr int TILE_SCAN_THREADS = 1024;                  // the one workgroup that scans the tile summaries

// Exclusive scan of one 32-bit value per thread over the workgroup's TILE_THREADS threads, in thread order; `total` gets
// the combination of all of them.  wave_tot: TILE_THREADS / 64 words of LDS.  One barrier, and all threads must call it;
// the caller puts another barrier in front of the next write to wave_tot.
template <class Combine>
__device__ inline uint32_t tile_wg_scan(uint32_t mine, uint32_t ident, Combine combine, uint32_t *wave_tot, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v = combine(u, v);
    }
    if (lane == 63) wave_tot[wave] = v;
    uint32_t before = __shfl_up(v, 1);
    if (lane == 0) before = ident;
    __syncthreads();
    uint32_t prefix = ident, all = ident;
#pragma unroll
    for (int j = 0; j < TILE_THREADS / 64; ++j) {
        const uint32_t t = wave_tot[j];
        if (j < wave) prefix = combine(prefix, t);
        all = combine(all, t);
    }
    total = all;
    return combine(prefix, before);
}

// part[0] = the combination of every thread's `mine`, in thread order, by a tree in LDS (part: THREADS elements).  Ends
// with a barrier; all threads must call it.
template <int THREADS, class T, class Combine>
__device__ inline void tile_wg_reduce(T mine, T *part, Combine combine)
{
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        if ((threadIdx.x & (2 * d - 1)) == 0) part[threadIdx.x] = combine(part[threadIdx.x], part[threadIdx.x + d]);
        __syncthreads();
    }
}

// One workgroup of TILE_SCAN_THREADS threads scans the n elements load(0) .. load(n - 1): emit(i, combination of the
// elements before i) is called once for every i, by the thread that owns i (imc::scan_share), and every thread gets the
// combination of all n back.  Every thread folds its consecutive elements, the folds are scanned in LDS (sc:
// TILE_SCAN_THREADS elements), and the thread walks its elements again from its own prefix.  The last barrier stands in
// front of the walk: a caller that uses sc again puts a barrier behind the call.
template <class T, class Load, class Combine, class Emit>
__device__ inline T tile_scan_elements(uint32_t n, T ident, T *sc, Load load, Combine combine, Emit emit)
{
    const imc::ScanShare own = imc::scan_share(n, TILE_SCAN_THREADS, threadIdx.x);
    T acc = ident;
    for (uint32_t i = own.lo; i < own.hi; ++i) acc = combine(acc, load(i));
    sc[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 1; d < TILE_SCAN_THREADS; d <<= 1) {         // inclusive scan in thread order
        T v = sc[threadIdx.x];
        if ((int)threadIdx.x >= d) v = combine(sc[threadIdx.x - d], v);
        __syncthreads();
        sc[threadIdx.x] = v;
        __syncthreads();
    }
    T run = threadIdx.x ? sc[threadIdx.x - 1] : ident;
    for (uint32_t i = own.lo; i < own.hi; ++i) {
        emit(i, run);
        run = combine(run, load(i));
    }
    return sc[TILE_SCAN_THREADS - 1];
}
