// kernels_ingest.hpp - observation ingestion on the device: the symbols read_observation_file / encode_pairwise
// (obs_io.hpp) produce on the host, from the bytes of the file or of the two sequences.  Plain HIP for gfx950; the rules -
// byte classes, token start and value, the summary of a range of bytes and how summaries combine, the 2-bit unpack, the
// pairwise rule - are the inline functions of ingest_tiles.hpp, which the CPU check drives against the host loops.
//
// TEXT.  A slab of the file (cut after a whitespace byte, so no token crosses its end and the byte before it is no
// digit) is parsed by three launches, ordered by kernel boundaries only:
//   k_ing_text_summary   one workgroup per tile of TILE_SIZE bytes: the token starts of every thread's 16 bytes (one flag
//                        word, kept for the scatter) and the tile's summary: token count, first bad byte, first token
//                        that is not below nsym - with the byte at which the host loop detects it, its value and its
//                        column within the tile -, and whether a digit run longer than 16 starts here (declined)
//   k_ing_scan           ONE workgroup: every tile's output offset and the slab's summary
//   k_ing_text_scatter   one workgroup per tile: every token start reads its digits (they may reach into the next tile,
//                        never beyond the slab) and the values go out in order, as bytes or as 16-bit symbols
// A tile is staged in LDS with the byte before it and ING_HALO bytes behind it; every use of a byte checks its offset
// against the slab's length, so what the buffer holds beyond it is never looked at.  The slab buffer is allocated to
// whole tiles plus the halo, so the 16-byte loads stay inside it.
//   k_ing_unpack2        2-bit cache payload -> symbols (bytes or 16-bit), four columns per thread
//   k_ing_pairwise       two byte sequences -> the symbols 0 / 1 / 2 of the pairwise rule, four columns per thread
// Both write whole words: the columns of the last word beyond the end are written as zeros (the padding of a chunk's
// symbol buffer is zero and stays so).
//
// No workgroup waits for another one, every loop bound is a constant or a launch argument, and indices are 32-bit: a
// slab holds fewer than 2^31 bytes and the host passes output pointers that already point at the slab's first column.
#pragma once
#include <hip/hip_runtime.h>

#include "ingest_tiles.hpp"
#include "tile_scan.hpp"

constexpr int ING_HALO = 16;                           // bytes behind a tile that a token starting in it may read
constexpr int ING_FRONT = 16;                          // LDS bytes in front of the tile (the last one: the byte before it)
constexpr int ING_TILE_TOKENS = TILE_SIZE / 2;          // a token start needs a non-digit before it
static_assert(ING_HALO >= (int)imc::kMaxTokenDigits, "the 17 bytes a token read looks at must be staged");

// bytes a slab buffer must have for a slab of n bytes
constexpr size_t ing_slab_alloc(size_t n) { return (n + TILE_SIZE - 1) / TILE_SIZE * TILE_SIZE + ING_HALO; }

// The tile's bytes into LDS: sb[ING_FRONT + i] = slab[tile_base + i] for -1 <= i < TILE_SIZE + ING_HALO (16-byte loads;
// the slab buffer is 16-byte aligned).  Ends with a barrier.
__device__ inline void ing_stage_tile(const uint8_t *slab, uint32_t tile_base, uint8_t *sb)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(slab + tile_base);
    uint4 *dst = reinterpret_cast<uint4 *>(sb + ING_FRONT);
    dst[threadIdx.x] = src[threadIdx.x];
    if (threadIdx.x == 0) dst[TILE_THREADS] = src[TILE_THREADS];
    if (threadIdx.x == 64) sb[ING_FRONT - 1] = tile_base ? slab[tile_base - 1] : (uint8_t)' ';
    __syncthreads();
}

__global__ __launch_bounds__(TILE_THREADS) void k_ing_text_summary(const uint8_t *slab, uint32_t n, uint32_t nsym, uint16_t *flags,
                                                                 imc::IngestSummary *sums)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ING_FRONT + TILE_SIZE + ING_HALO];
    __shared__ imc::IngestSummary part[TILE_THREADS];
    const uint32_t tile_base = blockIdx.x * (uint32_t)TILE_SIZE;
    ing_stage_tile(slab, tile_base, sb);
    const uint32_t local = threadIdx.x * (uint32_t)TILE_ITEMS;
    imc::IngestSummary s = imc::ingest_identity();
    uint32_t mask = 0;
    for (int i = 0; i < TILE_ITEMS; ++i) {
        const uint32_t at = tile_base + local + i;
        if (at < n) {
            const uint8_t *p = sb + ING_FRONT + local + i;
            const imc::IngestSummary one = imc::ingest_position(p, p[-1], at, n, nsym);
            mask |= one.count << i;
            s = imc::ingest_combine(s, one);
        }
    }
    flags[blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x] = (uint16_t)mask;
    tile_wg_reduce<TILE_THREADS>(s, part, [](const imc::IngestSummary &a, const imc::IngestSummary &b) { return imc::ingest_combine(a, b); });
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

// One workgroup.  tile_off[i] = tokens of the slab before tile i; *total = the slab's summary.
__global__ __launch_bounds__(TILE_SCAN_THREADS) void k_ing_scan(const imc::IngestSummary *sums, uint32_t ntiles, uint32_t *tile_off,
                                                               imc::IngestSummary *total)
{
    __shared__ imc::IngestSummary sc[TILE_SCAN_THREADS];
    const imc::IngestSummary all = tile_scan_elements(
        ntiles, imc::ingest_identity(), sc, [&](uint32_t i) { return sums[i]; },
        [](const imc::IngestSummary &a, const imc::IngestSummary &b) { return imc::ingest_combine(a, b); },
        [&](uint32_t i, const imc::IngestSummary &run) { tile_off[i] = run.count; });   // (of the walk's running summary only count is used)
    if (threadIdx.x == TILE_SCAN_THREADS - 1) *total = all;
}

// out points at the slab's first column and has room for out_room symbols (bytes, or 16-bit values when wide).
__global__ __launch_bounds__(TILE_THREADS) void k_ing_text_scatter(const uint8_t *slab, uint32_t n, const uint16_t *flags, const uint32_t *tile_off,
                                                                 uint8_t *out, uint32_t out_room, int wide)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ING_FRONT + TILE_SIZE + ING_HALO];
    __shared__ uint16_t stage[ING_TILE_TOKENS];
    __shared__ uint32_t wave_tot[TILE_THREADS / 64];
    const uint32_t tile_base = blockIdx.x * (uint32_t)TILE_SIZE;
    ing_stage_tile(slab, tile_base, sb);
    const uint32_t local = threadIdx.x * (uint32_t)TILE_ITEMS;
    const uint32_t mask = flags[blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x];
    uint32_t count;                                             // exclusive scan of the threads' token counts
    uint32_t w = tile_wg_scan((uint32_t)__popc(mask), 0u, [](uint32_t a, uint32_t b) { return a + b; }, wave_tot, count);
    for (int i = 0; i < TILE_ITEMS; ++i)
        if ((mask >> i) & 1u) {
            const uint32_t at = tile_base + local + i;
            const imc::TokenRead t = imc::token_read(sb + ING_FRONT + local + i, at < n ? n - at : 0u);
            if (w < (uint32_t)ING_TILE_TOKENS) stage[w] = (uint16_t)t.value;
            ++w;
        }
    __syncthreads();
    count = min(count, (uint32_t)ING_TILE_TOKENS);
    const uint32_t first = tile_off[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < count; j += TILE_THREADS) {
        const uint32_t col = first + j;
        if (col < out_room) {
            if (wide) reinterpret_cast<uint16_t *>(out)[col] = stage[j];
            else out[col] = (uint8_t)stage[j];
        }
    }
}

// Columns 4 i .. 4 i + 3 of a 2-bit payload of L columns (pk: the slab's packed bytes, dst: the slab's first column, both
// word aligned).  One word (bytes) or two (16-bit symbols) per thread; columns beyond L are written as zeros.
__global__ __launch_bounds__(TILE_THREADS) void k_ing_unpack2(const uint8_t *pk, uint32_t L, uint8_t *dst, int wide)
{
    const uint32_t i = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (4 * (uint64_t)i >= L) return;
    uint32_t s[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) s[k] = 4 * i + k < L ? imc::unpack2(pk, 4 * i + k) : 0u;
    if (wide) reinterpret_cast<uint2 *>(dst)[i] = make_uint2(s[0] | s[1] << 16, s[2] | s[3] << 16);
    else reinterpret_cast<uint32_t *>(dst)[i] = s[0] | s[1] << 8 | s[2] << 16 | s[3] << 24;
}

// Columns 4 i .. 4 i + 3 of the pairwise rule on a[0..L) and b[0..L) (a, b and dst word aligned); columns beyond L are
// written as zeros.
__global__ __launch_bounds__(TILE_THREADS) void k_ing_pairwise(const uint8_t *a, const uint8_t *b, uint32_t L, uint8_t *dst)
{
    const uint32_t i = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (4 * (uint64_t)i >= L) return;
    const uint32_t wa = reinterpret_cast<const uint32_t *>(a)[i], wb = reinterpret_cast<const uint32_t *>(b)[i];
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (4 * i + k < L) word |= imc::pairwise_symbol((uint8_t)(wa >> 8 * k), (uint8_t)(wb >> 8 * k)) << 8 * k;
    reinterpret_cast<uint32_t *>(dst)[i] = word;
}
