// kernels_encode.hpp - the pair-dictionary encoder on the device: the token streams imc::encode_levels() (pair_dict.hpp)
// produces on the host, bit for bit, from symbols that are already in HBM.  Plain HIP for gfx950; the parallel form of a
// pass and its proof obligations are in encode_tiles.hpp, whose inline functions the kernels call.
//
// The stream lives in two 16-bit ping-pong scratch buffers; bit 15 marks a chunk's first element (imc::kChunkMark), so
// K concatenated chunks go through one run of passes.  A PASS is three launches, ordered by kernel boundaries only:
//   k_enc_summary   one workgroup per tile of TILE_SIZE elements: the pair flag of every position (16 bits per thread,
//                   kept for the scatter) and the tile's summary (emitted count and outgoing carry per incoming carry)
//   k_enc_scan      ONE workgroup: every tile's incoming carry and output offset, and the new length
//   k_enc_scatter   one workgroup per tile: emits into LDS in order, then writes its part of the output coalesced
// A SNAPSHOT (a level of the dictionary) finds the chunk starts - the marked positions - with the same machinery
// (k_enc_mark_summary, k_enc_scan, k_enc_mark_scatter) and copies every chunk's part into its own level buffer
// (k_enc_snapshot: mark stripped, narrowed to bytes for alphabets up to 256); k_enc_histogram counts the tokens at
// positions >= 1 of every chunk with integer atomics (LDS bins, then one global add per non-empty bin and workgroup),
// so the counts do not depend on the order of arrival.
//   k_enc_load      raw symbols (bytes or 16-bit) -> scratch stream, first element marked
//   k_enc_validate  first column whose symbol is not below nsym (integer atomic min)
//   k_enc_narrow    1-, 2- or 4-byte symbols -> the chunk's own raw buffer (bytes, or 16-bit beyond 256 symbols)
//
// No workgroup ever waits for another one: there are no look-back chains, flags or spins, and every loop has a bound
// that is a launch argument or a constant.  Indices are 32-bit: a run of passes holds fewer than 2^31 elements.
//
// Host side (imcoal_fwd.hip, device_encode): all of this runs on the library's stream with g_mu held; the new length
// is read back once per pass, the chunk starts once per snapshot.
#pragma once
#include <hip/hip_runtime.h>

#include "encode_tiles.hpp"
#include "tile_scan.hpp"

constexpr int ENC_HIST_BINS = 4096;                    // largest alphabet whose tokens are counted (HYBRID_MAX_ALPHABET)
static_assert(TILE_SIZE < (int)imc::kPackedCountLimit, "a tile's counts must fit the packed summary");

struct EncPass {
    const uint16_t *left, *right;   // the dictionary's device copy: token z = left[z] followed by right[z]
    int z0, nz;                     // the pass replaces the pairs of tokens z0 .. z0 + nz - 1 (nz <= 256)
};

// Scratch buffers hold TILE_SIZE * tiles + TILE_ITEMS elements, so the vector loads of a tile's last thread and the
// look-ahead element stay inside the allocation; what lies beyond n is never used (every use checks the index).
__device__ inline void enc_load_items(const uint16_t *seq, uint32_t base, uint16_t (&x)[TILE_ITEMS + 1])
{
    const uint4 *p = reinterpret_cast<const uint4 *>(seq + base);
    const uint4 a = p[0], b = p[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        x[2 * j] = (uint16_t)(w[j] & 0xffffu);
        x[2 * j + 1] = (uint16_t)(w[j] >> 16);
    }
    x[TILE_ITEMS] = seq[base + TILE_ITEMS];
}

// The round's keys into the workgroup's LDS set (hk: kKeySlots words, hv: kKeySlots ids); nothing to do for one pair.
__device__ inline void enc_build_keys(const EncPass &ps, uint32_t *hk, uint16_t *hv)
{
    if (ps.nz <= 1) return;
    for (uint32_t s = threadIdx.x; s < imc::kKeySlots; s += TILE_THREADS) hk[s] = imc::kNoKey;
    __syncthreads();
    for (int q = threadIdx.x; q < ps.nz; q += TILE_THREADS) {
        const int z = ps.z0 + q;
        const uint32_t k = imc::key_of(ps.left[z], ps.right[z]);
        uint32_t s = imc::key_slot(k);
        for (uint32_t probe = 0; probe < imc::kKeySlots; ++probe) {
            if (atomicCAS(&hk[s], imc::kNoKey, k) == imc::kNoKey) { hv[s] = (uint16_t)z; break; }
            s = (s + 1) & (imc::kKeySlots - 1);
        }
    }
    __syncthreads();
}

// token of the pair (a, b) in this pass, or kNoToken
__device__ inline uint16_t enc_pair_token(const EncPass &ps, uint16_t one_a, uint16_t one_b, const uint32_t *hk, const uint16_t *hv,
                                          uint16_t a, uint16_t b)
{
    if (ps.nz <= 1) return (a == one_a && b == one_b) ? (uint16_t)ps.z0 : imc::kNoToken;
    return imc::key_lookup(hk, hv, imc::key_of(a, b));
}

// Exclusive scan of one packed summary per thread over the workgroup's TILE_THREADS threads, in thread order; `total`
// gets the whole tile's summary.  wave_tot: 4 words of LDS.  Two barriers; all threads must call it.
__device__ inline uint32_t enc_wg_scan(uint32_t mine, uint32_t *wave_tot, uint32_t &total)
{
    const uint32_t before = tile_wg_scan(
        mine, imc::tile_pack(imc::tile_identity()),
        [](uint32_t a, uint32_t b) { return imc::tile_pack(imc::tile_combine(imc::tile_unpack(a), imc::tile_unpack(b))); }, wave_tot, total);
    __syncthreads();
    return before;
}

__global__ __launch_bounds__(TILE_THREADS) void k_enc_summary(const uint16_t *seq, uint32_t n, EncPass ps, uint16_t *flags,
                                                            imc::TileSummary *sums)
{
    __shared__ uint32_t hk[imc::kKeySlots];
    __shared__ uint16_t hv[imc::kKeySlots];
    __shared__ uint32_t wave_tot[TILE_THREADS / 64];
    enc_build_keys(ps, hk, hv);
    const uint16_t one_a = ps.left[ps.z0], one_b = ps.right[ps.z0];
    const uint32_t base = blockIdx.x * (uint32_t)TILE_SIZE + threadIdx.x * (uint32_t)TILE_ITEMS;
    uint16_t x[TILE_ITEMS + 1];
    enc_load_items(seq, base, x);
    uint32_t mask = 0;
    imc::TileSummary s = imc::tile_identity();
#pragma unroll
    for (int i = 0; i < TILE_ITEMS; ++i) {
        const uint32_t t = base + i;
        const bool m = t + 1 < n && enc_pair_token(ps, one_a, one_b, hk, hv, x[i], x[i + 1]) != imc::kNoToken;
        mask |= (m ? 1u : 0u) << i;
        if (t < n) s = imc::tile_step(s, m);
    }
    flags[blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x] = (uint16_t)mask;
    uint32_t total;
    (void)enc_wg_scan(imc::tile_pack(s), wave_tot, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = imc::tile_unpack(total);
}

// One workgroup.  tile_in[i] = (output offset, incoming carry) of tile i; *new_n = elements emitted in all.
__global__ __launch_bounds__(TILE_SCAN_THREADS) void k_enc_scan(const imc::TileSummary *sums, uint32_t ntiles, uint2 *tile_in, uint32_t *new_n)
{
    __shared__ imc::TileSummary sc[TILE_SCAN_THREADS];
    const imc::TileSummary all = tile_scan_elements(
        ntiles, imc::tile_identity(), sc, [&](uint32_t i) { return sums[i]; },
        [](const imc::TileSummary &a, const imc::TileSummary &b) { return imc::tile_combine(a, b); },
        [&](uint32_t i, const imc::TileSummary &run) { tile_in[i] = make_uint2(run.cnt[0], run.out[0]); });   // the stream starts with nothing taken before it: case 0
    if (threadIdx.x == TILE_SCAN_THREADS - 1) *new_n = all.cnt[0];
}

__global__ __launch_bounds__(TILE_THREADS) void k_enc_scatter(const uint16_t *seq, uint32_t n, EncPass ps, const uint16_t *flags,
                                                            const uint2 *tile_in, uint16_t *out)
{
    __shared__ uint32_t hk[imc::kKeySlots];
    __shared__ uint16_t hv[imc::kKeySlots];
    __shared__ uint32_t wave_tot[TILE_THREADS / 64];
    __shared__ uint16_t stage[TILE_SIZE];
    enc_build_keys(ps, hk, hv);
    const uint16_t one_a = ps.left[ps.z0], one_b = ps.right[ps.z0];
    const uint32_t base = blockIdx.x * (uint32_t)TILE_SIZE + threadIdx.x * (uint32_t)TILE_ITEMS;
    uint16_t x[TILE_ITEMS + 1];
    enc_load_items(seq, base, x);
    const uint32_t mask = flags[blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x];
    const uint2 in = tile_in[blockIdx.x];
    imc::TileSummary s = imc::tile_identity();
#pragma unroll
    for (int i = 0; i < TILE_ITEMS; ++i)
        if (base + i < n) s = imc::tile_step(s, (mask >> i) & 1u);
    uint32_t total;
    const imc::TileSummary before = imc::tile_unpack(enc_wg_scan(imc::tile_pack(s), wave_tot, total));
    uint32_t carry = in.y ? before.out[1] : before.out[0], w = in.y ? before.cnt[1] : before.cnt[0];
#pragma unroll
    for (int i = 0; i < TILE_ITEMS; ++i) {
        if (base + i < n) {
            const imc::EmitKind kind = imc::emit_step((mask >> i) & 1u, carry);
            if (kind != imc::kEmitNothing) {
                const uint16_t v = kind == imc::kEmitToken ? enc_pair_token(ps, one_a, one_b, hk, hv, x[i], x[i + 1]) : x[i];
                if (w < (uint32_t)TILE_SIZE) stage[w] = v;
                ++w;
            }
        }
    }
    __syncthreads();
    const imc::TileSummary whole = imc::tile_unpack(total);
    const uint32_t count = min(in.y ? whole.cnt[1] : whole.cnt[0], (uint32_t)TILE_SIZE);
    for (uint32_t j = threadIdx.x; j < count; j += TILE_THREADS)
        if (in.x + j < n) out[in.x + j] = stage[j];            // (a pass never lengthens the stream)
}

// ---- chunk starts ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TILE_THREADS) void k_enc_mark_summary(const uint16_t *seq, uint32_t n, imc::TileSummary *sums)
{
    __shared__ uint32_t wave_tot[TILE_THREADS / 64];
    const uint32_t base = blockIdx.x * (uint32_t)TILE_SIZE + threadIdx.x * (uint32_t)TILE_ITEMS;
    uint16_t x[TILE_ITEMS + 1];
    enc_load_items(seq, base, x);
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < TILE_ITEMS; ++i) c += (base + i < n && (x[i] & imc::kChunkMark)) ? 1u : 0u;
    uint32_t total;
    (void)enc_wg_scan(imc::tile_pack(imc::TileSummary{{c, c}, {0u, 1u}}), wave_tot, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = imc::tile_unpack(total);
}

// pos[k] = position of the k-th marked element (k < K), pos[K] = n
__global__ __launch_bounds__(TILE_THREADS) void k_enc_mark_scatter(const uint16_t *seq, uint32_t n, const uint2 *tile_in, uint32_t *pos, uint32_t K)
{
    __shared__ uint32_t wave_tot[TILE_THREADS / 64];
    const uint32_t base = blockIdx.x * (uint32_t)TILE_SIZE + threadIdx.x * (uint32_t)TILE_ITEMS;
    uint16_t x[TILE_ITEMS + 1];
    enc_load_items(seq, base, x);
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < TILE_ITEMS; ++i) c += (base + i < n && (x[i] & imc::kChunkMark)) ? 1u : 0u;
    uint32_t total;
    const imc::TileSummary before = imc::tile_unpack(enc_wg_scan(imc::tile_pack(imc::TileSummary{{c, c}, {0u, 1u}}), wave_tot, total));
    uint32_t k = tile_in[blockIdx.x].x + before.cnt[0];
#pragma unroll
    for (int i = 0; i < TILE_ITEMS; ++i)
        if (base + i < n && (x[i] & imc::kChunkMark)) {
            if (k < K) pos[k] = base + i;
            ++k;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) pos[K] = n;
}

// Element t of the stream belongs to the chunk k with pos[k] <= t < pos[k + 1]; it goes to dst[k][t - pos[k]] without
// its mark, as a byte (narrow) or as a 16-bit id.  The level buffers were sized from the same pos[].
__global__ __launch_bounds__(TILE_THREADS) void k_enc_snapshot(const uint16_t *seq, uint32_t n, const uint32_t *pos, uint32_t K,
                                                             uint8_t *const *dst, int narrow)
{
    const uint32_t t = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (t >= n) return;
    uint32_t lo = 0, hi = K;                                   // invariant: pos[lo] <= t < pos[hi]
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pos[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t j = t - pos[lo];
    if (j >= pos[lo + 1] - pos[lo]) return;
    const uint16_t v = seq[t] & (uint16_t)~imc::kChunkMark;
    if (narrow) dst[lo][j] = (uint8_t)v;
    else reinterpret_cast<uint16_t *>(dst[lo])[j] = v;
}

// counts[k][z] += occurrences of token z at positions >= 1 of chunk k (blockIdx.y = k); counts zeroed by the caller.
__global__ __launch_bounds__(TILE_THREADS) void k_enc_histogram(const uint16_t *seq, const uint32_t *pos, int alphabet, uint32_t *counts)
{
    __shared__ uint32_t bins[ENC_HIST_BINS];
    for (int b = threadIdx.x; b < alphabet; b += TILE_THREADS) bins[b] = 0;
    __syncthreads();
    const uint32_t k = blockIdx.y, lo = pos[k] + 1, hi = pos[k + 1];
    const uint32_t stride = gridDim.x * (uint32_t)TILE_THREADS;
    for (uint64_t t = (uint64_t)lo + blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x; t < hi; t += stride) {
        const uint32_t z = seq[t] & (uint32_t)(imc::kChunkMark - 1);
        if (z < (uint32_t)alphabet) atomicAdd(&bins[z], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < alphabet; b += TILE_THREADS)
        if (bins[b]) atomicAdd(&counts[(size_t)k * alphabet + b], bins[b]);
}

// ---- raw symbols --------------------------------------------------------------------------------------
__device__ inline uint32_t enc_symbol(const void *src, int sym_bytes, size_t t)
{
    return sym_bytes == 1 ? (uint32_t) static_cast<const uint8_t *>(src)[t]
         : sym_bytes == 2 ? (uint32_t) static_cast<const uint16_t *>(src)[t]
                          : static_cast<const uint32_t *>(src)[t];          // (a negative int32 is a huge unsigned value)
}

__global__ __launch_bounds__(TILE_THREADS) void k_enc_load(const void *src, int sym_bytes, uint32_t L, uint16_t *dst)
{
    const uint32_t t = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (t < L) dst[t] = (uint16_t)(enc_symbol(src, sym_bytes, t) | (t == 0 ? (uint32_t)imc::kChunkMark : 0u));
}

__global__ __launch_bounds__(TILE_THREADS) void k_enc_validate(const void *src, int sym_bytes, uint32_t L, uint32_t nsym, uint32_t *first_bad)
{
    const uint32_t t = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (t < L && enc_symbol(src, sym_bytes, t) >= nsym) atomicMin(first_bad, t);
}

__global__ __launch_bounds__(TILE_THREADS) void k_enc_narrow(const void *src, int sym_bytes, uint32_t L, uint8_t *dst, int dst_wide)
{
    const uint32_t t = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (t >= L) return;
    const uint32_t v = enc_symbol(src, sym_bytes, t);
    if (dst_wide) reinterpret_cast<uint16_t *>(dst)[t] = (uint16_t)v;
    else dst[t] = (uint8_t)v;
}
