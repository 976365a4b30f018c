// kernels_train.hpp - pair-dictionary training on the device: the counts and choices of imc::train_dict /
// imc::train_dict_wide (pair_dict.hpp) from symbols that are already in HBM.  Plain HIP for gfx950; the rules the
// kernels share with the CPU check are train_tiles.hpp's inline functions, and every replacement pass is the encoder's
// (kernels_encode.hpp: k_enc_summary / k_enc_scan / k_enc_scatter) reading the device dictionary that training grows.
//
// The training stream lives in the encoder's two 16-bit ping-pong scratch streams, WITHOUT chunk marks: a sample is one
// stream, and pairs that straddle the joint of two chunks' heads count as they do on the host.
//   k_trn_load        a range of raw symbols (bytes or 16-bit) or of an encoded stream -> the training stream, mark stripped
//   byte phase, per merge:
//   k_trn_pair_hist   one workgroup per tile: counts of a * A + b over adjacent pairs (LDS bins while A * A fits
//                     kTrnLdsBins, then one global add per non-empty bin; global adds directly beyond)
//   k_trn_argmax      ONE workgroup: the eligible bin with the largest count, smallest key among equals; appends it to
//                     the device dictionary as token A and reports {a, b, count}
//   rounds, per round:
//   k_trn_pair_count  counts per distinct key a << 16 | b in an open-addressing table in global memory
//   k_trn_candidates  (count, key) of the slots at or above the threshold, compacted in arbitrary order (the host ranks
//                     them with pair_dict.hpp's comparator)
// Alignment streams are ~90 % one symbol in runs of thousands of columns, so a thread merges equal consecutive keys of
// its own items before it issues an atomic.  All atomics are integer adds, compare-and-swaps and ors: no result depends on
// the order of arrival.  No workgroup waits for another, every loop is bounded by a launch argument or a constant, and
// indices are 32-bit, as in the encoder.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_encode.hpp"
#include "train_tiles.hpp"

constexpr int TRN_HIST_SUBTILES = 8;                            // encoder tiles per workgroup of k_trn_pair_hist
constexpr int TRN_HIST_TILE = TRN_HIST_SUBTILES * TILE_SIZE;     // 32768 elements: the LDS bins are zeroed and flushed once per workgroup
constexpr int TRN_ARGMAX_THREADS = 1024;

// src[src_first + t] -> dst[t] for t < count, without bit 15 (sym_bytes 1: bytes; 2: 16-bit symbols or stream elements)
__global__ __launch_bounds__(TILE_THREADS) void k_trn_load(const void *src, int sym_bytes, uint32_t src_first, uint32_t count, uint16_t *dst)
{
    const uint32_t t = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (t >= count) return;
    const uint32_t v = sym_bytes == 1 ? (uint32_t) static_cast<const uint8_t *>(src)[(size_t)src_first + t]
                                      : (uint32_t) static_cast<const uint16_t *>(src)[(size_t)src_first + t];
    dst[t] = (uint16_t)(v & (uint32_t)(imc::kChunkMark - 1));
}

// counts[a * A + b] += adjacent pairs (seq[t], seq[t + 1]) = (a, b), t + 1 < n; the pair that straddles a tile edge
// belongs to the tile of its first element.  counts zeroed by the caller.  LDS: A * A <= kTrnLdsBins.
template <bool LDS>
__global__ __launch_bounds__(TILE_THREADS) void k_trn_pair_hist(const uint16_t *seq, uint32_t n, uint32_t A, uint32_t *counts)
{
    __shared__ uint32_t bins[LDS ? imc::kTrnLdsBins : 1];
    const uint32_t nbins = A * A;
    if (LDS) {
        for (uint32_t b = threadIdx.x; b < nbins && b < imc::kTrnLdsBins; b += TILE_THREADS) bins[b] = 0;
        __syncthreads();
    }
    for (int sub = 0; sub < TRN_HIST_SUBTILES; ++sub) {
        const uint32_t base = (blockIdx.x * (uint32_t)TRN_HIST_SUBTILES + sub) * (uint32_t)TILE_SIZE + threadIdx.x * (uint32_t)TILE_ITEMS;
        if (base + 1 >= n) continue;                               // (no pair starts here; uniform exit is not needed: no barrier in the loop)
        uint16_t x[TILE_ITEMS + 1];
        enc_load_items(seq, base, x);
        uint32_t run_key = imc::kNoBin, run_n = 0;
#pragma unroll
        for (int i = 0; i < TILE_ITEMS; ++i) {
            const bool valid = base + i + 1 < n && x[i] < A && x[i + 1] < A;
            const uint32_t k = valid ? imc::pair_bin(x[i], x[i + 1], A) : imc::kNoBin;
            if (k == run_key) {
                ++run_n;
            } else {
                if (run_n && run_key != imc::kNoBin) atomicAdd(LDS ? &bins[run_key] : &counts[run_key], run_n);
                run_key = k;
                run_n = 1;
            }
        }
        if (run_n && run_key != imc::kNoBin) atomicAdd(LDS ? &bins[run_key] : &counts[run_key], run_n);
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nbins && b < imc::kTrnLdsBins; b += TILE_THREADS)
            if (bins[b]) atomicAdd(&counts[b], bins[b]);
    }
}

// One workgroup.  The winner of counts[0 .. A * A) under the depth cap becomes token A of the device dictionary
// (left, right, depth: at least A + 1 entries); out3 = {a, b, count}, count 0 when no pair is eligible.
__global__ __launch_bounds__(TRN_ARGMAX_THREADS) void k_trn_argmax(const uint32_t *counts, uint32_t A, int max_depth, uint16_t *left, uint16_t *right,
                                                                  uint16_t *depth, uint32_t *out3)
{
    __shared__ imc::PairBest sc[TRN_ARGMAX_THREADS];
    const uint32_t nbins = A * A;
    imc::PairBest best = imc::best_identity();
    for (uint32_t bin = threadIdx.x; bin < nbins; bin += TRN_ARGMAX_THREADS) {
        const uint32_t c = counts[bin];
        if (c == 0) continue;
        const uint32_t a = bin / A, b = bin - a * A;
        if (imc::pair_eligible(c, depth[a], depth[b], max_depth)) best = imc::best_combine(best, imc::PairBest{c, bin});
    }
    sc[threadIdx.x] = best;
    __syncthreads();
    for (int d = TRN_ARGMAX_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) sc[threadIdx.x] = imc::best_combine(sc[threadIdx.x], sc[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const imc::PairBest w = sc[0];
        uint32_t a = 0, b = 0;
        if (w.count) {
            a = w.key / A;
            b = w.key - a * A;
            left[A] = (uint16_t)a;
            right[A] = (uint16_t)b;
            const uint16_t da = depth[a], db = depth[b];
            depth[A] = (uint16_t)(1 + (da > db ? da : db));
        }
        out3[0] = a;
        out3[1] = b;
        out3[2] = w.count;
    }
}

// keys / counts: `capacity` slots (a power of two >= 2 n), keys filled with kNoKey and counts zeroed by the caller.
// *overflow is set if a key finds no slot within `capacity` probes (impossible at this load factor; the host checks).
__global__ __launch_bounds__(TILE_THREADS) void k_trn_pair_count(const uint16_t *seq, uint32_t n, uint32_t capacity, uint32_t *keys, uint32_t *counts,
                                                               uint32_t *overflow)
{
    const uint32_t base = blockIdx.x * (uint32_t)TILE_SIZE + threadIdx.x * (uint32_t)TILE_ITEMS;
    if (base + 1 >= n) return;
    uint16_t x[TILE_ITEMS + 1];
    enc_load_items(seq, base, x);
    uint32_t run_key = imc::kNoKey, run_n = 0;
    auto add = [&](uint32_t k, uint32_t c) {
        uint32_t s = imc::count_slot(k, capacity);
        for (uint32_t probe = 0; probe < capacity; ++probe) {
            uint32_t have = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (have == imc::kNoKey) {
                have = atomicCAS(&keys[s], imc::kNoKey, k);
                if (have == imc::kNoKey) have = k;
            }
            if (have == k) {
                atomicAdd(&counts[s], c);
                return;
            }
            s = (s + 1) & (capacity - 1);
        }
        atomicOr(overflow, 1u);
    };
#pragma unroll
    for (int i = 0; i < TILE_ITEMS; ++i) {
        const uint32_t k = base + i + 1 < n ? imc::key_of(x[i], x[i + 1]) : imc::kNoKey;
        if (k == run_key) {
            ++run_n;
        } else {
            if (run_n && run_key != imc::kNoKey) add(run_key, run_n);
            run_key = k;
            run_n = 1;
        }
    }
    if (run_n && run_key != imc::kNoKey) add(run_key, run_n);
}

// list[i] = (count, key) of every slot with count >= threshold, i < *list_n in arbitrary order; entries beyond
// list_capacity are counted but not written (the host checks).  *list_n zeroed by the caller.
__global__ __launch_bounds__(TILE_THREADS) void k_trn_candidates(const uint32_t *keys, const uint32_t *counts, uint32_t capacity, uint32_t threshold,
                                                               uint2 *list, uint32_t list_capacity, uint32_t *list_n)
{
    const uint32_t s = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
    if (s >= capacity) return;
    const uint32_t k = keys[s], c = counts[s];
    if (k == imc::kNoKey || c < threshold) return;
    const uint32_t i = atomicAdd(list_n, 1u);
    if (i < list_capacity) list[i] = make_uint2(c, k);
}
