// kernels_align.hpp - FASTA alignments on the device: the sequences imc::read_fasta (fasta_io.hpp) produces on the host,
// from the bytes of the file, and the symbols of a pair's or a triplet's chunk from sequences that stay resident.  Plain
// HIP for gfx950; the rules - what a byte is in which state, the summary of a range of bytes and how summaries combine,
// the column rules - are the inline functions of align_tiles.hpp, which the CPU check drives against the host reader.
//
// PARSE.  A slab of the file (never cut inside a header line) is parsed by three launches, ordered by kernel boundaries
// only:
//   k_aln_summary   one workgroup per tile of ALN_TILE bytes: the tile's summary as a function of the state it is entered in
//   k_aln_scan      ONE workgroup: from the state the slab is entered in, every tile's entry state and the kept bytes and
//                   headers in front of it, and the slab's total (state behind it, kept bytes, headers, decline)
//   k_aln_scatter   one workgroup per tile: the kept bytes are compacted in LDS and go out behind those of all tiles and
//                   slabs before them, as aligned words where a word is the tile's alone; every header writes where its
//                   '>' stands in the slab and how many kept bytes lie in front of it
// A tile is staged in LDS with the byte before it; every use of a byte checks its offset against the slab's length.  The
// slab buffer is allocated to whole tiles plus 16 bytes (ing_slab_alloc), so the 16-byte loads stay inside it.
//
// COLUMNS.  k_aln_columns<K> reads K sequences at arbitrary byte offsets of the resident buffer - records are packed back
// to back, so their starts are not word aligned - as aligned words, shifts them into place and writes sixteen columns per
// thread as one 16-byte store; columns of the last store beyond L are written as zeros (the padding of a chunk's symbol
// buffer is zero and stays so).  A word is loaded only if its first byte lies in front of the sequence's end, so no load
// leaves the buffer, whose size is a multiple of 16.
//
// No workgroup waits for another one, every loop bound is a constant or a launch argument; offsets within a slab and
// column indices are 32-bit, offsets into the resident buffer 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include "align_tiles.hpp"
#include "kernels_ingest.hpp"

constexpr int ALN_THREADS = 256;
constexpr int ALN_ITEMS = 16;                          // consecutive bytes per thread
constexpr int ALN_TILE = ALN_THREADS * ALN_ITEMS;      // 4096 bytes per workgroup
constexpr int ALN_FRONT = 16;                          // LDS bytes in front of the tile (the last one: the byte before it)
constexpr int ALN_SCAN_THREADS = 1024;
constexpr int ALN_COLUMNS = (int)imc::kAlnColumns;     // columns per thread of k_aln_columns
static_assert(ALN_TILE == ING_TILE, "slab buffers are allocated by ing_slab_alloc");

struct AlnTileIn {
    uint32_t state, seq, hdr, pad;                     // the tile's entry state; kept bytes and headers of the slab in front of it
};

// The tile's bytes into LDS: sb[ALN_FRONT + i] = slab[tile_base + i] for -1 <= i < ALN_TILE (16-byte loads; the slab
// buffer is 16-byte aligned); prev0: the byte before the slab.  Ends with a barrier.
__device__ inline void aln_stage_tile(const uint8_t *slab, uint32_t tile_base, uint8_t prev0, uint8_t *sb)
{
    reinterpret_cast<uint4 *>(sb + ALN_FRONT)[threadIdx.x] = reinterpret_cast<const uint4 *>(slab + tile_base)[threadIdx.x];
    if (threadIdx.x == 64) sb[ALN_FRONT - 1] = tile_base ? slab[tile_base - 1] : prev0;
    __syncthreads();
}

// the summary of this thread's bytes of the staged tile
__device__ inline imc::AlnSummary aln_thread_summary(const uint8_t *sb, uint32_t tile_base, uint32_t n)
{
    const uint32_t local = threadIdx.x * (uint32_t)ALN_ITEMS, at = tile_base + local;
    const uint32_t count = at < n ? min(n - at, (uint32_t)ALN_ITEMS) : 0u;
    const uint8_t *p = sb + ALN_FRONT + local;
    return imc::aln_range(p, p[-1], count);
}

__global__ __launch_bounds__(ALN_THREADS) void k_aln_summary(const uint8_t *slab, uint32_t n, uint32_t prev0, imc::AlnSummary *sums)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ALN_FRONT + ALN_TILE];
    __shared__ imc::AlnSummary part[ALN_THREADS];
    const uint32_t tile_base = blockIdx.x * (uint32_t)ALN_TILE;
    aln_stage_tile(slab, tile_base, (uint8_t)prev0, sb);
    part[threadIdx.x] = aln_thread_summary(sb, tile_base, n);
    __syncthreads();
    for (int d = 1; d < ALN_THREADS; d <<= 1) {                // in thread order: the combine is not commutative
        if ((threadIdx.x & (2 * d - 1)) == 0) part[threadIdx.x] = imc::aln_combine(part[threadIdx.x], part[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

// One workgroup.  Every thread folds the maps of ceil(ntiles / ALN_SCAN_THREADS) consecutive tiles, the folds are scanned
// in LDS, which gives the thread the state its first tile is entered in; it then walks its tiles in that state for their
// counts, the counts are scanned, and a second walk writes every tile's entry.
__global__ __launch_bounds__(ALN_SCAN_THREADS) void k_aln_scan(const imc::AlnSummary *sums, uint32_t ntiles, uint32_t entry, AlnTileIn *tile_in,
                                                              imc::AlnTotal *total)
{
    __shared__ uint32_t sm[ALN_SCAN_THREADS];
    __shared__ uint32_t sseq[ALN_SCAN_THREADS], shdr[ALN_SCAN_THREADS];
    __shared__ uint32_t sdecline;
    const uint32_t per = (ntiles + ALN_SCAN_THREADS - 1) / ALN_SCAN_THREADS;
    const uint32_t lo = min(threadIdx.x * per, ntiles), hi = min(lo + per, ntiles);
    uint32_t m = imc::kAlnIdentityMap;
    for (uint32_t i = lo; i < hi; ++i) m = imc::aln_compose(m, sums[i].map);
    sm[threadIdx.x] = m;
    if (threadIdx.x == 0) sdecline = 0u;
    __syncthreads();
    for (int d = 1; d < ALN_SCAN_THREADS; d <<= 1) {           // inclusive scan in thread order
        uint32_t v = sm[threadIdx.x];
        if ((int)threadIdx.x >= d) v = imc::aln_compose(sm[threadIdx.x - d], v);
        __syncthreads();
        sm[threadIdx.x] = v;
        __syncthreads();
    }
    const uint32_t first = imc::aln_exit(threadIdx.x ? sm[threadIdx.x - 1] : imc::kAlnIdentityMap, entry);
    uint32_t state = first, seq = 0, hdr = 0, decline = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t map = sums[i].map;
        seq += sums[i].seq[state];
        hdr += sums[i].hdr[state];
        decline |= imc::aln_declines(map, state);
        state = imc::aln_exit(map, state);
    }
    sseq[threadIdx.x] = seq;
    shdr[threadIdx.x] = hdr;
    if (decline) atomicOr(&sdecline, 1u);
    __syncthreads();
    for (int d = 1; d < ALN_SCAN_THREADS; d <<= 1) {
        uint32_t a = sseq[threadIdx.x], b = shdr[threadIdx.x];
        if ((int)threadIdx.x >= d) { a += sseq[threadIdx.x - d]; b += shdr[threadIdx.x - d]; }
        __syncthreads();
        sseq[threadIdx.x] = a;
        shdr[threadIdx.x] = b;
        __syncthreads();
    }
    state = first;
    uint32_t run_seq = sseq[threadIdx.x] - seq, run_hdr = shdr[threadIdx.x] - hdr;
    for (uint32_t i = lo; i < hi; ++i) {
        tile_in[i] = AlnTileIn{state, run_seq, run_hdr, 0u};
        run_seq += sums[i].seq[state];
        run_hdr += sums[i].hdr[state];
        state = imc::aln_exit(sums[i].map, state);
    }
    if (threadIdx.x == ALN_SCAN_THREADS - 1)
        *total = imc::AlnTotal{imc::aln_exit(sm[ALN_SCAN_THREADS - 1], entry), sseq[ALN_SCAN_THREADS - 1], shdr[ALN_SCAN_THREADS - 1], sdecline};
}

// bases: the resident buffer (room bytes), base_kept: the kept bytes of all slabs before this one; table[rec_base + k]:
// header k of the slab, written while below rec_cap.
__global__ __launch_bounds__(ALN_THREADS) void k_aln_scatter(const uint8_t *slab, uint32_t n, uint32_t prev0, const AlnTileIn *tile_in, uint8_t *bases,
                                                            uint64_t base_kept, uint64_t room, imc::AlnRecord *table, uint32_t rec_base, uint32_t rec_cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ALN_FRONT + ALN_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t stage[ALN_TILE + 16];
    __shared__ uint32_t wave_map[ALN_THREADS / 64], wave_tot[ALN_THREADS / 64];
    const uint32_t tile_base = blockIdx.x * (uint32_t)ALN_TILE;
    aln_stage_tile(slab, tile_base, (uint8_t)prev0, sb);
    const imc::AlnSummary mine = aln_thread_summary(sb, tile_base, n);
    const AlnTileIn in = tile_in[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the state this thread's bytes are entered in: exclusive scan of the threads' maps
    uint32_t m = mine.map;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(m, d);
        if (lane >= d) m = imc::aln_compose(u, m);
    }
    if (lane == 63) wave_map[wave] = m;
    uint32_t before = __shfl_up(m, 1);
    if (lane == 0) before = imc::kAlnIdentityMap;
    __syncthreads();
    uint32_t front = imc::kAlnIdentityMap;
#pragma unroll
    for (int j = 0; j < ALN_THREADS / 64; ++j)
        if (j < wave) front = imc::aln_compose(front, wave_map[j]);
    const uint32_t entry = imc::aln_exit(imc::aln_compose(front, before), in.state);
    // exclusive scan of the threads' kept bytes (low half) and headers (high half): a tile holds at most 4096 of each
    const uint32_t own = imc::aln_pick(mine.seq, entry) | imc::aln_pick(mine.hdr, entry) << 16;
    uint32_t v = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    if (lane == 63) wave_tot[wave] = v;
    __syncthreads();
    uint32_t w = v - own, count = 0;
#pragma unroll
    for (int j = 0; j < ALN_THREADS / 64; ++j) {
        if (j < wave) w += wave_tot[j];
        count += wave_tot[j];
    }
    count &= 0xffffu;
    const uint64_t first = base_kept + in.seq;                 // where the tile's kept bytes go
    const uint32_t mis = (uint32_t)(first & 3u);
    uint32_t at_seq = w & 0xffffu, at_hdr = w >> 16;
    const uint32_t local = threadIdx.x * (uint32_t)ALN_ITEMS, at = tile_base + local;
    const uint32_t mine_n = at < n ? min(n - at, (uint32_t)ALN_ITEMS) : 0u;
    const uint8_t *p = sb + ALN_FRONT + local;
    uint32_t state = entry;
    for (uint32_t i = 0; i < (uint32_t)ALN_ITEMS; ++i)
        if (i < mine_n) {
            const imc::AlnStep st = imc::aln_step(state, p[(int)i - 1], p[i]);
            if (st.cls == imc::kAlnKept) {
                if (at_seq < (uint32_t)ALN_TILE) stage[mis + at_seq] = p[i];
                ++at_seq;
            } else if (st.cls == imc::kAlnHeaderStart) {
                const uint32_t rec = rec_base + in.hdr + at_hdr;
                if (rec < rec_cap) table[rec] = imc::AlnRecord{at + i, 0u, first + at_seq};
                ++at_hdr;
            }
            state = st.next;
        }
    __syncthreads();
    count = min(count, (uint32_t)ALN_TILE);
    if (first + count > room) return;
    // stage[mis ..) lies over the output's aligned words: whole words go out as words, the two ends byte by byte
    const uint32_t end = mis + count;
    uint8_t *dst = bases + (first - mis);
    for (uint32_t word = threadIdx.x; 4 * word < end; word += ALN_THREADS) {
        const uint32_t lo = 4 * word, hi = lo + 4;
        if (lo >= mis && hi <= end) reinterpret_cast<uint32_t *>(dst)[word] = reinterpret_cast<const uint32_t *>(stage)[word];
        else
            for (uint32_t b = max(lo, mis); b < min(hi, end); ++b) dst[b] = stage[b];
    }
}

// Columns ALN_COLUMNS i .. + 15 of the K sequences that start at bases + o0, o1, o2 (o2 unused for K = 2), each L bytes;
// dst is 16-byte aligned with zeroed room up to the next multiple of 16 columns.
template <int K>
__global__ __launch_bounds__(ALN_THREADS) void k_aln_columns(const uint8_t *bases, uint64_t o0, uint64_t o1, uint64_t o2, uint32_t L, uint8_t *dst)
{
    static_assert(K == 2 || K == 3, "pairs and triplets");
    const uint32_t i = blockIdx.x * (uint32_t)ALN_THREADS + threadIdx.x;
    if ((uint64_t)ALN_COLUMNS * i >= L) return;
    const uint32_t col0 = ALN_COLUMNS * i;
    uint32_t a[4], b[4], c[4] = {0u, 0u, 0u, 0u}, out[4];
    imc::aln_gather(bases, o0, col0, L, a);
    imc::aln_gather(bases, o1, col0, L, b);
    if (K == 3) imc::aln_gather(bases, o2, col0, L, c);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) out[j] = imc::aln_symbols<K>(a[j], b[j], c[j], L - col0 > 4 * j ? L - col0 - 4 * j : 0u);
    reinterpret_cast<uint4 *>(dst)[i] = make_uint4(out[0], out[1], out[2], out[3]);
}
