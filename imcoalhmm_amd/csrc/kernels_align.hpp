// kernels_align.hpp - FASTA alignments on the device: the sequences imc::read_fasta (fasta_io.hpp) produces on the host,
// from the bytes of the file, and the symbols of a pair's or a triplet's chunk from sequences that stay resident.  Plain
// HIP for gfx950; the rules - what a byte is in which state, the summary of a range of bytes and how summaries combine,
// the column rules - are the inline functions of align_tiles.hpp, which the CPU check drives against the host reader.
//
// PARSE.  A slab of the file (never cut inside a header line) is parsed by three launches, ordered by kernel boundaries
// only:
//   k_aln_summary   one workgroup per tile of TILE_SIZE bytes: the tile's summary as a function of the state it is entered in
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
#include "tile_scan.hpp"

constexpr int ALN_FRONT = 16;                          // LDS bytes in front of the tile (the last one: the byte before it)
constexpr int ALN_COLUMNS = (int)imc::kAlnColumns;     // columns per thread of k_aln_columns

struct AlnTileIn {
    uint32_t state, seq, hdr, pad;                     // the tile's entry state; kept bytes and headers of the slab in front of it
};

// The tile's bytes into LDS: sb[ALN_FRONT + i] = slab[tile_base + i] for -1 <= i < TILE_SIZE (16-byte loads; the slab
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
    const uint32_t local = threadIdx.x * (uint32_t)TILE_ITEMS, at = tile_base + local;
    const uint32_t count = at < n ? min(n - at, (uint32_t)TILE_ITEMS) : 0u;
    const uint8_t *p = sb + ALN_FRONT + local;
    return imc::aln_range(p, p[-1], count);
}

__global__ __launch_bounds__(TILE_THREADS) void k_aln_summary(const uint8_t *slab, uint32_t n, uint32_t prev0, imc::AlnSummary *sums)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ALN_FRONT + TILE_SIZE];
    __shared__ imc::AlnSummary part[TILE_THREADS];
    const uint32_t tile_base = blockIdx.x * (uint32_t)TILE_SIZE;
    aln_stage_tile(slab, tile_base, (uint8_t)prev0, sb);
    tile_wg_reduce<TILE_THREADS>(aln_thread_summary(sb, tile_base, n), part,
                                 [](const imc::AlnSummary &a, const imc::AlnSummary &b) { return imc::aln_combine(a, b); });
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

struct AlnCounts {
    uint32_t seq, hdr, decline;                        // kept bytes, headers, and whether a tile declines, of a run of tiles
};

// One workgroup, two scans: the tiles' maps under composition give every tile the state it is entered in, then the
// tiles' counts in those states, under addition, give the kept bytes and headers in front of it.
__global__ __launch_bounds__(TILE_SCAN_THREADS) void k_aln_scan(const imc::AlnSummary *sums, uint32_t ntiles, uint32_t entry, AlnTileIn *tile_in,
                                                               imc::AlnTotal *total)
{
    __shared__ AlnCounts sc[TILE_SCAN_THREADS];
    const uint32_t all_map = tile_scan_elements(
        ntiles, imc::kAlnIdentityMap, reinterpret_cast<uint32_t *>(sc), [&](uint32_t i) { return sums[i].map; },
        [](uint32_t a, uint32_t b) { return imc::aln_compose(a, b); },
        [&](uint32_t i, uint32_t before) { tile_in[i].state = imc::aln_exit(before, entry); });
    __syncthreads();                                   // (the counts reuse the maps' LDS)
    const AlnCounts all = tile_scan_elements(
        ntiles, AlnCounts{0u, 0u, 0u}, sc,
        [&](uint32_t i) {
            const uint32_t state = tile_in[i].state;   // (written above by this thread: the shares are the same)
            return AlnCounts{sums[i].seq[state], sums[i].hdr[state], imc::aln_declines(sums[i].map, state)};
        },
        [](const AlnCounts &a, const AlnCounts &b) { return AlnCounts{a.seq + b.seq, a.hdr + b.hdr, a.decline | b.decline}; },
        [&](uint32_t i, const AlnCounts &before) { tile_in[i] = AlnTileIn{tile_in[i].state, before.seq, before.hdr, 0u}; });
    if (threadIdx.x == TILE_SCAN_THREADS - 1) *total = imc::AlnTotal{imc::aln_exit(all_map, entry), all.seq, all.hdr, all.decline};
}

// bases: the resident buffer (room bytes), base_kept: the kept bytes of all slabs before this one; table[rec_base + k]:
// header k of the slab, written while below rec_cap.
__global__ __launch_bounds__(TILE_THREADS) void k_aln_scatter(const uint8_t *slab, uint32_t n, uint32_t prev0, const AlnTileIn *tile_in, uint8_t *bases,
                                                            uint64_t base_kept, uint64_t room, imc::AlnRecord *table, uint32_t rec_base, uint32_t rec_cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ALN_FRONT + TILE_SIZE];
    __shared__ __attribute__((aligned(16))) uint8_t stage[TILE_SIZE + 16];
    __shared__ uint32_t wave_map[TILE_THREADS / 64], wave_tot[TILE_THREADS / 64];
    const uint32_t tile_base = blockIdx.x * (uint32_t)TILE_SIZE;
    aln_stage_tile(slab, tile_base, (uint8_t)prev0, sb);
    const imc::AlnSummary mine = aln_thread_summary(sb, tile_base, n);
    const AlnTileIn in = tile_in[blockIdx.x];
    // the state this thread's bytes are entered in: exclusive scan of the threads' maps
    uint32_t unused;
    const uint32_t front = tile_wg_scan(mine.map, imc::kAlnIdentityMap, [](uint32_t a, uint32_t b) { return imc::aln_compose(a, b); }, wave_map, unused);
    const uint32_t entry = imc::aln_exit(front, in.state);
    // exclusive scan of the threads' kept bytes (low half) and headers (high half): a tile holds at most 4096 of each
    uint32_t count;
    const uint32_t w = tile_wg_scan(imc::aln_pick(mine.seq, entry) | imc::aln_pick(mine.hdr, entry) << 16, 0u,
                                    [](uint32_t a, uint32_t b) { return a + b; }, wave_tot, count);
    count &= 0xffffu;
    const uint64_t first = base_kept + in.seq;                 // where the tile's kept bytes go
    const uint32_t mis = (uint32_t)(first & 3u);
    uint32_t at_seq = w & 0xffffu, at_hdr = w >> 16;
    const uint32_t local = threadIdx.x * (uint32_t)TILE_ITEMS, at = tile_base + local;
    const uint32_t mine_n = at < n ? min(n - at, (uint32_t)TILE_ITEMS) : 0u;
    const uint8_t *p = sb + ALN_FRONT + local;
    uint32_t state = entry;
    for (uint32_t i = 0; i < (uint32_t)TILE_ITEMS; ++i)
        if (i < mine_n) {
            const imc::AlnStep st = imc::aln_step(state, p[(int)i - 1], p[i]);
            if (st.cls == imc::kAlnKept) {
                if (at_seq < (uint32_t)TILE_SIZE) stage[mis + at_seq] = p[i];
                ++at_seq;
            } else if (st.cls == imc::kAlnHeaderStart) {
                const uint32_t rec = rec_base + in.hdr + at_hdr;
                if (rec < rec_cap) table[rec] = imc::AlnRecord{at + i, 0u, first + at_seq};
                ++at_hdr;
            }
            state = st.next;
        }
    __syncthreads();
    count = min(count, (uint32_t)TILE_SIZE);
    if (first + count > room) return;
    // stage[mis ..) lies over the output's aligned words: whole words go out as words, the two ends byte by byte
    const uint32_t end = mis + count;
    uint8_t *dst = bases + (first - mis);
    for (uint32_t word = threadIdx.x; 4 * word < end; word += TILE_THREADS) {
        const uint32_t lo = 4 * word, hi = lo + 4;
        if (lo >= mis && hi <= end) reinterpret_cast<uint32_t *>(dst)[word] = reinterpret_cast<const uint32_t *>(stage)[word];
        else
            for (uint32_t b = max(lo, mis); b < min(hi, end); ++b) dst[b] = stage[b];
    }
}

// Columns ALN_COLUMNS i .. + 15 of the K sequences that start at bases + o0, o1, o2 (o2 unused for K = 2), each L bytes;
// dst is 16-byte aligned with zeroed room up to the next multiple of 16 columns.
template <int K>
__global__ __launch_bounds__(TILE_THREADS) void k_aln_columns(const uint8_t *bases, uint64_t o0, uint64_t o1, uint64_t o2, uint32_t L, uint8_t *dst)
{
    static_assert(K == 2 || K == 3, "pairs and triplets");
    const uint32_t i = blockIdx.x * (uint32_t)TILE_THREADS + threadIdx.x;
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
