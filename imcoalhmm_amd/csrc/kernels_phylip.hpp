// kernels_phylip.hpp - PHYLIP alignments on the device: the sequences imc::read_phylip (phylip_io.hpp) produces on the
// host, from the bytes of the file, each record at r * length of the resident buffer.  Plain HIP for gfx950; the rules -
// what a byte is in which state, the summary of a range and how summaries combine, where a kept byte goes, the stride-n
// offsets - are the inline functions of phylip_tiles.hpp, which the CPU check drives against the host reader.
//
// A slab of the file (cut anywhere) is parsed by six launches, ordered by kernel boundaries only:
//   k_phy_summary   one workgroup per tile of TILE_SIZE bytes: the tile's summary as a function of the state it is entered in
//   k_phy_scan      ONE workgroup: from the cursor the slab is entered at, every tile's cursor (state, counted lines, the
//                   open line's printable and first-word bytes) and the slab's total
//   k_phy_count     one workgroup per tile: the kept bytes of every line of the tile, added up in LDS, go into the line
//                   table (integer atomics: the sum does not depend on the order), the name bytes into the name lengths
//   k_phy_partial   the stride-n scan of the line table for the lines that started in the slab: sums of pieces of chains,
//   k_phy_offsets   then every piece walks its rows from the sums in front of it
//   k_phy_scatter   one workgroup per tile: the kept bytes are compacted in LDS, line by line, and every line's run goes to
//                   its record at its offset, as aligned words where a word is the run's alone; name bytes go to the name
//                   table.  A run that would end outside its record is not written and raises kPhyFlagOutside.
// A tile is staged in LDS with the byte before it (aln_stage_tile); every use of a byte checks its offset against the
// slab's length, every table access its line against the table's size, every store its place against the record.
//
// No workgroup waits for another one, every loop bound is a constant or a launch argument or a value a previous launch
// wrote; offsets within a slab, line numbers and places within a record are 32-bit, offsets into the resident buffer 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_align.hpp"
#include "phylip_tiles.hpp"

constexpr int PHY_SEGMENTS = TILE_SIZE / 2 + 2;        // lines a tile can touch: the open one and a new one every two bytes

// the summary of this thread's bytes of the staged tile
__device__ inline imc::PhySummary phy_thread_summary(const uint8_t *sb, uint32_t tile_base, uint32_t n)
{
    const uint32_t local = threadIdx.x * (uint32_t)TILE_ITEMS, at = tile_base + local;
    const uint32_t count = at < n ? min(n - at, (uint32_t)TILE_ITEMS) : 0u;
    const uint8_t *p = sb + ALN_FRONT + local;
    return imc::phy_range(p, p[-1], count);
}

__global__ __launch_bounds__(TILE_THREADS) void k_phy_summary(const uint8_t *slab, uint32_t n, uint32_t prev0, imc::PhySummary *sums)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ALN_FRONT + TILE_SIZE];
    __shared__ imc::PhySummary part[TILE_THREADS];
    const uint32_t tile_base = blockIdx.x * (uint32_t)TILE_SIZE;
    aln_stage_tile(slab, tile_base, (uint8_t)prev0, sb);
    tile_wg_reduce<TILE_THREADS>(phy_thread_summary(sb, tile_base, n), part,
                                 [](const imc::PhySummary &a, const imc::PhySummary &b) { return imc::phy_combine(a, b); });
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

// One workgroup, two scans: the tiles' maps under composition give every tile the state it is entered in, then the
// tiles' runs in those states give the cursor in front of it.  entry: the cursor the slab is entered at.
__global__ __launch_bounds__(TILE_SCAN_THREADS) void k_phy_scan(const imc::PhySummary *sums, uint32_t ntiles, imc::PhyCursor entry, imc::PhyCursor *tile_in,
                                                               imc::PhyTotal *total)
{
    __shared__ imc::PhyRun sc[TILE_SCAN_THREADS];
    const uint32_t all_map = tile_scan_elements(
        ntiles, imc::kPhyIdentityMap, reinterpret_cast<uint32_t *>(sc), [&](uint32_t i) { return sums[i].map; },
        [](uint32_t a, uint32_t b) { return imc::phy_compose(a, b); },
        [&](uint32_t i, uint32_t before) { tile_in[i].state = imc::phy_exit(before, entry.state); });
    __syncthreads();                                   // (the runs reuse the maps' LDS)
    const imc::PhyRun all = tile_scan_elements(
        ntiles, imc::PhyRun{0u, 0u, 0u, 0u}, sc,
        [&](uint32_t i) { return imc::phy_run_of(sums[i], tile_in[i].state); },   // (the state: written above by this thread or kept below)
        [](const imc::PhyRun &a, const imc::PhyRun &b) { return imc::phy_run_combine(a, b); },
        [&](uint32_t i, const imc::PhyRun &before) { tile_in[i] = imc::phy_cursor_behind(entry, before, tile_in[i].state); });
    if (threadIdx.x == TILE_SCAN_THREADS - 1) {
        total->end = imc::phy_cursor_behind(entry, all, imc::phy_exit(all_map, entry.state));
        total->decline = all.flags & imc::kPhyMapDecline ? 1u : 0u;
    }
}

// The state and the counted lines in front of this thread's bytes: two exclusive scans over the workgroup.
__device__ inline imc::PhyCursor phy_thread_entry(const imc::PhySummary &mine, const imc::PhyCursor &in, uint32_t *wave_a, uint32_t *wave_b, uint32_t &tile_lines)
{
    uint32_t unused;
    const uint32_t front = tile_wg_scan(mine.map, imc::kPhyIdentityMap, [](uint32_t a, uint32_t b) { return imc::phy_compose(a, b); }, wave_a, unused);
    const uint32_t state = imc::phy_exit(front, in.state);
    const uint32_t lines = tile_wg_scan(imc::phy_pick(mine.lines, state), 0u, [](uint32_t a, uint32_t b) { return a + b; }, wave_b, tile_lines);
    return imc::PhyCursor{state, in.lines + lines, 0u, 0u};
}

// cnt[j] += the kept bytes of line j in this tile (j < cap); nlen[j - 1] += its name bytes (1 <= j <= nrec).
__global__ __launch_bounds__(TILE_THREADS) void k_phy_count(const uint8_t *slab, uint32_t n, uint32_t prev0, const imc::PhyCursor *tile_in, uint32_t nrec, uint32_t *cnt,
                                                          uint32_t *nlen, uint32_t cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ALN_FRONT + TILE_SIZE];
    __shared__ uint32_t seg_cnt[PHY_SEGMENTS];
    __shared__ uint32_t wave_a[TILE_THREADS / 64], wave_b[TILE_THREADS / 64];
    const uint32_t tile_base = blockIdx.x * (uint32_t)TILE_SIZE;
    for (uint32_t c = threadIdx.x; c < (uint32_t)PHY_SEGMENTS; c += TILE_THREADS) seg_cnt[c] = 0u;
    aln_stage_tile(slab, tile_base, (uint8_t)prev0, sb);
    const imc::PhyCursor in = tile_in[blockIdx.x];
    uint32_t tile_lines;
    imc::PhyCursor cur = phy_thread_entry(phy_thread_summary(sb, tile_base, n), in, wave_a, wave_b, tile_lines);
    const uint32_t local = threadIdx.x * (uint32_t)TILE_ITEMS, at = tile_base + local;
    const uint32_t mine_n = at < n ? min(n - at, (uint32_t)TILE_ITEMS) : 0u;
    const uint8_t *p = sb + ALN_FRONT + local;
    uint32_t run_j = 0u, run_kept = 0u, run_name = 0u;     // what this thread has seen of line run_j
    auto flush = [&]() {
        const uint32_t c = run_j + 1u - in.lines;           // the line's number within the tile: 0 is the one open in front of it
        if (run_kept && c < (uint32_t)PHY_SEGMENTS) atomicAdd(&seg_cnt[c], run_kept);
        if (run_name && run_j >= 1u && run_j <= nrec) atomicAdd(&nlen[run_j - 1u], run_name);
        run_kept = run_name = 0u;
    };
    for (uint32_t i = 0; i < (uint32_t)TILE_ITEMS; ++i)
        if (i < mine_n) {
            const imc::PhyPlace pl = imc::phy_advance(cur, p[(int)i - 1], p[i], nrec);
            if (pl.kind != imc::kPhyNothing) {
                if (pl.j != run_j) {
                    flush();
                    run_j = pl.j;
                }
                run_kept += pl.kind == imc::kPhyKeptByte ? 1u : 0u;
                run_name += pl.kind == imc::kPhyNameByte ? 1u : 0u;
            }
        }
    flush();
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < (uint32_t)PHY_SEGMENTS; c += TILE_THREADS) {
        const uint32_t kept = seg_cnt[c], j = in.lines + c - 1u;
        if (kept && in.lines + c >= 1u && j < cap) atomicAdd(&cnt[j], kept);
    }
}

// The lines [j0, total->end.lines) started in the slab (at most up to cap); `pieces` pieces of `rows` rows per chain.
__device__ inline uint32_t phy_slab_lines(const imc::PhyTotal *total, uint32_t j0, uint32_t cap)
{
    const uint32_t j1 = min(total->end.lines, cap);
    return j1 > j0 ? j1 - j0 : 0u;
}

__global__ __launch_bounds__(TILE_THREADS) void k_phy_partial(const uint32_t *cnt, const imc::PhyTotal *total, uint32_t j0, uint32_t cap, uint32_t nrec, uint32_t rows,
                                                            uint32_t pieces, uint32_t *part)
{
    const uint64_t unit = (uint64_t)blockIdx.x * TILE_THREADS + threadIdx.x;
    if (unit >= (uint64_t)pieces * nrec) return;
    const uint32_t q = (uint32_t)(unit / nrec), c = (uint32_t)(unit % nrec);
    part[unit] = imc::phy_chain_partial(cnt, j0, phy_slab_lines(total, j0, cap), nrec, rows, q, c);
}

__global__ __launch_bounds__(TILE_THREADS) void k_phy_offsets(const uint32_t *cnt, uint32_t *off, const uint32_t *part, const imc::PhyTotal *total, uint32_t j0,
                                                            uint32_t cap, uint32_t nrec, uint32_t rows, uint32_t pieces)
{
    const uint64_t unit = (uint64_t)blockIdx.x * TILE_THREADS + threadIdx.x;
    if (unit >= (uint64_t)pieces * nrec) return;
    const uint32_t q = (uint32_t)(unit / nrec), c = (uint32_t)(unit % nrec);
    imc::phy_chain_walk(cnt, off, part, j0, phy_slab_lines(total, j0, cap), nrec, rows, q, c);
}

// bases: the resident buffer, record r at r * length; names: nrec rows of kPhyNameMax bytes; total->flags collects the
// declines raised here.
__global__ __launch_bounds__(TILE_THREADS) void k_phy_scatter(const uint8_t *slab, uint32_t n, uint32_t prev0, const imc::PhyCursor *tile_in, uint32_t nrec,
                                                            uint32_t length, const uint32_t *off, uint32_t cap, uint8_t *bases, uint8_t *names, imc::PhyTotal *total)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[ALN_FRONT + TILE_SIZE];
    __shared__ __attribute__((aligned(16))) uint8_t stage[TILE_SIZE + 16];
    __shared__ uint32_t seg_start[PHY_SEGMENTS], seg_cnt[PHY_SEGMENTS], seg_rel[PHY_SEGMENTS];
    __shared__ uint32_t wave_a[TILE_THREADS / 64], wave_b[TILE_THREADS / 64], wave_c[TILE_THREADS / 64], wave_d[TILE_THREADS / 64];
    const uint32_t tile_base = blockIdx.x * (uint32_t)TILE_SIZE;
    for (uint32_t c = threadIdx.x; c < (uint32_t)PHY_SEGMENTS; c += TILE_THREADS) {
        seg_start[c] = 0xffffffffu;
        seg_cnt[c] = 0u;
    }
    aln_stage_tile(slab, tile_base, (uint8_t)prev0, sb);
    const imc::PhySummary mine = phy_thread_summary(sb, tile_base, n);
    const imc::PhyCursor in = tile_in[blockIdx.x];
    uint32_t tile_lines, unused;
    imc::PhyCursor cur = phy_thread_entry(mine, in, wave_a, wave_b, tile_lines);
    // the open line's printable (bits 13-25) and first-word (bits 0-12) bytes in front of this thread; bit 31: a '\n' lies
    // between the tile's start and this thread
    const uint32_t brk = mine.map & imc::kPhyMapBreak ? 1u << 31 : 0u;
    const uint32_t pw = tile_wg_scan(
        brk | imc::phy_pick(mine.P, cur.state) << 13 | imc::phy_pick(mine.W, cur.state), 0u,
        [](uint32_t a, uint32_t b) { return b >> 31 ? b : (a & 1u << 31) | ((a & 0x7fffffffu) + b); }, wave_c, unused);
    cur.P = (pw >> 31 ? 0u : in.P) + ((pw >> 13) & 0x1fffu);
    cur.W = (pw >> 31 ? 0u : in.W) + (pw & 0x1fffu);
    const uint32_t local = threadIdx.x * (uint32_t)TILE_ITEMS, at = tile_base + local;
    const uint32_t mine_n = at < n ? min(n - at, (uint32_t)TILE_ITEMS) : 0u;
    const uint8_t *p = sb + ALN_FRONT + local;
    // this thread's kept bytes, and where they stand among the tile's
    uint32_t kept = 0u;
    {
        imc::PhyCursor c = cur;
        for (uint32_t i = 0; i < (uint32_t)TILE_ITEMS; ++i)
            if (i < mine_n) kept += imc::phy_advance(c, p[(int)i - 1], p[i], nrec).kind == imc::kPhyKeptByte ? 1u : 0u;
    }
    uint32_t k = tile_wg_scan(kept, 0u, [](uint32_t a, uint32_t b) { return a + b; }, wave_d, unused);
    uint32_t flags = 0u, run_c = 0xffffffffu, run_kept = 0u;     // what this thread has kept of the tile's line run_c
    for (uint32_t i = 0; i < (uint32_t)TILE_ITEMS; ++i)
        if (i < mine_n) {
            const imc::PhyPlace pl = imc::phy_advance(cur, p[(int)i - 1], p[i], nrec);
            flags |= pl.flag;
            if (pl.kind == imc::kPhyNameByte) {
                if (pl.pos < imc::kPhyNameMax) names[(size_t)(pl.j - 1u) * imc::kPhyNameMax + pl.pos] = p[i];
            } else if (pl.kind == imc::kPhyKeptByte) {
                const uint32_t c = pl.j + 1u - in.lines;   // the line's number within the tile: 0 is the one open in front of it
                if (c < (uint32_t)PHY_SEGMENTS && k < (uint32_t)TILE_SIZE) {
                    stage[k] = p[i];
                    if (c != run_c) {
                        if (run_kept) atomicAdd(&seg_cnt[run_c], run_kept);
                        atomicMin(&seg_start[c], k);
                        seg_rel[c] = pl.pos - k;           // (the same for every kept byte of the line in this tile)
                        run_c = c;
                        run_kept = 0u;
                    }
                    ++run_kept;
                }
                ++k;
            }
        }
    if (run_kept) atomicAdd(&seg_cnt[run_c], run_kept);
    __syncthreads();
    // one team per line: the workgroup when the tile holds few lines, else a wavefront
    const uint32_t nseg = min(tile_lines + 1u, (uint32_t)PHY_SEGMENTS);
    const uint32_t team = nseg <= 4u ? (uint32_t)TILE_THREADS : 64u, lane = threadIdx.x % team;
    for (uint32_t c = threadIdx.x / team; c < nseg; c += TILE_THREADS / team) {
        const uint32_t count = seg_cnt[c];
        if (!count) continue;
        const uint32_t j = in.lines + c - 1u, start = seg_start[c];
        if (in.lines + c < 2u) continue;                   // (nothing of the header line is kept)
        if (j >= cap) { flags |= imc::kPhyFlagLines; continue; }
        const uint64_t first = (uint64_t)off[j] + (uint32_t)(seg_rel[c] + start);
        if (first + count > length) { flags |= imc::kPhyFlagOutside; continue; }
        const uint64_t dest0 = (uint64_t)((j - 1u) % nrec) * length + first;
        // stage[start - mis ..) lies over the output's aligned words: whole words go out as words, the two ends byte by byte
        const uint32_t mis = (uint32_t)(dest0 & 3u), end = mis + count;
        uint8_t *dst = bases + (dest0 - mis);
        for (uint32_t word = lane; 4 * word < end; word += team) {
            const uint32_t lo = 4 * word, hi = lo + 4;
            if (lo >= mis && hi <= end) {
                const uint8_t *s = stage + (start + lo - mis);
                reinterpret_cast<uint32_t *>(dst)[word] = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
            } else
                for (uint32_t b = max(lo, mis); b < min(hi, end); ++b) dst[b] = stage[start + b - mis];
        }
    }
    if (flags) atomicOr(&total->flags, flags);
}
