// plan_host.hpp - host-only launch geometry of the forward engine: the schedules the table-build, GEMM-chain and
// blocked-scan kernels run from, as pure functions of (dictionary, S, A), of (segments, slabs) or of (B, blocks).
// No HIP here: imcoal_fwd.hip uploads what these return (PlanBuilder::upload), tests/plan_host_check.cpp checks them
// on the CPU under ASan/UBSan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "pair_dict.hpp"

namespace imc {

// One descriptor entry as the table-build kernels load it (an int4 on the device).
struct alignas(16) Desc4 { int32_t x, y, z, w; };
static_assert(sizeof(Desc4) == 16 && alignof(Desc4) == 16, "Desc4 is one 16-byte load");

// A schedule of table-build launches: the descriptor list and, per launch, (first entry, entries).
struct TableSchedule {
    std::vector<Desc4> desc;
    std::vector<std::pair<int, int>> launches;
};

// Merged tokens of a level's alphabet (ids S .. A-1) grouped by dictionary depth: the tokens of the k-th depth present
// are order[lvl[k] .. lvl[k+1]).
struct DepthOrder {
    std::vector<tok_t> order;
    std::vector<int> lvl;
    int nlvl = 0;
};

inline DepthOrder depth_order_below(const std::vector<tok_t> &dict_order, const std::vector<int> &depth, int A)
{
    DepthOrder o;
    o.lvl.assign(1, 0);
    int cur = -1;
    for (tok_t z : dict_order) {                        // (sorted by depth, then id)
        if ((int)z >= A) continue;
        if (depth[z] != cur) {
            if (cur >= 0) o.lvl.push_back((int)o.order.size());
            cur = depth[z];
        }
        o.order.push_back(z);
    }
    o.lvl.push_back((int)o.order.size());
    o.nlvl = o.order.empty() ? 0 : (int)o.lvl.size() - 1;
    return o;
}

// Runs (first index, count) of the dictionary's WHOLE depth order that hold one depth and only ids < A: what
// k_big_table_level is launched over, one launch per run (tokens of a depth are independent).
inline std::vector<std::pair<int, int>> depth_runs_below(const std::vector<tok_t> &dict_order, const std::vector<int> &depth, int A)
{
    std::vector<std::pair<int, int>> runs;
    size_t i0 = 0;
    while (i0 < dict_order.size()) {
        size_t i1 = i0;
        while (i1 < dict_order.size() && depth[dict_order[i1]] == depth[dict_order[i0]]) ++i1;
        size_t r0 = i0;                                 // the contiguous sub-runs of [i0, i1) whose token id < A
        while (r0 < i1) {
            while (r0 < i1 && (int)dict_order[r0] >= A) ++r0;
            size_t r1 = r0;
            while (r1 < i1 && (int)dict_order[r1] < A) ++r1;
            if (r1 > r0) runs.push_back({(int)r0, (int)(r1 - r0)});
            r0 = r1;
        }
        i0 = i1;
    }
    return runs;
}

// One depth per launch (k_z4_level): {token, left, right, 0} per entry of the depth order.
inline std::vector<Desc4> level_descriptors(const PairDict &d, const DepthOrder &o)
{
    std::vector<Desc4> desc;
    for (tok_t z : o.order) desc.push_back(Desc4{(int)z, (int)d.left[z], (int)d.right[z], 0});
    return desc;
}

// Two depths per launch (k_z4_level2), two Desc4 per entry: launch k builds depths 2k+1 and 2k+2; a second-depth token
// whose child sits in the first depth recomputes it from the grandchildren.  Entries of a launch: the first depth's,
// then the second depth's grouped by which children they recompute (flags: 1 left, 2 right, 3 both), every group
// padded to whole wavefronts (four entries) with idle entries (token -1).
inline TableSchedule pairs_schedule(const PairDict &d, const std::vector<int> &depth, const DepthOrder &o, int S)
{
    TableSchedule s;
    std::vector<Desc4> &d2 = s.desc;
    const std::vector<int> &lvl = o.lvl;
    auto pad4 = [&]() { while ((d2.size() / 2) % 4) { d2.push_back(Desc4{-1, 0, 0, 0}); d2.push_back(Desc4{0, 0, 0, 0}); } };
    for (int dl = 0; dl < o.nlvl; dl += 2) {
        const int first = (int)(d2.size() / 2);
        for (int k = lvl[dl]; k < lvl[dl + 1]; ++k) {
            const int z = o.order[k];
            d2.push_back(Desc4{z, (int)d.left[z], (int)d.right[z], 0});
            d2.push_back(Desc4{0, 0, 0, 0});
        }
        pad4();
        if (dl + 1 < o.nlvl) {
            const int d_first = depth[o.order[lvl[dl]]];
            for (int flags = 1; flags <= 3; ++flags) {
                for (int k = lvl[dl + 1]; k < lvl[dl + 2]; ++k) {
                    const int z = o.order[k], zl = d.left[z], zr = d.right[z];
                    const bool nl = zl >= S && depth[zl] == d_first, nr = zr >= S && depth[zr] == d_first;
                    if ((nl ? 1 : 0) + (nr ? 2 : 0) != flags) continue;
                    d2.push_back(Desc4{z, zl, zr, flags});
                    d2.push_back(Desc4{nl ? (int)d.left[zl] : 0, nl ? (int)d.right[zl] : 0,
                                       nr ? (int)d.left[zr] : 0, nr ? (int)d.right[zr] : 0});
                }
                pad4();
            }
        }
        s.launches.push_back({first, (int)(d2.size() / 2) - first});
    }
    return s;
}

// Three depths per launch (k_z4_level3), three Desc4 per token - {token, leaves 0-2}, {leaves 3-6}, {leaf 7}: launch k
// builds depths 3k+1 .. 3k+3, one wavefront per token; a token's eight leaves are the nodes of its dictionary tree that
// lie at depth <= 3k (already in the table), a ready node in the first leaf of its range and the identity (encoded as
// A) in the rest of it.
inline TableSchedule triples_schedule(const PairDict &d, const std::vector<int> &depth, const DepthOrder &o, int S, int A)
{
    TableSchedule s;
    std::vector<Desc4> &d3 = s.desc;
    const std::vector<int> &lvl = o.lvl;
    for (int dl = 0; dl < o.nlvl; dl += 3) {
        const int first = (int)(d3.size() / 3);
        const int d_ready = depth[o.order[lvl[dl]]] - 1;                // entries up to this depth exist
        for (int k = lvl[dl]; k < lvl[std::min(dl + 3, o.nlvl)]; ++k) {
            int leaves[8];
            for (int &x : leaves) x = A;                                // the identity entry
            struct Fill {
                const PairDict &d; const std::vector<int> &depth; int S, d_ready; int *leaves;
                void operator()(int t, int lo, int hi) const
                {
                    if (t < S || depth[t] <= d_ready || hi - lo == 1) { leaves[lo] = t; return; }
                    const int mid = (lo + hi) / 2;
                    (*this)((int)d.left[t], lo, mid);
                    (*this)((int)d.right[t], mid, hi);
                }
            } fill{d, depth, S, d_ready, leaves};
            fill((int)o.order[k], 0, 8);
            d3.push_back(Desc4{(int)o.order[k], leaves[0], leaves[1], leaves[2]});
            d3.push_back(Desc4{leaves[3], leaves[4], leaves[5], leaves[6]});
            d3.push_back(Desc4{leaves[7], 0, 0, 0});
        }
        s.launches.push_back({first, (int)(d3.size() / 3) - first});
    }
    return s;
}

// Hot set of the hybrid table: the token ids 0 .. count.size()-1 by falling count (ties: by id); the caller takes as
// many from the front as LDS holds.
inline std::vector<tok_t> hot_order(const std::vector<uint64_t> &count)
{
    std::vector<tok_t> ids(count.size());
    for (size_t z = 0; z < ids.size(); ++z) ids[z] = (tok_t)z;
    std::stable_sort(ids.begin(), ids.end(), [&](tok_t x, tok_t y) { return count[x] > count[y]; });
    return ids;
}

// Workgroup list of the GEMM chain.  Block is {segment, slab, level-0 vector, 0} (BigBlock on the device).  A first
// segment is a vector and takes one workgroup; every other segment takes one per column slab.  Non-first segments are
// dealt in tiles of 8 segments x nslab so that the slabs of one segment sit 8 ids apart (same XCD -> they share the
// operator rows in L2); the first segments come last.
template <class Block>
std::vector<Block> deal_slabs(const std::vector<uint32_t> &seg_ids, const std::vector<uint32_t> &seg_out,
                              const std::vector<uint8_t> &seg_first, int nslab)
{
    std::vector<Block> firsts, rest, dealt;
    for (size_t i = 0; i < seg_ids.size(); ++i) {       // segment-major
        const bool fst = seg_first[seg_ids[i]] != 0;
        for (int sl = 0; sl < (fst ? 1 : nslab); ++sl)
            (fst ? firsts : rest).push_back(Block{seg_ids[i], (uint32_t)sl, seg_out[i], 0u});
    }
    const size_t ns = (size_t)nslab;
    for (size_t base = 0; base < rest.size(); base += 8 * ns) {
        const size_t nseg = std::min<size_t>(8, (rest.size() - base) / ns);
        for (size_t sl = 0; sl < ns; ++sl)
            for (size_t k = 0; k < nseg; ++k) dealt.push_back(rest[base + k * ns + sl]);
    }
    for (const Block &bb : firsts) dealt.push_back(bb);
    return dealt;
}

// Block list of the rank-one hand-off's tail launches: one entry per segment (first segments included).
template <class Block>
std::vector<Block> tail_list(const std::vector<uint32_t> &seg_ids, const std::vector<uint32_t> &seg_out)
{
    std::vector<Block> tails;
    for (size_t i = 0; i < seg_ids.size(); ++i) tails.push_back(Block{seg_ids[i], 0u, seg_out[i], 0u});
    return tails;
}

// XCD-affine grid of k_zpropagate4 (BigArgs::n_phases): B parameter sets x `blocks` workgroups on a one-dimensional
// grid of `grid` workgroups, cut into phases that each load the eight XCDs evenly - the B / 8 * 8 sets eight at a
// time, then phases of four, two and one set for the bits of B % 8.
struct PhaseTable {
    int n_phases = 0, ph_begin[4] = {0, 0, 0, 0}, ph_first[4] = {0, 0, 0, 0}, ph_sets[4] = {0, 0, 0, 0};
    int grid = 0;
};

inline PhaseTable xcd_phases(int B, int blocks)
{
    PhaseTable t;
    int first = 0, wg = 0;
    auto phase = [&](int sets, int n_sets_total) {
        t.ph_begin[t.n_phases] = wg; t.ph_first[t.n_phases] = first; t.ph_sets[t.n_phases] = sets;
        ++t.n_phases;
        wg += sets >= 8 ? 8 * blocks * (n_sets_total / 8) : 8 * ((blocks + 8 / sets - 1) / (8 / sets));
        first += n_sets_total;
    };
    if (B >= 8) phase(8, B / 8 * 8);
    for (int sets : {4, 2, 1})
        if ((B % 8) & sets) phase(sets, sets);
    t.grid = wg;
    return t;
}

}  // namespace imc
