// plan_host.hpp - host-only launch geometry of the forward engine.  Two layers, both pure functions:
//  - the schedules the table-build, GEMM-chain and blocked-scan kernels run from, of (dictionary, S, A), of
//    (segments, slabs) or of (B, blocks);
//  - what a plan is made of once imc::decide_groups (planner_host.hpp) has decided: plan_geometry() cuts the segments,
//    forms the stitch units, level-0 vectors, block lists, fused-tail records and the stitch hierarchy; group_schedules()
//    gathers a group's schedules of the first layer.
// No HIP and no device pointer here: imcoal_fwd.hip resolves the segment cuts against its chunk handles and uploads
// the rest as it stands (PlanBuilder::upload), tests/plan_host_check.cpp checks all of it on the CPU under ASan/UBSan.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "launch_desc.hpp"
#include "pair_dict.hpp"
#include "planner_host.hpp"

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

// Workgroup list of the GEMM chain: {segment, slab, level-0 vector, 0} per entry.  A first
// segment is a vector and takes one workgroup; every other segment takes one per column slab.  Non-first segments are
// dealt in tiles of 8 segments x nslab so that the slabs of one segment sit 8 ids apart (same XCD -> they share the
// operator rows in L2); the first segments come last.
inline std::vector<BigBlock> deal_slabs(const std::vector<uint32_t> &seg_ids, const std::vector<uint32_t> &seg_out,
                                        const std::vector<uint8_t> &seg_first, int nslab)
{
    std::vector<BigBlock> firsts, rest, dealt;
    for (size_t i = 0; i < seg_ids.size(); ++i) {       // segment-major
        const bool fst = seg_first[seg_ids[i]] != 0;
        for (int sl = 0; sl < (fst ? 1 : nslab); ++sl)
            (fst ? firsts : rest).push_back(BigBlock{seg_ids[i], (uint32_t)sl, seg_out[i], 0u});
    }
    const size_t ns = (size_t)nslab;
    for (size_t base = 0; base < rest.size(); base += 8 * ns) {
        const size_t nseg = std::min<size_t>(8, (rest.size() - base) / ns);
        for (size_t sl = 0; sl < ns; ++sl)
            for (size_t k = 0; k < nseg; ++k) dealt.push_back(rest[base + k * ns + sl]);
    }
    for (const BigBlock &bb : firsts) dealt.push_back(bb);
    return dealt;
}

// Block list of the rank-one hand-off's tail launches: one entry per segment (first segments included).
inline std::vector<BigBlock> tail_list(const std::vector<uint32_t> &seg_ids, const std::vector<uint32_t> &seg_out)
{
    std::vector<BigBlock> tails;
    for (size_t i = 0; i < seg_ids.size(); ++i) tails.push_back(BigBlock{seg_ids[i], 0u, seg_out[i], 0u});
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

// ---- the geometry of one plan: what every kernel indexes device memory through ----

// One segment as the host cuts it; the engine turns it into a SegDesc, whose pointer is the stream's device base +
// offset * (2 for SEG_WIDE, else 1).
struct SegCut {
    uint32_t chunk;
    size_t offset;        // first stream element of the segment
    uint32_t len, flags;  // SEG_FIRST | SEG_WIDE
};

struct GroupGeometry {     // a launch group's part
    uint32_t vec_begin = 0, n_vecs = 0;
    uint64_t vsteps = 0;   // executed vector-steps per parameter set (columns or tokens)
    uint64_t stream_len = 0;
    // GemmChain / MatVecChain
    std::vector<uint32_t> seg_ids, seg_out;   // segment ids and their level-0 vector index
    // BlockedLds / BlockedGlobal
    std::vector<Z2Block> blocks;              // one entry per workgroup
    std::vector<Z2Tail> tails;                // fused tail (zip3_tail): per workgroup {chunk, unit, units of the chunk}
    int tail_stride = 0;
};

struct HostLevel {         // one level of the stitch hierarchy, level 0 = propagate output (the stitch units)
    std::vector<uint32_t> chunk_seg, vec0;    // chunk -> its first unit (n_chunks + 1 entries); unit -> its first vector
    std::vector<uint8_t> first;
    std::vector<ChainDesc> chains;            // chains that produce THIS level from the previous one
    uint32_t n_vecs = 0;
};

struct PlanGeometry {
    bool too_many_vectors = false;      // the call is refused: nothing after the vectors was built
    std::vector<SegCut> segs;           // all segments, chunk order
    std::vector<uint8_t> seg_first;
    std::vector<uint32_t> chunk_seg;    // chunk -> first segment (n_chunks + 1 entries)
    std::vector<VecDesc> vecs;          // level-0 vectors
    std::vector<GroupGeometry> groups;
    std::vector<HostLevel> levels;
    std::vector<int32_t> final_vec;     // chunk -> its single remaining unit's vector at the last level (-1: empty chunk)
    bool finish_fused = false;          // the last chain level writes the log-likelihoods itself (no k_finish launch)
    uint64_t chain_steps = 0;           // serial depth of the stitch (sum over levels of the longest chain)
    size_t pstride = 0;                 // doubles per parameter set
};

// mfma: the blocked kernels of this plan are the fp64-MFMA ones (kc.use3(blocked_variant), or the wide scan).
inline PlanGeometry plan_geometry(const PlanDecision &dec, const std::vector<ChunkFacts> &chunks, const KernelFacts &kc,
                                  int N, int S, bool op_mode, bool mfma)
{
    PlanGeometry g;
    const int n_chunks = (int)chunks.size();
    std::vector<SegCut> &segs = g.segs;
    std::vector<uint8_t> &seg_first = g.seg_first;
    std::vector<uint32_t> &chunk_seg = g.chunk_seg;
    std::vector<VecDesc> &vecs = g.vecs;
    auto stream_length = [&](const GroupDecision &gr, int f) { return gr.tokens ? chunks[f].level[gr.level].ntok : chunks[f].L; };

    // ---- segments in chunk order ----
    chunk_seg.assign(n_chunks + 1, 0);
    for (int f = 0; f < n_chunks; ++f) {
        chunk_seg[f] = (uint32_t)segs.size();
        const GroupDecision &gr = dec.groups[dec.chunk_group[f]];
        const size_t L = stream_length(gr, f);
        if (!L) continue;
        const size_t K0 = (L + gr.seglen - 1) / gr.seglen;
        const size_t sl = round_up((L + K0 - 1) / K0, is_blocked(gr.kind) ? Z2GRAN : 16);   // equalised; a multiple of 16 (16-byte aligned
                                                                                        // loads) except for the blocked kernels
        for (size_t off = 0, k = 0; off < L; off += sl, ++k) {
            const bool wide = gr.tokens ? chunks[f].level[gr.level].wide : chunks[f].wide_raw;
            const bool fst = k == 0 && !op_mode;   // operator mode: the chunk's own first segment is an operator too
            segs.push_back(SegCut{(uint32_t)f, off, (uint32_t)std::min(sl, L - off), (fst ? SEG_FIRST : 0u) | (wide ? SEG_WIDE : 0u)});
            seg_first.push_back(fst);
        }
    }
    chunk_seg[n_chunks] = (uint32_t)segs.size();

    // ---- stitch units and their vectors, contiguous per group ----
    // A unit is what the stitch hierarchy sees at level 0: a segment, or (blocked kernel) a workgroup's
    // run of up to 32 consecutive segments of one chunk, already folded inside the kernel.
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> chunk_units(n_chunks);   // per chunk: (seg0, nsegs)
    for (int f = 0; f < n_chunks; ++f) {
        const GroupDecision &gr = dec.groups[dec.chunk_group[f]];
        const uint32_t step = is_blocked(gr.kind) ? (uint32_t)kc.z4_slots() : 1u;
        for (uint32_t sid = chunk_seg[f]; sid < chunk_seg[f + 1]; sid += step)
            chunk_units[f].push_back({sid, std::min(step, chunk_seg[f + 1] - sid)});
    }
    std::vector<uint32_t> chunk_unit(n_chunks + 1, 0);
    for (int f = 0; f < n_chunks; ++f) chunk_unit[f + 1] = chunk_unit[f] + (uint32_t)chunk_units[f].size();
    std::vector<uint32_t> unit_vec0(chunk_unit[n_chunks], 0);
    std::vector<uint8_t> unit_first(chunk_unit[n_chunks], 0);
    g.groups.resize(dec.groups.size());
    for (size_t q = 0; q < dec.groups.size(); ++q) {
        const GroupDecision &gr = dec.groups[q];
        GroupGeometry &gg = g.groups[q];
        const bool blocked = is_blocked(gr.kind);
        gg.vec_begin = (uint32_t)vecs.size();
        for (int f : gr.chunks) {
            gg.stream_len += stream_length(gr, f);
            for (size_t u = 0; u < chunk_units[f].size(); ++u) {
                const uint32_t sid = chunk_units[f][u].first, ns = chunk_units[f][u].second;
                const uint32_t uid = chunk_unit[f] + (uint32_t)u;
                const bool fst = seg_first[sid] != 0;
                unit_first[uid] = fst;
                unit_vec0[uid] = (uint32_t)vecs.size();
                const int nv = fst ? 1 : N;
                for (int c = 0; c < nv; ++c) vecs.push_back(VecDesc{sid, (uint32_t)c});
                if (is_chain(gr.kind)) { gg.seg_ids.push_back(sid); gg.seg_out.push_back(unit_vec0[uid]); }
                if (blocked) {
                    std::vector<Z2Block> &blocks = gg.blocks;
                    // A chunk that is ONE segment needs no fold: up to 32 consecutive such chunks share a workgroup, each
                    // in a slot of its own (Z2Block::first == 2).  One workgroup per chunk left 31 of 32 rows idle when
                    // the chunks are short (10000 chunks of 1e4 columns, 20 states: 39 rounds of workgroups, 1.97 ms).
                    const bool whole = mfma && fst && ns == 1 && chunk_units[f].size() == 1;
                    if (whole && !blocks.empty() && blocks.back().first == 2 && blocks.back().n < (uint32_t)kc.z4_slots() &&
                        blocks.back().seg0 + blocks.back().n == sid && blocks.back().out_vec0 + blocks.back().n == unit_vec0[uid])
                        ++blocks.back().n;
                    else
                        blocks.push_back(Z2Block{sid, ns, unit_vec0[uid], whole ? 2u : fst ? 1u : 0u});
                }
                for (uint32_t q2 = 0; q2 < ns; ++q2)
                    gg.vsteps += (uint64_t)((seg_first[sid + q2] && !blocked) ? 1 : N) * segs[sid + q2].len;
            }
        }
        gg.n_vecs = (uint32_t)vecs.size() - gg.vec_begin;
    }
    // fused tail: one blocked-MFMA group holds every chunk, no chunk is empty or longer than a workgroup has slots
    if (dec.groups.size() == 1 && is_blocked(dec.groups[0].kind) && mfma && !op_mode && n_chunks > 0) {
        GroupGeometry &bl = g.groups[0];
        bool ok = true;
        size_t most = 0;
        for (int f = 0; f < n_chunks; ++f) {
            ok = ok && !chunk_units[f].empty() && chunk_units[f].size() <= (size_t)kc.z4_slots();
            most = std::max(most, chunk_units[f].size());
        }
        if (ok) {
            for (int f : dec.groups[0].chunks)
                for (size_t u = 0; u < chunk_units[f].size(); ++u)
                    bl.tails.push_back(Z2Tail{(uint32_t)f, (uint32_t)u, (uint32_t)chunk_units[f].size(), 0u});
            bl.tail_stride = (int)most;
            if (bl.tails.size() != bl.blocks.size()) bl.tails.clear();      // packed blocks: several chunks share a workgroup
            else
                for (Z2Block &bk : bl.blocks)                               // (a packed block of ONE chunk is an ordinary first block,
                    if (bk.first == 2) bk.first = 1;                        //  and the fused tail writes that chunk's result)
        }
    }
    if (vecs.size() >= (size_t)UINT32_MAX / 2) { g.too_many_vectors = true; return g; }
    const uint32_t n_vecs = (uint32_t)vecs.size();
    g.pstride = round_up((size_t)kc.NP + (size_t)kc.NP * kc.NP + (size_t)S * kc.NP, 2);

    // ---- stitch hierarchy: fold runs of g ~ sqrt(K) consecutive segments until one vector per chunk ----
    std::vector<HostLevel> &hl = g.levels;
    hl.assign(1, HostLevel());
    hl[0].chunk_seg = std::move(chunk_unit); hl[0].vec0 = std::move(unit_vec0); hl[0].first = std::move(unit_first); hl[0].n_vecs = n_vecs;
    for (;;) {
        const HostLevel &cur = hl.back();
        uint32_t kmax = 0;
        for (int f = 0; f < n_chunks; ++f) kmax = std::max(kmax, cur.chunk_seg[f + 1] - cur.chunk_seg[f]);
        // a level whose chunks all hold one first-vector is final; level 0 operators always need one pass
        if (kmax <= 1 && hl.size() > 1) break;
        if (kmax == 0) break;
        // ~3 levels: per level a chain costs g serial steps (0.38 us each at 20 states, profiles/mb_chain_step.txt) plus
        // one launch (~3 us up to its second step)
        const uint32_t gsz = kmax <= 16 ? kmax : std::max<uint32_t>(12, (uint32_t)std::ceil(std::cbrt((double)kmax)));
        g.chain_steps += gsz;
        HostLevel nx;
        nx.chunk_seg.assign(n_chunks + 1, 0);
        nx.n_vecs = 0;
        for (int f = 0; f < n_chunks; ++f) {
            nx.chunk_seg[f] = (uint32_t)nx.vec0.size();
            const uint32_t s0 = cur.chunk_seg[f], s1 = cur.chunk_seg[f + 1];
            for (uint32_t rb = s0; rb < s1; rb += gsz) {
                const uint32_t re = std::min(rb + gsz, s1);
                const bool fst = rb == s0 && !op_mode;
                nx.vec0.push_back(nx.n_vecs);
                nx.first.push_back(fst);
                const int nvv = fst ? 1 : N;
                // the start vector and the first operator's vectors: known here, so no chain looks them up on the device
                const uint32_t op0 = rb + (fst ? 1u : 0u);
                const uint32_t vec_first = fst ? cur.vec0[rb] : 0u, vbase = op0 < re ? cur.vec0[op0] : 0u;
                for (int c = 0; c < nvv; ++c)
                    nx.chains.push_back(ChainDesc{rb, re, (uint32_t)c, nx.n_vecs + c, fst ? 1u : 0u, 0u, vec_first, vbase});
                nx.n_vecs += nvv;
            }
        }
        nx.chunk_seg[n_chunks] = (uint32_t)nx.vec0.size();
        const bool done = kmax <= gsz;
        hl.push_back(std::move(nx));
        if (done) break;
    }
    std::vector<int32_t> &final_vec = g.final_vec;
    final_vec.assign(std::max(n_chunks, 1), -1);
    bool all_from_chains = hl.size() > 1 && !op_mode && n_chunks > 0;
    for (int f = 0; f < n_chunks; ++f) {
        const HostLevel &last = hl.back();
        if (last.chunk_seg[f + 1] > last.chunk_seg[f]) final_vec[f] = (int32_t)last.vec0[last.chunk_seg[f]];
        else all_from_chains = false;               // an empty chunk: k_finish writes its 0.0
    }
    // every chunk's final vector comes out of a chain of the last level: those chains write the log-likelihoods
    // themselves and k_finish is not launched
    g.finish_fused = false;
    if (all_from_chains) {
        HostLevel &last = hl.back();
        std::vector<char> seen((size_t)n_chunks, 0);
        for (ChainDesc &cd : last.chains)
            for (int f = 0; f < n_chunks; ++f)
                if (cd.first && final_vec[f] == (int32_t)cd.out_vec) { cd.chunk1 = (uint32_t)f + 1; seen[f] = 1; }
        g.finish_fused = std::all_of(seen.begin(), seen.end(), [](char c) { return c != 0; });
        if (!g.finish_fused)
            for (ChainDesc &cd : last.chains) cd.chunk1 = 0;
    }
    return g;
}

// ---- a group's schedules: what its launches read beside the geometry ----

struct GroupSchedules {
    // GemmChain / MatVecChain
    std::vector<BigBlock> big_blocks;         // one entry per (segment, column slab) workgroup
    std::vector<std::pair<int, int>> table_runs;   // (first, count) in the dictionary's depth order per k_big_table_level launch
    std::vector<BigBlock> tail_blocks;        // rank-one hand-off: one entry per segment (operator tails and first segments)
    std::vector<std::pair<uint32_t, uint32_t>> r1_segs;   // ... (plan-wide id, length) of the operator segments
    // BlockedLds / BlockedGlobal on tokens: merged tokens of the alphabet by dictionary depth (tab.lvl: the depth offsets)
    DepthOrder tab;
    // global table: its build's descriptor lists with their launch lists (first entry, entries)
    std::vector<Desc4> tab_desc;              // {token, left, right, 0} per entry of the depth order
    TableSchedule tab2;                       // two Desc4 per entry of the two-depths-per-launch schedule (k_z4_level2)
    TableSchedule tab3;                       // three Desc4 per token of the three-depths-per-launch schedule (k_z4_level3)
    bool stream_table = false;                // nothing cached in LDS: the launch's tables are small enough to stay cache resident
    int n_hot = 0;                            // hybrid table: operators cached in LDS
    std::vector<tok_t> hot;
    PhaseTable phases;                        // the XCD-affine grid of the scan (used when B > 1)
};

// wide: the plan runs 25-32 states on the streamed blocked scan.  dict: the group's dictionary (token groups), else null.
inline GroupSchedules group_schedules(const PlanOptions &opt, const KernelFacts &kc, bool wide, const GroupDecision &gr,
                                      const PlanGeometry &g, const GroupGeometry &gg, const std::vector<ChunkFacts> &chunks,
                                      const TrainedDict *dict, int S, int B)
{
    GroupSchedules s;
    if (gr.kind == GroupKind::BlockedGlobal) {
        // hot set: the most frequent tokens of this group's chunks, as many as LDS holds beside the identity
        std::vector<uint64_t> cnt((size_t)gr.A, 0);
        for (int f : gr.chunks) {
            const std::vector<uint32_t> &tc = chunks[f].level[gr.level].counts();
            for (size_t z = 0; z < tc.size() && z < cnt.size(); ++z) cnt[z] += tc[z];
        }
        const std::vector<tok_t> ids = hot_order(cnt);
        const double tables = (double)B * (gr.A + 1) * kc.tok_doubles * 8.0;
        s.stream_table = wide || z4_streamed(opt, tables, B);
        s.n_hot = s.stream_table ? 0 : std::min(gr.A, kc.zip4_max_hot(gr.A, LDS_BUDGET));
        s.hot.assign(ids.begin(), ids.begin() + s.n_hot);
        s.phases = xcd_phases(B, (int)gg.blocks.size());
    }
    if (is_blocked(gr.kind) && gr.tokens) {
        s.tab = depth_order_below(dict->order, dict->depth, gr.A);
        if (gr.kind == GroupKind::BlockedGlobal) {
            s.tab_desc = level_descriptors(dict->dict, s.tab);
            s.tab2 = pairs_schedule(dict->dict, dict->depth, s.tab, S);
            s.tab3 = triples_schedule(dict->dict, dict->depth, s.tab, S, gr.A);
        }
    }
    if (!is_chain(gr.kind)) return s;
    if (gr.tokens) s.table_runs = depth_runs_below(dict->order, dict->depth, gr.A);
    s.big_blocks = deal_slabs(gg.seg_ids, gg.seg_out, g.seg_first, kc.big_nslab);
    if (gr.rank1) {
        s.tail_blocks = tail_list(gg.seg_ids, gg.seg_out);
        for (uint32_t id : gg.seg_ids)
            if (!g.seg_first[id]) s.r1_segs.push_back({id, g.segs[id].len});
    }
    return s;
}

}  // namespace imc
