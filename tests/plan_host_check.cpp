#include "../imcoalhmm_amd/csrc/pair_dict.hpp"
#include "../imcoalhmm_amd/csrc/plan_host.hpp"
#include "plan_check_common.hpp"
#include <cstdio>
#include <set>
#include <string>
// The launch schedules of plan_host.hpp on trained dictionaries, checked against what the kernels that run from them
// need: every table entry is built exactly once, from operands that are raw symbols or were finished by an EARLIER
// launch, and the product it describes is the token's own (the expansion of a token is the string of raw symbols
// obtained by recursive left + right).
// The geometry of a plan (plan_geometry) the same way: decisions made as tests/planner_host_check.cpp makes them, and
// for every result what the kernels need of the segments, stitch units, vectors, block lists, fused-tail records and the
// stitch hierarchy they index device memory through.  Built with -fsanitize=address,undefined.

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static int n_cases = 0, max_tokens = 0, max_depth_seen = 0;

static int check_dictionary(const imc::PairDict &d, int A, const std::vector<std::string> &exp)
{
    const int S = d.nsym;
    const std::vector<int> depth = imc::dict_depths(d);
    const std::vector<imc::tok_t> all = imc::dict_order(d, depth);
    CHECK((int)all.size() == d.alphabet - S, "A %d", A);
    const imc::DepthOrder o = imc::depth_order_below(all, depth, A);

    // depth order: every token S .. A-1 once, depths do not decrease, the offsets cut at the depth changes
    {
        std::vector<int> seen((size_t)A, 0);
        for (size_t k = 0; k < o.order.size(); ++k) {
            const int z = o.order[k];
            CHECK(z >= S && z < A && !seen[z]++, "token %d", z);
            if (k) CHECK(depth[o.order[k - 1]] < depth[z] || (depth[o.order[k - 1]] == depth[z] && o.order[k - 1] < z), "position %zu", k);
        }
        CHECK((int)o.order.size() == A - S, "%zu tokens of %d", o.order.size(), A - S);
        CHECK(o.nlvl == (o.order.empty() ? 0 : (int)o.lvl.size() - 1) && o.lvl.front() == 0 && o.lvl.back() == (int)o.order.size(), "offsets");
        for (int l = 0; l < o.nlvl; ++l) {
            CHECK(o.lvl[l] < o.lvl[l + 1], "empty depth %d", l);
            for (int k = o.lvl[l]; k < o.lvl[l + 1]; ++k) CHECK(depth[o.order[k]] == depth[o.order[o.lvl[l]]], "depth %d", l);
            if (l) CHECK(depth[o.order[o.lvl[l]]] > depth[o.order[o.lvl[l] - 1]], "depth %d", l);
        }
    }
    // one depth per launch: {token, left, right, 0} in the depth order
    {
        const std::vector<imc::Desc4> desc = imc::level_descriptors(d, o);
        CHECK(desc.size() == o.order.size(), "size");
        for (size_t k = 0; k < desc.size(); ++k)
            CHECK(desc[k].x == o.order[k] && desc[k].y == d.left[o.order[k]] && desc[k].z == d.right[o.order[k]] && desc[k].w == 0, "entry %zu", k);
    }
    // pairs
    {
        const imc::TableSchedule s = imc::pairs_schedule(d, depth, o, S);
        CHECK(s.desc.size() % 2 == 0, "size");
        std::vector<int> built((size_t)A, 0), ready((size_t)A, 0);       // ready: raw, or built by an earlier launch
        for (int z = 0; z < S; ++z) ready[z] = 1;
        int next = 0;
        for (const auto &lc : s.launches) {
            CHECK(lc.first == next && lc.second > 0 && lc.second % 4 == 0, "launch at %d: %d entries", lc.first, lc.second);
            next = lc.first + lc.second;
            CHECK((size_t)next * 2 <= s.desc.size(), "launch past the list");
            for (int e = lc.first; e < next; ++e) {
                const imc::Desc4 a = s.desc[2 * (size_t)e], g = s.desc[2 * (size_t)e + 1];
                if (a.x == -1) continue;                                   // idle entry
                CHECK(a.x >= S && a.x < A && !built[a.x]++, "token %d", a.x);
                CHECK(a.y >= 0 && a.y < A && a.z >= 0 && a.z < A && a.w >= 0 && a.w <= 3, "entry %d", e);
                std::string left, right;
                if (a.w & 1) {
                    CHECK(a.y >= S && g.x == d.left[a.y] && g.y == d.right[a.y] && ready[g.x] && ready[g.y], "token %d left", a.x);
                    left = exp[g.x] + exp[g.y];
                } else {
                    CHECK(ready[a.y], "token %d: left child %d not ready", a.x, a.y);
                    left = exp[a.y];
                }
                if (a.w & 2) {
                    CHECK(a.z >= S && g.z == d.left[a.z] && g.w == d.right[a.z] && ready[g.z] && ready[g.w], "token %d right", a.x);
                    right = exp[g.z] + exp[g.w];
                } else {
                    CHECK(ready[a.z], "token %d: right child %d not ready", a.x, a.z);
                    right = exp[a.z];
                }
                CHECK(left + right == exp[a.x], "token %d: product", a.x);
            }
            // k_z4_level2 runs four entries per wavefront: one flag value per group of four, the first depth's groups
            // (no recompute) ahead of the second depth's, those in the order of their flags
            int last_flags = 0;
            for (int e0 = lc.first; e0 < next; e0 += 4) {
                int flags = -1;
                for (int e = e0; e < e0 + 4; ++e) {
                    const imc::Desc4 a = s.desc[2 * (size_t)e];
                    if (a.x == -1) continue;
                    CHECK(flags < 0 || flags == a.w, "entries %d..%d mix the flags %d and %d", e0, e0 + 3, flags, a.w);
                    flags = a.w;
                }
                CHECK(flags >= last_flags, "group at %d: flags %d after %d", e0, flags, last_flags);   // (a group is never all idle)
                last_flags = flags;
            }
            for (int e = lc.first; e < next; ++e)
                if (s.desc[2 * (size_t)e].x >= 0) ready[s.desc[2 * (size_t)e].x] = 1;
        }
        CHECK((size_t)next * 2 == s.desc.size(), "launches do not tile the list");
        for (int z = S; z < A; ++z) CHECK(built[z] == 1, "token %d built %d times", z, built[z]);
    }
    // triples
    {
        const imc::TableSchedule s = imc::triples_schedule(d, depth, o, S, A);
        CHECK(s.desc.size() % 3 == 0, "size");
        std::vector<int> built((size_t)A, 0), ready((size_t)A, 0);
        for (int z = 0; z < S; ++z) ready[z] = 1;
        int next = 0;
        for (const auto &lc : s.launches) {
            CHECK(lc.first == next && lc.second > 0, "launch at %d", lc.first);
            next = lc.first + lc.second;
            CHECK((size_t)next * 3 <= s.desc.size(), "launch past the list");
            for (int e = lc.first; e < next; ++e) {
                const imc::Desc4 a = s.desc[3 * (size_t)e], b = s.desc[3 * (size_t)e + 1], c = s.desc[3 * (size_t)e + 2];
                const int leaves[8] = {a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x};
                CHECK(a.x >= S && a.x < A && !built[a.x]++, "token %d", a.x);
                std::string prod;
                for (int leaf : leaves) {
                    if (leaf == A) continue;                               // the identity
                    CHECK(leaf >= 0 && leaf < A && ready[leaf], "token %d: leaf %d not ready", a.x, leaf);
                    prod += exp[leaf];
                }
                CHECK(prod == exp[a.x], "token %d: product", a.x);
            }
            for (int e = lc.first; e < next; ++e) ready[s.desc[3 * (size_t)e].x] = 1;
        }
        CHECK((size_t)next * 3 == s.desc.size(), "launches do not tile the list");
        for (int z = S; z < A; ++z) CHECK(built[z] == 1, "token %d built %d times", z, built[z]);
    }
    // depth runs of the whole dictionary order: exactly the ids < A, one depth per run
    {
        std::vector<int> seen((size_t)d.alphabet, 0);
        int last_end = 0;
        for (const auto &run : imc::depth_runs_below(all, depth, A)) {
            CHECK(run.first >= last_end && run.second > 0 && (size_t)(run.first + run.second) <= all.size(), "run at %d", run.first);
            last_end = run.first + run.second;
            for (int k = run.first; k < last_end; ++k) {
                CHECK((int)all[k] < A && !seen[all[k]]++ && depth[all[k]] == depth[all[run.first]], "run at %d, entry %d", run.first, k);
            }
        }
        for (int z = S; z < d.alphabet; ++z) CHECK(seen[z] == (z < A ? 1 : 0), "token %d in %d runs", z, seen[z]);
    }
    ++n_cases;
    max_tokens = std::max(max_tokens, A);
    for (int z = S; z < A; ++z) max_depth_seen = std::max(max_depth_seen, depth[z]);
    return 0;
}

static int check_hot_order(std::mt19937 &rng)
{
    for (int n : {0, 1, 5, 256, 4096}) {
        std::vector<uint64_t> count((size_t)n);
        for (auto &c : count) c = rng() % 7 == 0 ? 0 : rng() % 50;            // many ties
        const std::vector<imc::tok_t> ids = imc::hot_order(count);
        CHECK((int)ids.size() == n, "size");
        std::set<int> seen(ids.begin(), ids.end());
        CHECK((int)seen.size() == n, "not a permutation");
        for (int k = 1; k < n; ++k)
            CHECK(count[ids[k - 1]] > count[ids[k]] || (count[ids[k - 1]] == count[ids[k]] && ids[k - 1] < ids[k]), "position %d", k);
    }
    return 0;
}

static int check_dealing(std::mt19937 &rng)
{
    for (int nslab : {1, 2, 3, 7, 8})
        for (int nseg : {0, 1, 7, 8, 9, 16, 61}) {
            std::vector<uint8_t> seg_first((size_t)nseg + 5, 0);
            std::vector<uint32_t> seg_ids, seg_out;
            for (int k = 0; k < nseg + 5; ++k) {
                seg_first[k] = rng() % 4 == 0;
                if (k % 6 != 5) { seg_ids.push_back((uint32_t)k); seg_out.push_back((uint32_t)(1000 + 3 * k)); }   // (the group holds part of the plan's segments)
            }
            const std::vector<BigBlock> wg = imc::deal_slabs(seg_ids, seg_out, seg_first, nslab);
            std::set<std::pair<uint32_t, uint32_t>> want, got;
            size_t n_first = 0;
            for (uint32_t id : seg_ids) {
                n_first += seg_first[id];
                for (int sl = 0; sl < (seg_first[id] ? 1 : nslab); ++sl) want.insert({id, (uint32_t)sl});
            }
            for (const BigBlock &b : wg) {
                CHECK(got.insert({b.seg, b.slab}).second && b.out_vec0 == 1000 + 3 * b.seg && b.pad == 0, "segment %u slab %u", b.seg, b.slab);
            }
            CHECK(got == want, "not a permutation of the (segment, slab) pairs");
            const size_t n_rest = wg.size() - n_first;
            for (size_t k = 0; k < wg.size(); ++k) CHECK((seg_first[wg[k].seg] != 0) == (k >= n_rest), "first segments come last (%zu)", k);
            for (size_t base = 0; base + 8 * (size_t)nslab <= n_rest; base += 8 * (size_t)nslab)         // full tiles
                for (size_t k = 0; k < 8; ++k)
                    for (int sl = 0; sl < nslab; ++sl)
                        CHECK(wg[base + 8 * sl + k].seg == wg[base + k].seg && wg[base + 8 * sl + k].slab == (uint32_t)sl, "tile at %zu", base);
            const std::vector<BigBlock> tails = imc::tail_list(seg_ids, seg_out);
            CHECK(tails.size() == seg_ids.size(), "size");
            for (size_t k = 0; k < tails.size(); ++k)
                CHECK(tails[k].seg == seg_ids[k] && tails[k].slab == 0 && tails[k].out_vec0 == seg_out[k] && tails[k].pad == 0, "tail %zu", k);
        }
    return 0;
}

// The workgroup -> (parameter set, block) rule of k_zpropagate4, restated from kernels_zip4.hpp (the `a.n_phases > 0`
// block at the top of the kernel): returns false for a workgroup the kernel returns from.
static bool decode_workgroup(const imc::PhaseTable &t, int nb, int wg, int &b, int &bx)
{
    int ph = 0;
    while (ph + 1 < t.n_phases && wg >= t.ph_begin[ph + 1]) ++ph;
    const int local = wg - t.ph_begin[ph], xcd = local & 7, turn = local >> 3;
    const int sets = t.ph_sets[ph];
    if (sets >= 8) {
        b = t.ph_first[ph] + xcd + 8 * (turn / nb);
        bx = turn % nb;
    } else {
        b = t.ph_first[ph] + xcd % sets;
        bx = turn * (8 / sets) + xcd / sets;
        if (bx >= nb) return false;
    }
    return true;
}

static int check_phases()
{
    for (int B = 2; B <= 26; ++B)
        for (int blocks : {1, 2, 3, 7, 8, 9, 33}) {
            const imc::PhaseTable t = imc::xcd_phases(B, blocks);
            CHECK(t.n_phases >= 1 && t.n_phases <= 4 && t.ph_begin[0] == 0 && t.grid > 0, "B %d blocks %d", B, blocks);
            std::vector<int> hit((size_t)B * blocks, 0);
            for (int wg = 0; wg < t.grid; ++wg) {
                int b = -1, bx = -1;
                if (!decode_workgroup(t, blocks, wg, b, bx)) continue;
                CHECK(b >= 0 && b < B && bx >= 0 && bx < blocks, "B %d blocks %d: workgroup %d -> (%d, %d)", B, blocks, wg, b, bx);
                hit[(size_t)b * blocks + bx]++;
            }
            for (int k = 0; k < B * blocks; ++k) CHECK(hit[k] == 1, "B %d blocks %d: (set %d, block %d) hit %d times", B, blocks, k / blocks, k % blocks, hit[k]);
        }
    return 0;
}

// ---- the geometry of a plan ----

static long n_geo = 0, n_packed = 0, n_tail = 0, n_tail_withdrawn = 0, n_ff[2], n_empty_chunk = 0, n_op_mode = 0, n_deep = 0, n_geo_kind[6];

static bool same_geometry(const imc::PlanGeometry &a, const imc::PlanGeometry &b)
{
    auto eq = [](const auto &x, const auto &y, auto same) {
        if (x.size() != y.size()) return false;
        for (size_t k = 0; k < x.size(); ++k) if (!same(x[k], y[k])) return false;
        return true;
    };
    auto chain = [](const ChainDesc &x, const ChainDesc &y) {
        return x.seg_begin == y.seg_begin && x.seg_end == y.seg_end && x.c == y.c && x.out_vec == y.out_vec && x.first == y.first &&
               x.chunk1 == y.chunk1 && x.vec_first == y.vec_first && x.vbase == y.vbase;
    };
    auto group = [&](const imc::GroupGeometry &x, const imc::GroupGeometry &y) {
        return x.vec_begin == y.vec_begin && x.n_vecs == y.n_vecs && x.vsteps == y.vsteps && x.stream_len == y.stream_len &&
               x.seg_ids == y.seg_ids && x.seg_out == y.seg_out && x.tail_stride == y.tail_stride &&
               eq(x.blocks, y.blocks, [](const Z2Block &p, const Z2Block &q) { return p.seg0 == q.seg0 && p.n == q.n && p.out_vec0 == q.out_vec0 && p.first == q.first; }) &&
               eq(x.tails, y.tails, [](const Z2Tail &p, const Z2Tail &q) { return p.chunk == q.chunk && p.unit == q.unit && p.n_units == q.n_units && p.pad == q.pad; });
    };
    auto level = [&](const imc::HostLevel &x, const imc::HostLevel &y) {
        return x.chunk_seg == y.chunk_seg && x.vec0 == y.vec0 && x.first == y.first && x.n_vecs == y.n_vecs && eq(x.chains, y.chains, chain);
    };
    return a.too_many_vectors == b.too_many_vectors && a.seg_first == b.seg_first && a.chunk_seg == b.chunk_seg && a.final_vec == b.final_vec &&
           a.finish_fused == b.finish_fused && a.chain_steps == b.chain_steps && a.pstride == b.pstride &&
           eq(a.segs, b.segs, [](const imc::SegCut &p, const imc::SegCut &q) { return p.chunk == q.chunk && p.offset == q.offset && p.len == q.len && p.flags == q.flags; }) &&
           eq(a.vecs, b.vecs, [](const VecDesc &p, const VecDesc &q) { return p.seg == q.seg && p.c == q.c; }) &&
           eq(a.groups, b.groups, group) && eq(a.levels, b.levels, level);
}

static int check_geometry(const imc::PlanDecision &dec, const std::vector<imc::ChunkFacts> &chunks, const imc::KernelFacts &kc,
                          int N, int S, bool op_mode, bool mfma)
{
    using namespace imc;
    const PlanGeometry g = plan_geometry(dec, chunks, kc, N, S, op_mode, mfma);
    ++n_geo;
    n_op_mode += op_mode;
    const int n_chunks = (int)chunks.size();
    const uint32_t slots = (uint32_t)kc.z4_slots();
    CHECK(!g.too_many_vectors, "refused");
    CHECK(g.pstride == round_up((size_t)kc.NP + (size_t)kc.NP * kc.NP + (size_t)S * kc.NP, 2), "pstride %zu", g.pstride);
    auto group_of = [&](int f) -> const GroupDecision & { return dec.groups[dec.chunk_group[f]]; };
    auto length_of = [&](int f) { const GroupDecision &gr = group_of(f); return gr.tokens ? chunks[f].level[gr.level].ntok : chunks[f].L; };

    // ---- segments: every chunk's stream covered exactly once, in order ----
    CHECK((int)g.chunk_seg.size() == n_chunks + 1 && g.chunk_seg[0] == 0 && g.chunk_seg[n_chunks] == g.segs.size() && g.seg_first.size() == g.segs.size(), "chunk_seg");
    bool any_empty = false;
    for (int f = 0; f < n_chunks; ++f) {
        const GroupDecision &gr = group_of(f);
        const size_t gran = is_blocked(gr.kind) ? Z2GRAN : 16, L = length_of(f);
        const bool wide = gr.tokens ? chunks[f].level[gr.level].wide : chunks[f].wide_raw;
        CHECK(g.chunk_seg[f] <= g.chunk_seg[f + 1], "chunk %d", f);
        size_t at = 0;
        for (uint32_t sid = g.chunk_seg[f]; sid < g.chunk_seg[f + 1]; ++sid) {
            const SegCut &sc = g.segs[sid];
            CHECK(sc.chunk == (uint32_t)f && sc.offset == at && sc.len > 0 && sc.offset % gran == 0, "chunk %d segment %u: offset %zu len %u", f, sid, sc.offset, sc.len);
            const bool fst = sid == g.chunk_seg[f] && !op_mode;
            CHECK(((sc.flags & SEG_FIRST) != 0) == fst && (g.seg_first[sid] != 0) == fst, "chunk %d segment %u: first", f, sid);
            CHECK(((sc.flags & SEG_WIDE) != 0) == wide && !(sc.flags & ~(SEG_FIRST | SEG_WIDE)), "chunk %d segment %u: flags %u", f, sid, sc.flags);
            at += sc.len;
        }
        CHECK(at == L, "chunk %d: %zu of %zu elements covered", f, at, L);
        any_empty = any_empty || L == 0;
    }
    n_empty_chunk += any_empty;

    // ---- level 0: the stitch units, read off the vectors (a unit's vectors name its first segment) ----
    CHECK(!g.levels.empty(), "no level");
    const HostLevel &l0 = g.levels[0];
    CHECK((int)l0.chunk_seg.size() == n_chunks + 1 && l0.chunk_seg[0] == 0 && l0.chunk_seg[n_chunks] == l0.vec0.size() && l0.first.size() == l0.vec0.size() &&
          l0.chains.empty() && l0.n_vecs == g.vecs.size(), "level 0");
    std::vector<uint32_t> unit_seg0(l0.vec0.size()), unit_ns(l0.vec0.size());
    const uint32_t NO_UNIT = UINT32_MAX;
    std::vector<uint32_t> unit_at_seg(g.segs.size(), NO_UNIT);   // a unit's first segment -> the unit
    for (int f = 0; f < n_chunks; ++f) {
        const bool blocked = is_blocked(group_of(f).kind);
        const uint32_t u0 = l0.chunk_seg[f], u1 = l0.chunk_seg[f + 1];
        CHECK(u0 <= u1 && (u0 == u1) == (g.chunk_seg[f] == g.chunk_seg[f + 1]), "chunk %d: units", f);
        for (uint32_t uid = u0; uid < u1; ++uid) {
            CHECK(l0.vec0[uid] < g.vecs.size(), "unit %u", uid);
            unit_seg0[uid] = g.vecs[l0.vec0[uid]].seg;
        }
        for (uint32_t uid = u0; uid < u1; ++uid) {         // the units tile the chunk's segments in order
            const uint32_t end = uid + 1 < u1 ? unit_seg0[uid + 1] : g.chunk_seg[f + 1];
            CHECK(unit_seg0[uid] == (uid == u0 ? g.chunk_seg[f] : unit_seg0[uid - 1] + unit_ns[uid - 1]) && end > unit_seg0[uid] && end <= g.chunk_seg[f + 1], "chunk %d unit %u", f, uid);
            unit_ns[uid] = end - unit_seg0[uid];
            CHECK(unit_ns[uid] <= slots && (blocked || unit_ns[uid] == 1), "chunk %d unit %u: %u segments", f, uid, unit_ns[uid]);
            CHECK((l0.first[uid] != 0) == (g.seg_first[unit_seg0[uid]] != 0), "unit %u: first", uid);
            unit_at_seg[unit_seg0[uid]] = uid;
        }
    }

    // ---- groups: vectors contiguous per group in group order; vsteps, stream_len; the chain family's lists ----
    CHECK(g.groups.size() == dec.groups.size(), "groups");
    uint32_t next_vec = 0;
    for (size_t q = 0; q < dec.groups.size(); ++q) {
        const GroupDecision &gr = dec.groups[q];
        const GroupGeometry &gg = g.groups[q];
        const bool blocked = is_blocked(gr.kind), chain = is_chain(gr.kind);
        n_geo_kind[(int)gr.kind]++;
        CHECK(gg.vec_begin == next_vec, "group %zu: vec_begin %u", q, gg.vec_begin);
        uint64_t vsteps = 0, stream = 0;
        std::vector<uint32_t> ids, outs;
        for (int f : gr.chunks) {
            stream += length_of(f);
            for (uint32_t uid = l0.chunk_seg[f]; uid < l0.chunk_seg[f + 1]; ++uid) {
                CHECK(l0.vec0[uid] == next_vec, "group %zu chunk %d unit %u: vector %u", q, f, uid, l0.vec0[uid]);
                const uint32_t nv = l0.first[uid] ? 1u : (uint32_t)N;
                CHECK((size_t)next_vec + nv <= g.vecs.size(), "unit %u", uid);
                for (uint32_t c = 0; c < nv; ++c) CHECK(g.vecs[next_vec + c].seg == unit_seg0[uid] && g.vecs[next_vec + c].c == c, "vector %u", next_vec + c);
                next_vec += nv;
                ids.push_back(unit_seg0[uid]); outs.push_back(l0.vec0[uid]);
            }
            for (uint32_t sid = g.chunk_seg[f]; sid < g.chunk_seg[f + 1]; ++sid) vsteps += (uint64_t)((g.seg_first[sid] && !blocked) ? 1 : N) * g.segs[sid].len;
        }
        CHECK(gg.n_vecs == next_vec - gg.vec_begin && gg.vsteps == vsteps && gg.stream_len == stream, "group %zu: n_vecs %u vsteps %llu stream %llu", q, gg.n_vecs,
              (unsigned long long)gg.vsteps, (unsigned long long)gg.stream_len);
        if (chain) CHECK(gg.seg_ids == ids && gg.seg_out == outs, "group %zu: chain segments", q);
        else CHECK(gg.seg_ids.empty() && gg.seg_out.empty(), "group %zu: chain segments on kind %d", q, (int)gr.kind);

        // ---- blocks: cover the group's segments exactly once, unit by unit or (packed) chunk by chunk ----
        if (!blocked) { CHECK(gg.blocks.empty() && gg.tails.empty(), "group %zu: blocks on kind %d", q, (int)gr.kind); continue; }
        std::vector<uint32_t> want;                       // the group's segments in its order
        for (int f : gr.chunks) for (uint32_t sid = g.chunk_seg[f]; sid < g.chunk_seg[f + 1]; ++sid) want.push_back(sid);
        size_t w = 0;
        bool packed = false;
        for (size_t i = 0; i < gg.blocks.size(); ++i) {
            const Z2Block &bk = gg.blocks[i];
            CHECK(bk.n >= 1 && bk.n <= slots && w + bk.n <= want.size() && bk.first <= 2, "group %zu block %zu", q, i);
            for (uint32_t k = 0; k < bk.n; ++k) CHECK(want[w + k] == bk.seg0 + k, "group %zu block %zu: segment %u", q, i, bk.seg0 + k);
            w += bk.n;
            if (bk.first == 2) {
                packed = true;
                CHECK(mfma, "group %zu block %zu: packed without the MFMA kernels", q, i);
                for (uint32_t k = 0; k < bk.n; ++k) {      // every segment a whole first-segment chunk, in a slot of its own
                    const uint32_t sid = bk.seg0 + k, f = g.segs[sid].chunk;
                    CHECK(g.chunk_seg[f] == sid && g.chunk_seg[f + 1] == sid + 1 && g.seg_first[sid], "group %zu block %zu: segment %u is not a whole chunk", q, i, sid);
                    CHECK(unit_at_seg[sid] != NO_UNIT && l0.vec0[unit_at_seg[sid]] == bk.out_vec0 + k, "group %zu block %zu: slot %u", q, i, k);
                }
            } else {
                CHECK(unit_at_seg[bk.seg0] != NO_UNIT, "group %zu block %zu: not a unit", q, i);
                const uint32_t uid = unit_at_seg[bk.seg0];
                CHECK(bk.n == unit_ns[uid] && bk.out_vec0 == l0.vec0[uid] && bk.first == (g.seg_first[bk.seg0] ? 1u : 0u), "group %zu block %zu", q, i);
            }
        }
        CHECK(w == want.size(), "group %zu: blocks cover %zu of %zu segments", q, w, want.size());
        n_packed += packed;

        // ---- fused tail ----
        bool tail_possible = dec.groups.size() == 1 && mfma && !op_mode && n_chunks > 0;
        for (int f = 0; f < n_chunks && tail_possible; ++f) {
            const uint32_t nu = l0.chunk_seg[f + 1] - l0.chunk_seg[f];
            tail_possible = nu > 0 && nu <= slots;
        }
        if (gg.tails.empty()) {
            if (tail_possible) { CHECK(packed, "group %zu: no fused tail although nothing is packed", q); ++n_tail_withdrawn; }
        } else {
            ++n_tail;
            CHECK(tail_possible && gg.tails.size() == gg.blocks.size() && !packed, "group %zu: fused tail", q);
            uint32_t most = 0;
            for (size_t i = 0; i < gg.tails.size(); ++i) {
                const Z2Tail &t = gg.tails[i];
                CHECK((int)t.chunk < n_chunks && t.pad == 0, "tail %zu", i);
                const uint32_t nu = l0.chunk_seg[t.chunk + 1] - l0.chunk_seg[t.chunk];
                CHECK(t.n_units == nu && nu <= slots && t.unit < nu && unit_seg0[l0.chunk_seg[t.chunk] + t.unit] == gg.blocks[i].seg0, "tail %zu: chunk %u unit %u of %u", i, t.chunk, t.unit, t.n_units);
                most = std::max(most, nu);
            }
            CHECK(gg.tail_stride == (int)most, "tail_stride %d", gg.tail_stride);
        }
    }
    CHECK(next_vec == g.vecs.size(), "the groups hold %u of %zu vectors", next_vec, g.vecs.size());

    // ---- hierarchy ----
    uint64_t steps = 0;
    for (size_t l = 1; l < g.levels.size(); ++l) {
        const HostLevel &prev = g.levels[l - 1], &cur = g.levels[l];
        CHECK((int)cur.chunk_seg.size() == n_chunks + 1 && cur.chunk_seg[0] == 0 && cur.chunk_seg[n_chunks] == cur.vec0.size() && cur.first.size() == cur.vec0.size(), "level %zu", l);
        uint32_t kmax = 0, longest = 0, out = 0;
        size_t ci = 0;
        for (int f = 0; f < n_chunks; ++f) {
            const uint32_t s0 = prev.chunk_seg[f], s1 = prev.chunk_seg[f + 1];
            kmax = std::max(kmax, s1 - s0);
            uint32_t at = s0;
            CHECK(cur.chunk_seg[f] <= cur.chunk_seg[f + 1], "level %zu chunk %d", l, f);
            for (uint32_t uu = cur.chunk_seg[f]; uu < cur.chunk_seg[f + 1]; ++uu) {
                CHECK(ci < cur.chains.size(), "level %zu unit %u: no chain", l, uu);
                const uint32_t rb = cur.chains[ci].seg_begin, re = cur.chains[ci].seg_end;
                const bool fst = rb == s0 && !op_mode;
                CHECK(rb == at && re > rb && re <= s1 && (cur.first[uu] != 0) == fst && cur.vec0[uu] == out, "level %zu chunk %d: run [%u, %u)", l, f, rb, re);
                const uint32_t nvv = fst ? 1u : (uint32_t)N, op0 = rb + (fst ? 1u : 0u);
                CHECK(ci + nvv <= cur.chains.size(), "level %zu unit %u: chains", l, uu);
                for (uint32_t c = 0; c < nvv; ++c) {
                    const ChainDesc &cd = cur.chains[ci + c];
                    CHECK(cd.seg_begin == rb && cd.seg_end == re && cd.c == c && cd.out_vec == out + c && cd.first == (fst ? 1u : 0u), "level %zu chain %zu", l, ci + c);
                    CHECK(cd.vec_first == (fst ? prev.vec0[rb] : 0u) && cd.vbase == (op0 < re ? prev.vec0[op0] : 0u), "level %zu chain %zu: vec_first %u vbase %u", l, ci + c, cd.vec_first, cd.vbase);
                    if (l + 1 < g.levels.size() || !g.finish_fused) CHECK(cd.chunk1 == 0, "level %zu chain %zu: chunk1 %u", l, ci + c, cd.chunk1);
                }
                ci += nvv; out += nvv; at = re;
                longest = std::max(longest, re - rb);
            }
            CHECK(at == s1, "level %zu chunk %d: runs cover %u of [%u, %u)", l, f, at, s0, s1);
        }
        CHECK(ci == cur.chains.size() && out == cur.n_vecs, "level %zu: %zu chains, %u vectors", l, ci, out);
        const uint32_t gsz = kmax <= 16 ? kmax : std::max<uint32_t>(12, (uint32_t)std::ceil(std::cbrt((double)kmax)));
        CHECK(longest == gsz, "level %zu: longest run %u, %u units at most per chunk", l, longest, kmax);
        steps += gsz;
    }
    CHECK(g.chain_steps == steps, "chain_steps %llu", (unsigned long long)g.chain_steps);
    n_deep += g.levels.size() >= 3;
    const HostLevel &last = g.levels.back();
    CHECK((int)g.final_vec.size() == std::max(n_chunks, 1), "final_vec");
    if (!n_chunks) CHECK(g.final_vec[0] == -1, "final_vec");
    bool none_empty = true;
    for (int f = 0; f < n_chunks; ++f) {
        const uint32_t nu = last.chunk_seg[f + 1] - last.chunk_seg[f];
        CHECK(nu <= 1 && (nu == 1) == (length_of(f) > 0), "chunk %d: %u units at the last level", f, nu);
        CHECK(g.final_vec[f] == (nu ? (int32_t)last.vec0[last.chunk_seg[f]] : -1), "chunk %d: final_vec %d", f, g.final_vec[f]);
        none_empty = none_empty && nu == 1;
    }
    // ---- finish_fused ----
    std::vector<int> has((size_t)n_chunks, 0);
    for (const ChainDesc &cd : last.chains)
        if (cd.chunk1) {
            CHECK(cd.first && (int)cd.chunk1 <= n_chunks && g.final_vec[cd.chunk1 - 1] == (int32_t)cd.out_vec, "chunk1 %u", cd.chunk1);
            has[cd.chunk1 - 1]++;
        }
    bool all_have = n_chunks > 0;
    for (int f = 0; f < n_chunks; ++f) all_have = all_have && has[f] == 1;
    CHECK(g.finish_fused == (!op_mode && g.levels.size() > 1 && none_empty && all_have), "finish_fused %d", (int)g.finish_fused);
    CHECK(g.finish_fused == (!op_mode && g.levels.size() > 1 && none_empty && n_chunks > 0), "finish_fused %d although every chunk ends in a first chain", (int)g.finish_fused);
    n_ff[g.finish_fused]++;

    // ---- determinism ----
    if (chunks.size() < 100) CHECK(same_geometry(g, plan_geometry(dec, chunks, kc, N, S, op_mode, mfma)), "the same input gave another geometry");
    return 0;
}

// A group's schedules are the functions checked above, called with the group's own lists: the sizes that the upload
// relies on.
static int check_schedules(const imc::PlanOptions &opt, const imc::KernelFacts &kc, bool wide, const imc::PlanDecision &dec,
                           const std::vector<imc::ChunkFacts> &chunks, const imc::TrainedDict *dict, int N, int S, int B, bool op_mode, bool mfma)
{
    using namespace imc;
    const PlanGeometry g = plan_geometry(dec, chunks, kc, N, S, op_mode, mfma);
    for (size_t q = 0; q < dec.groups.size(); ++q) {
        const GroupDecision &gr = dec.groups[q];
        const GroupGeometry &gg = g.groups[q];
        const GroupSchedules s = group_schedules(opt, kc, wide, gr, g, gg, chunks, gr.dict >= 0 ? dict : nullptr, S, B);
        size_t n_first = 0;
        for (uint32_t id : gg.seg_ids) n_first += g.seg_first[id];
        CHECK(s.big_blocks.size() == (is_chain(gr.kind) ? n_first + (gg.seg_ids.size() - n_first) * kc.big_nslab : 0), "group %zu: %zu workgroups", q, s.big_blocks.size());
        CHECK(s.tail_blocks.size() == (gr.rank1 ? gg.seg_ids.size() : 0) && s.r1_segs.size() == (gr.rank1 ? gg.seg_ids.size() - n_first : 0), "group %zu: hand-off lists", q);
        for (const auto &sl : s.r1_segs) CHECK(!g.seg_first[sl.first] && sl.second == g.segs[sl.first].len, "group %zu: hand-off segment %u", q, sl.first);
        CHECK((int)s.hot.size() == s.n_hot && (gr.kind == GroupKind::BlockedGlobal || (s.n_hot == 0 && !s.stream_table)) && !(s.stream_table && s.n_hot), "group %zu: hot set", q);
        std::set<int> hot(s.hot.begin(), s.hot.end());
        CHECK((int)hot.size() == s.n_hot && (hot.empty() || *hot.rbegin() < gr.A), "group %zu: hot set", q);
        if (gr.kind == GroupKind::BlockedGlobal) {
            const PhaseTable t = xcd_phases(B, (int)gg.blocks.size());
            CHECK(s.phases.grid == t.grid && s.phases.n_phases == t.n_phases, "group %zu: phases", q);
            CHECK(s.tab_desc.size() == s.tab.order.size() && !s.tab2.launches.empty() && !s.tab3.launches.empty(), "group %zu: table schedules", q);
        } else
            CHECK(s.tab_desc.empty() && s.tab2.desc.empty() && s.tab3.desc.empty(), "group %zu: table schedules on kind %d", q, (int)gr.kind);
        CHECK(s.tab.order.size() == (is_blocked(gr.kind) && gr.tokens ? (size_t)(gr.A - S) : 0), "group %zu: depth order", q);
        CHECK(s.table_runs.empty() || (is_chain(gr.kind) && gr.tokens), "group %zu: table runs", q);
    }
    return 0;
}

static int check_geometry_sweep()
{
    using namespace imc;
    std::mt19937 rng(11);
    const int S = 3;
    const std::unique_ptr<HostDict> hd = train(rng, S);
    CHECK(hd->dict.alphabet > 1000, "dictionary too small: %d tokens", hd->dict.alphabet);
    std::vector<std::unique_ptr<HostChunk>> store;
    auto chunk_set = [&](const std::vector<size_t> &lens) {
        std::vector<ChunkFacts> v;
        for (size_t L : lens) { store.push_back(make_chunk(rng, L, S, hd.get(), 0)); v.push_back(store.back()->facts); }
        return v;
    };
    std::vector<size_t> mixed(61, 6000);
    mixed[0] = 200000;
    // one long chunk; an empty chunk; chunks shorter than one segment (too short for a dictionary, too); many one-segment
    // chunks; one long chunk beside many short ones; no chunk at all
    const std::vector<std::vector<ChunkFacts>> sets = {chunk_set({200000}), chunk_set({70001, 0, 4099}), chunk_set({100, 37, 5000, 1, 15}),
                                                       chunk_set(std::vector<size_t>(70, 5000)), chunk_set(mixed), chunk_set({})};
    const std::vector<DictFacts> dicts = {DictFacts{&hd->depth}};
    const int pairs[6][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {0, 1}, {0, 2}};   // imc_set_compression(0, 1, 2, 3, 4, 5)
    long idx = 0;
    for (int N : {4, 10, 20, 24, 28, 32, 48, 100, 150})
        for (int B : {1, 3, 9})
            for (size_t cs = 0; cs < sets.size(); ++cs)
                for (const int *pr : pairs)
                    // the planner's own length; 16 (more than 144 units in the long chunks: three levels and more); one
                    // longer than the short chunks (whole chunks as single segments)
                    for (size_t seg : {(size_t)0, (size_t)16, (size_t)8192})
                        for (bool op_mode : {false, true}) {
                            ++idx;
                            // a fixed quarter of the cross product; the counters checked at the end say that it still reaches
                            // every case the sweep is there for
                            if ((((unsigned)idx * 2654435761u) >> 16) % 4) continue;
                            PlanOptions opt;
                            opt.compression = pr[0]; opt.kernel_pref = pr[1]; opt.seg_override = seg;
                            g_mode = (int)(idx % N_MODES);
                            opt.blocked_variant = (const int[]){4, 3, 5, 2, 4, 4, 4}[idx % 7];
                            opt.z4_stream = (const int[]){-1, -1, 0, 1}[idx % 4];
                            opt.rank1_handoff = idx % 9 != 0;
                            const std::vector<ChunkFacts> &chunks = sets[cs];
                            const KernelFacts *kc = choose(N, prefer_gemm(opt, chunks, N, S));
                            CHECK(kc, "no entry for %d states", N);
                            g_np = kc->NP;
                            const PlanDecision d = decide_groups(opt, *kc, false, chunks, dicts, N, S, B, op_mode);
                            const bool mfma = kc->use3(opt.blocked_variant);
                            if (check_geometry(d, chunks, *kc, N, S, op_mode, mfma) || check_schedules(opt, *kc, false, d, chunks, hd.get(), N, S, B, op_mode, mfma)) {
                                std::printf("  (N %d B %d set %zu c %d k %d seg %zu op %d mode %d variant %d)\n", N, B, cs, pr[0], pr[1], seg, (int)op_mode, g_mode, opt.blocked_variant);
                                return 1;
                            }
                            const KernelFacts *kw = (N > 24 && N <= 32) ? choose(N, false) : nullptr;
                            if (kw && kw->wide_blocked && opt.compression == 1 && opt.kernel_pref == 0 && !chunks.empty()) {   // the wide scan's plan
                                g_np = kw->NP;
                                const PlanDecision wd = decide_groups(opt, *kw, true, chunks, dicts, N, S, B, op_mode);
                                if (check_geometry(wd, chunks, *kw, N, S, op_mode, true) || check_schedules(opt, *kw, true, wd, chunks, hd.get(), N, S, B, op_mode, true)) {
                                    std::printf("  (wide: N %d B %d set %zu seg %zu op %d mode %d)\n", N, B, cs, seg, (int)op_mode, g_mode);
                                    return 1;
                                }
                            }
                        }
    CHECK(n_packed > 0 && n_tail > 0 && n_tail_withdrawn > 0 && n_ff[0] > 0 && n_ff[1] > 0 && n_empty_chunk > 0 && n_op_mode > 0 && n_deep > 0,
          "the sweep misses a case: packed %ld, fused tail %ld, withdrawn %ld, finish_fused %ld / %ld, empty chunk %ld, op_mode %ld, three levels %ld",
          n_packed, n_tail, n_tail_withdrawn, n_ff[1], n_ff[0], n_empty_chunk, n_op_mode, n_deep);
    for (int k = 0; k < 6; ++k) CHECK(n_geo_kind[k] > 0, "kind %d never planned", k);
    return 0;
}

int main()
{
    std::mt19937 rng(7);
    for (int S : {2, 3, 4})
        for (size_t L : {(size_t)3000, (size_t)200000, (size_t)3000000}) {
            std::vector<uint8_t> obs(L);
            uint8_t cur = 0;
            for (auto &x : obs) { if (rng() % 100 >= 96) cur = (uint8_t)(rng() % S); x = cur; }   // sticky
            imc::PairDict d;
            imc::train_dict(d, S, std::vector<uint8_t>(obs.begin() + 1, obs.end()), 4);
            if (d.alphabet >= imc::kByteAlphabet) {
                const std::vector<uint8_t> b = imc::encode_bytes(d, obs.data(), L, nullptr);
                imc::train_dict_wide(d, std::vector<imc::tok_t>(b.begin() + 1, b.end()), 3);
            }
            std::vector<std::string> exp((size_t)d.alphabet);
            for (int z = 0; z < d.alphabet; ++z) exp[z] = z < S ? std::string(1, (char)('a' + z)) : exp[d.left[z]] + exp[d.right[z]];
            std::set<int> sizes = {S, S + 1, S + 2, 8, 44, 256, 257, 1000, 4096, d.alphabet};
            for (int A : sizes)
                if (A >= S && A <= d.alphabet)
                    if (check_dictionary(d, A, exp)) { std::printf("  (S %d, L %zu, A %d of %d)\n", S, L, A, d.alphabet); return 1; }
        }
    if (max_tokens <= 1000 || max_depth_seen < 6) { std::printf("dictionaries too small: %d tokens, depth %d\n", max_tokens, max_depth_seen); return 1; }
    if (check_hot_order(rng) || check_dealing(rng) || check_phases() || check_geometry_sweep()) return 1;
    std::printf("plan_host ok: %d (dictionary, alphabet) cases, up to %d tokens and depth %d; %ld geometries: %ld with a packed block, %ld with the fused tail, "
                "%ld with it withdrawn for packed blocks, finish_fused %ld true / %ld false, %ld with an empty chunk, %ld in operator mode, %ld of three or more "
                "levels; groups by kind %ld %ld %ld %ld %ld %ld\n",
                n_cases, max_tokens, max_depth_seen, n_geo, n_packed, n_tail, n_tail_withdrawn, n_ff[1], n_ff[0], n_empty_chunk, n_op_mode, n_deep,
                n_geo_kind[0], n_geo_kind[1], n_geo_kind[2], n_geo_kind[3], n_geo_kind[4], n_geo_kind[5]);
    return 0;
}
