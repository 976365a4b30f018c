#include "plan_check_common.hpp"
#include <cstdio>
#include <string>
// The planner's decisions (planner_host.hpp) on the CPU: chunk facts come from dictionaries trained on sticky random
// streams and from encode_levels(), exactly as the library installs them; the kernel table is a stand-in with the shapes
// of the real one and small LDS size functions (plan_check_common.hpp), because the properties below do not depend on
// the real sizes.  Built with -fsanitize=address,undefined.
//
// Two properties are asserted as the code has them, not as first stated for this check:
//  - chain slot target: a group with the rank-one hand-off cuts its segments m <= 6 times shorter (m rounds of heads), so
//    the sum of ceil(L / seglen) is bounded by 6 x the target there, and by the target itself everywhere else;
//  - "does not fit LDS": such a level is BlockedGlobal when the plan's blocked kernels are the MFMA ones and the vector
//    family is not pinned; otherwise the level is not taken by a blocked kernel at all (never BlockedLds).

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

// ---- the properties ----
static long n_decisions = 0, n_kind[6], n_rank1 = 0, n_forced = 0, n_slot = 0;

static bool same(const PlanDecision &a, const PlanDecision &b, const std::vector<int> &dict_map)
{
    if (a.chunk_group != b.chunk_group || a.wide_ok != b.wide_ok || a.groups.size() != b.groups.size()) return false;
    for (size_t q = 0; q < a.groups.size(); ++q) {
        const GroupDecision &x = a.groups[q], &y = b.groups[q];
        if (x.tokens != y.tokens || x.level != y.level || x.A != y.A || (x.dict < 0 ? -1 : dict_map[x.dict]) != y.dict ||
            x.chunks != y.chunks || x.kind != y.kind || x.seglen != y.seglen || x.wide_tokens != y.wide_tokens || x.rank1 != y.rank1 ||
            x.checkpoints != y.checkpoints || x.model_us != y.model_us || x.model_tab_us != y.model_tab_us) return false;
    }
    return true;
}

static size_t stream_len(const ChunkFacts &c, const GroupDecision &gr) { return gr.tokens ? c.level[gr.level].ntok : c.L; }

static int check_decision(const PlanDecision &d, const PlanOptions &opt, const KernelFacts &kc, bool wide,
                          const std::vector<ChunkFacts> &chunks, int S, int B, bool op_mode)
{
    ++n_decisions;
    // grouping
    CHECK(d.chunk_group.size() == chunks.size(), "size");
    std::vector<int> seen(chunks.size(), 0);
    for (size_t q = 0; q < d.groups.size(); ++q) {
        const GroupDecision &gr = d.groups[q];
        CHECK(!gr.chunks.empty(), "group %zu is empty", q);
        for (int f : gr.chunks) {
            CHECK(f >= 0 && f < (int)chunks.size() && !seen[f]++ && d.chunk_group[f] == (int)q, "group %zu chunk %d", q, f);
            if (gr.tokens) {
                CHECK(chunks[f].dict == gr.dict && gr.dict >= 0, "group %zu chunk %d: dictionary", q, f);
                CHECK(gr.level >= 0 && gr.level < kNumLevels && chunks[f].level[gr.level].stream, "group %zu chunk %d: no stream at level %d", q, f, gr.level);
                CHECK(gr.A == chunks[f].level[gr.level].alphabet && gr.A > chunks[f].nsym, "group %zu chunk %d: alphabet %d", q, f, gr.A);
            }
        }
        if (!gr.tokens) CHECK(gr.A == S && gr.dict < 0 && gr.level < 0, "group %zu: A %d", q, gr.A);
    }
    for (size_t f = 0; f < chunks.size(); ++f) CHECK(seen[f] == 1, "chunk %zu in %d groups", f, seen[f]);

    const bool mfma_blocked = kc.R != 0 && (kc.use3(opt.blocked_variant) || wide) && opt.kernel_pref != 1;
    for (size_t q = 0; q < d.groups.size(); ++q) {
        const GroupDecision &gr = d.groups[q];
        const bool chain = gr.kind == GroupKind::GemmChain || gr.kind == GroupKind::MatVecChain;
        const bool blocked = gr.kind == GroupKind::BlockedLds || gr.kind == GroupKind::BlockedGlobal;
        n_kind[(int)gr.kind]++;
        // kind against gates
        CHECK(chain == (kc.R == 0), "group %zu: kind %d on entry R %d", q, (int)gr.kind, kc.R);
        if (opt.kernel_pref == 1) CHECK(!blocked, "group %zu: blocked kind with the vector family pinned", q);
        if (gr.kind == GroupKind::TokenVector || gr.kind == GroupKind::BlockedGlobal) CHECK(gr.tokens, "group %zu: kind %d on raw columns", q, (int)gr.kind);
        if (gr.kind == GroupKind::ColumnVector) CHECK(!gr.tokens, "group %zu", q);
        if (g_mode == BLOCKED_NEVER && !chain) {
            CHECK(gr.kind != GroupKind::BlockedLds, "group %zu: BlockedLds although nothing fits", q);
            if (gr.tokens && mfma_blocked) CHECK(gr.kind == GroupKind::BlockedGlobal, "group %zu: kind %d", q, (int)gr.kind);
        }
        size_t lmax = 0, total = 0, nonempty = 0;
        for (int f : gr.chunks) { const size_t L = stream_len(chunks[f], gr); lmax = std::max(lmax, L); total += L; nonempty += L > 0; }
        if (gr.kind == GroupKind::MatVecChain) CHECK(lmax <= gr.seglen && !op_mode, "group %zu: mat-vec chain, longest %zu, segment %zu", q, lmax, gr.seglen);
        // segment length
        CHECK(gr.seglen >= 16 && gr.seglen % (blocked ? Z2GRAN : 16) == 0, "group %zu: segment length %zu", q, gr.seglen);
        if (opt.seg_override) CHECK(gr.seglen == round_up(std::max<size_t>(opt.seg_override, 16), 16), "group %zu: segment length %zu", q, gr.seglen);
        // chain slot target
        if (chain && !opt.seg_override) {
            const size_t per_cu = std::max<size_t>(1, std::min<size_t>(LDS_BUDGET / kc.big_lds, (size_t)32 / (size_t)kc.G));
            const size_t target = std::max<size_t>(1, (size_t)opt.cus * per_cu / ((size_t)B * kc.big_nslab));
            if (nonempty <= target && gr.kind == GroupKind::GemmChain) {
                size_t count = 0;
                for (int f : gr.chunks) count += (stream_len(chunks[f], gr) + gr.seglen - 1) / gr.seglen;
                CHECK(count <= (gr.rank1 ? 6 : 1) * target, "group %zu: %zu segments of %zu for %zu slots (rank1 %d)", q, count, gr.seglen, target, (int)gr.rank1);
                ++n_slot;
            }
        }
        // rank-one checkpoints
        if (gr.rank1) {
            ++n_rank1;
            CHECK(gr.kind == GroupKind::GemmChain && opt.rank1_handoff, "group %zu: hand-off on kind %d", q, (int)gr.kind);
            CHECK(!gr.checkpoints.empty() && (int)gr.checkpoints.size() <= R1_MAX_ROUNDS, "group %zu: %zu checkpoints", q, gr.checkpoints.size());
            for (size_t k = 0; k < gr.checkpoints.size(); ++k)
                CHECK(gr.checkpoints[k] > 0 && gr.checkpoints[k] % 16 == 0 && (!k || gr.checkpoints[k] > gr.checkpoints[k - 1]), "group %zu: checkpoint %zu", q, k);
            CHECK((size_t)gr.checkpoints.back() + gr.seglen / 8 < gr.seglen, "group %zu: last checkpoint %d of %zu", q, gr.checkpoints.back(), gr.seglen);
        } else
            CHECK(gr.checkpoints.empty(), "group %zu: checkpoints without the hand-off", q);
    }
    return 0;
}

// the forced level's eligibility, restated from assign_groups (the first chunk of the dictionary decides)
static bool force_eligible(int l, const ChunkFacts &o0, const PlanOptions &opt, const KernelFacts &kc, bool wide)
{
    const bool big = kc.R == 0, mfma_blocked = !big && (kc.use3(opt.blocked_variant) || wide) && opt.kernel_pref != 1;
    int a_max = 0;
    if (big) a_max = kMaxAlphabet;
    else
        for (int A = 1; A <= kByteAlphabet; ++A)
            if (zip_lds(A) <= LDS_BUDGET || (kc.has_zip2 && opt.kernel_pref != 1 && kc.blocked_lds(A, opt.blocked_variant) <= LDS_BUDGET)) a_max = A;
    if (l < 0 || l >= kNumLevels) return false;
    const ChunkFacts::Level &lv = o0.level[l];
    const bool hybrid = mfma_blocked && (wide || (kc.has_zip4 && opt.blocked_variant >= 4)) && !o0.wide_raw;
    if (!(lv.alphabet <= (hybrid ? HYBRID_MAX_ALPHABET : a_max) && lv.alphabet > o0.nsym && lv.stream)) return false;
    if (hybrid && (wide || kc.blocked_lds(lv.alphabet, opt.blocked_variant) > LDS_BUDGET) && kc.zip4_lds(lv.alphabet, 0) > LDS_BUDGET) return false;
    return hybrid ? !lv.counts().empty() : !lv.wide;
}

static int check_call(const PlanOptions &opt, const KernelFacts &kc, bool wide, const std::vector<ChunkFacts> &chunks,
                      const std::vector<DictFacts> &dicts, int N, int S, int B, bool op_mode, bool with_forced, PlanDecision *out)
{
    g_np = kc.NP;
    const PlanDecision d = decide_groups(opt, kc, wide, chunks, dicts, N, S, B, op_mode);
    if (check_decision(d, opt, kc, wide, chunks, S, B, op_mode)) return 1;
    std::vector<int> identity(dicts.size());
    for (size_t k = 0; k < identity.size(); ++k) identity[k] = (int)k;
    if (chunks.size() < 100) CHECK(same(d, decide_groups(opt, kc, wide, chunks, dicts, N, S, B, op_mode), identity), "the same facts gave another decision");
    if (with_forced && opt.compression)
        for (int l : {0, 3, 7, 10, 12, 15, 18, kNumLevels - 1, kNumLevels}) {
            PlanOptions fo = opt;
            fo.force_level = l;
            const PlanDecision fd = decide_groups(fo, kc, wide, chunks, dicts, N, S, B, op_mode);
            if (check_decision(fd, fo, kc, wide, chunks, S, B, op_mode)) return 1;
            bool any = false;
            std::vector<int> first(dicts.size(), -1);
            for (size_t f = 0; f < chunks.size(); ++f)
                if (chunks[f].dict >= 0 && chunks[f].nsym == S && first[chunks[f].dict] < 0) first[chunks[f].dict] = (int)f;
            for (size_t di = 0; di < dicts.size(); ++di) {
                if (first[di] < 0 || !force_eligible(l, chunks[first[di]], opt, kc, wide)) continue;
                any = true;
                for (const GroupDecision &gr : fd.groups)
                    if (gr.dict == (int)di) CHECK(gr.tokens && gr.level == l, "forced level %d, dictionary %zu: level %d", l, di, gr.level);
                ++n_forced;
            }
            if (!any) CHECK(same(d, fd, identity), "forced level %d is not eligible, yet the decision changed", l);
        }
    if (out) *out = d;
    return 0;
}

int main()
{
    std::mt19937 rng(11);
    const int S = 3;
    std::unique_ptr<HostDict> hd[2] = {train(rng, S), train(rng, S)};
    if (hd[0]->dict.alphabet <= 1000) { std::printf("dictionary too small: %d tokens\n", hd[0]->dict.alphabet); return 1; }
    std::vector<std::unique_ptr<HostChunk>> store;
    auto chunk_set = [&](const std::vector<size_t> &lens, bool two_dicts) {
        std::vector<ChunkFacts> v;
        for (size_t k = 0; k < lens.size(); ++k) {
            const int di = two_dicts ? (int)(k % 2) : 0;
            store.push_back(make_chunk(rng, lens[k], S, hd[di].get(), di));
            v.push_back(store.back()->facts);
        }
        return v;
    };
    std::vector<size_t> mixed(501, 6000);
    mixed[0] = 3000000;
    const std::vector<std::vector<ChunkFacts>> sets = {chunk_set({3000000}, false), chunk_set({70001, 0, 4099}, false),
                                                       chunk_set(std::vector<size_t>(40, 5000), false), chunk_set(mixed, false)};
    const std::vector<ChunkFacts> two = chunk_set({300000, 200000, 0, 5000, 100, 41000}, true);
    const std::vector<DictFacts> dicts = {DictFacts{&hd[0]->depth}, DictFacts{&hd[1]->depth}};
    const int pairs[6][2] = {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {0, 1}, {0, 2}};   // imc_set_compression(0, 1, 2, 3, 4, 5)

    long idx = 0;
    for (int N : {4, 10, 20, 24, 28, 32, 48, 100, 150})
        for (int B : {1, 8, 64})
            for (size_t cs = 0; cs < sets.size(); ++cs)
                for (const int *pr : pairs)
                    for (size_t seg : {(size_t)0, (size_t)64})
                        for (bool op_mode : {false, true}) {
                            ++idx;
                            // a fixed quarter of the cross product (an eighth with the 501 chunks); the counters checked at
                            // the end say that it still reaches every kind, gate and property
                            const unsigned pick = ((unsigned)idx * 2654435761u) >> 16;
                            if (pick % (cs == 3 ? 8 : 4)) continue;
                            PlanOptions opt;
                            opt.compression = pr[0]; opt.kernel_pref = pr[1]; opt.seg_override = seg;
                            g_mode = (int)(idx % N_MODES);
                            opt.blocked_variant = (const int[]){4, 3, 5, 2, 4, 4, 4}[idx % 7];
                            opt.z4_stream = (const int[]){-1, -1, 0, 1}[idx % 4];
                            opt.rank1_handoff = idx % 9 != 0;
                            opt.table_pairs = idx % 13 != 0;
                            const std::vector<ChunkFacts> &chunks = sets[cs];
                            const KernelFacts *kc = choose(N, prefer_gemm(opt, chunks, N, S));
                            CHECK(kc, "no entry for %d states", N);
                            if (kc->R == 0 && (kc->G == 7 || kc->G == 9) && next_shape_hands_off(opt, *kc, *(kc + 1), chunks, S, B)) kc = kc + 1;
                            PlanDecision base;
                            const bool forced = cs != 3 && pick % 3 == 0;                 // (the forced levels: nine more calls)
                            if (check_call(opt, *kc, false, chunks, dicts, N, S, B, op_mode, forced, &base)) { std::printf("  (N %d B %d set %zu c %d k %d seg %zu op %d mode %d)\n", N, B, cs, pr[0], pr[1], seg, (int)op_mode, g_mode); return 1; }
                            const KernelFacts *kw = (N > 24 && N <= 32) ? choose(N, false) : nullptr;
                            if (kw && kw->wide_blocked && opt.compression == 1 && opt.kernel_pref == 0) {
                                PlanDecision wd;
                                if (check_call(opt, *kw, true, chunks, dicts, N, S, B, op_mode, forced, &wd)) { std::printf("  (wide: N %d B %d set %zu seg %zu op %d mode %d)\n", N, B, cs, seg, (int)op_mode, g_mode); return 1; }
                                const bool wins = wide_plan_wins(opt, base, kc->R == 0, wd, chunks, N);
                                CHECK(wins == wide_plan_wins(opt, base, kc->R == 0, wd, chunks, N), "comparison");
                                if (wins) {
                                    bool any = false;
                                    for (const GroupDecision &gr : wd.groups) any = any || gr.kind == GroupKind::BlockedGlobal;
                                    CHECK(any && wd.wide_ok, "the blocked scan won without a group");
                                }
                            }
                        }

    // "129 segments for 128 slots": 150 states (NP = 160, two slabs), three raw chunks of 3e6 columns, one set, 256 CUs
    for (bool handoff : {false, true}) {
        PlanOptions opt;
        opt.rank1_handoff = handoff;
        std::vector<ChunkFacts> raw(3);
        for (ChunkFacts &c : raw) { c.L = 3000000; c.nsym = S; for (auto &lv : c.level) lv.alphabet = S; }
        const KernelFacts *kc = choose(150, prefer_gemm(opt, raw, 150, S));
        CHECK(kc && kc->NP == 160 && kc->big_nslab == 2, "entry");
        PlanDecision d;
        const long before = n_slot;
        if (check_call(opt, *kc, false, raw, {}, 150, S, 1, false, false, &d)) return 1;
        CHECK(n_slot == before + 1 && d.groups.size() == 1 && d.groups[0].kind == GroupKind::GemmChain, "not a GEMM-chain group with a slot target");
        if (!handoff) CHECK(3 * ((3000000 + d.groups[0].seglen - 1) / d.groups[0].seglen) <= 128, "segment length %zu", d.groups[0].seglen);
    }

    // dictionary numbering: the same call with the two dictionaries' indices exchanged
    for (int N : {10, 20, 32, 100})
        for (int B : {1, 8}) {
            PlanOptions opt;
            g_mode = AFFINE;
            std::vector<ChunkFacts> swapped(two);
            for (ChunkFacts &c : swapped) if (c.dict >= 0) c.dict ^= 1;
            const KernelFacts *kc = choose(N, prefer_gemm(opt, two, N, S));
            PlanDecision a, b;
            if (check_call(opt, *kc, false, two, dicts, N, S, B, false, true, &a)) return 1;
            if (check_call(opt, *kc, false, swapped, {dicts[1], dicts[0]}, N, S, B, false, false, &b)) return 1;
            CHECK(same(a, b, {1, 0}), "N %d B %d: the decision depends on the dictionaries' numbering", N, B);
            int token_groups = 0;
            for (const GroupDecision &gr : a.groups) token_groups += gr.tokens;
            CHECK(token_groups == 2, "N %d B %d: %d token groups for two dictionaries", N, B, token_groups);
        }

    for (int w = 0; w < 5; ++w) CHECK(gate_hits[w][0] > 0 && gate_hits[w][1] > 0, "size function %d was not driven both ways (%ld / %ld)", w, gate_hits[w][0], gate_hits[w][1]);
    for (int k = 0; k < 6; ++k) CHECK(n_kind[k] > 0, "kind %d never decided", k);
    CHECK(n_rank1 > 0 && n_forced > 0 && n_slot > 0, "hand-off %ld, forced levels %ld, slot targets %ld", n_rank1, n_forced, n_slot);
    std::printf("planner_host ok: %ld decisions; groups by kind %ld %ld %ld %ld %ld %ld; %ld with the hand-off, %ld forced levels honoured, %ld slot targets\n",
                n_decisions, n_kind[0], n_kind[1], n_kind[2], n_kind[3], n_kind[4], n_kind[5], n_rank1, n_forced, n_slot);
    return 0;
}
