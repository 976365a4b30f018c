#include "../imcoalhmm_amd/csrc/pair_dict.hpp"
#include "../imcoalhmm_amd/csrc/plan_host.hpp"
#include <cstdio>
#include <random>
#include <set>
#include <string>
// The launch schedules of plan_host.hpp on trained dictionaries, checked against what the kernels that run from them
// need: every table entry is built exactly once, from operands that are raw symbols or were finished by an EARLIER
// launch, and the product it describes is the token's own (the expansion of a token is the string of raw symbols
// obtained by recursive left + right).  Built with -fsanitize=address,undefined.

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

struct Block { uint32_t seg, slab, out_vec0, pad; };

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
            const std::vector<Block> wg = imc::deal_slabs<Block>(seg_ids, seg_out, seg_first, nslab);
            std::set<std::pair<uint32_t, uint32_t>> want, got;
            size_t n_first = 0;
            for (uint32_t id : seg_ids) {
                n_first += seg_first[id];
                for (int sl = 0; sl < (seg_first[id] ? 1 : nslab); ++sl) want.insert({id, (uint32_t)sl});
            }
            for (const Block &b : wg) {
                CHECK(got.insert({b.seg, b.slab}).second && b.out_vec0 == 1000 + 3 * b.seg && b.pad == 0, "segment %u slab %u", b.seg, b.slab);
            }
            CHECK(got == want, "not a permutation of the (segment, slab) pairs");
            const size_t n_rest = wg.size() - n_first;
            for (size_t k = 0; k < wg.size(); ++k) CHECK((seg_first[wg[k].seg] != 0) == (k >= n_rest), "first segments come last (%zu)", k);
            for (size_t base = 0; base + 8 * (size_t)nslab <= n_rest; base += 8 * (size_t)nslab)         // full tiles
                for (size_t k = 0; k < 8; ++k)
                    for (int sl = 0; sl < nslab; ++sl)
                        CHECK(wg[base + 8 * sl + k].seg == wg[base + k].seg && wg[base + 8 * sl + k].slab == (uint32_t)sl, "tile at %zu", base);
            const std::vector<Block> tails = imc::tail_list<Block>(seg_ids, seg_out);
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
    if (check_hot_order(rng) || check_dealing(rng) || check_phases()) return 1;
    std::printf("plan_host ok: %d (dictionary, alphabet) cases, up to %d tokens and depth %d\n", n_cases, max_tokens, max_depth_seen);
    return 0;
}
