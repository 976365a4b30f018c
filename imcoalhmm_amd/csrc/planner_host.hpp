// planner_host.hpp - host-only decisions of the launch planner: which dictionary level a dictionary's chunks run on, the
// launch groups and the kernel family of each, the segment length, the rank-one checkpoints, and the comparisons between
// kernel entries that build_plan makes.  Everything here is a pure function of plain facts (PlanOptions, KernelFacts,
// ChunkFacts, DictFacts): no HIP and no device pointers.  imcoal_fwd.hip gathers the facts from its chunk handles,
// plan_host.hpp turns a PlanDecision into launch descriptors; tests/planner_host_check.cpp asks the same functions on
// the CPU under ASan/UBSan.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "options_host.hpp"
#include "pair_dict.hpp"

namespace imc {

// k_zpropagate4 caches nothing in LDS while the operator tables of one launch (all parameter sets) fit this many bytes -
// they then stay in L2 / the Infinity Cache and a step's operands arrive from there a step ahead (IMC_Z4_STREAM=0/1
// forces the hybrid / the streamed form).  With more than one parameter set and the XCD-affine grid the streamed form is
// used whatever the total (z4_streamed).
constexpr double Z4_STREAM_MAX_BYTES = 32.0e6;
constexpr size_t LDS_BUDGET = 160 * 1024 - 1024;   // bytes of LDS a compressed-path workgroup may use
constexpr size_t CTAB_BUDGET = (size_t)24 << 30;   // largest operator table (all parameter sets) a plan may allocate
#ifndef IMC_HYBRID_MAX_ALPHABET
#define IMC_HYBRID_MAX_ALPHABET 4096
#endif
// hybrid table (k_zpropagate4): largest dictionary level considered.  Measured at N = 20 on the bench alignment: 1024 tokens
// (3.3 MB of operators, resident in every XCD's 4 MB L2) 0.360 ms per evaluation, 1536: 0.347, 4096 (13 MB, Infinity
// Cache): 0.342 - the columns per token saturate (133 / 139 / 150) while a cold step gets dearer
constexpr int HYBRID_MAX_ALPHABET = IMC_HYBRID_MAX_ALPHABET;
constexpr size_t Z2GRAN = 4;                       // blocked kernels: segment lengths are multiples of this many tokens
constexpr size_t R1_MIN_SEGLEN = 1024;             // rank-one hand-off: segments at least this long (stream elements) ...
constexpr size_t R1_MIN_HEAD = 256;                // ... run at least this many on the GEMM chain before the test
constexpr double R1_HEAD_COLUMNS = 65536.0;        // planner's estimate of the columns a head needs before it collapses
constexpr double R1_HEAD_MIN_COLUMNS = 8192.0;     // first checkpoint of the hand-off test, in alignment columns
constexpr int R1_MAX_ROUNDS = 24;                  // checkpoints per evaluation
constexpr double R1_DENSE_COLUMNS = 1.0e5;         // ... spaced 1.125x up to this many alignment columns, 1.5x beyond

// Which kernel family runs a launch group: fixed once, at the end of decide_groups(); everything after that point reads
// the kind or one of Group's predicates.  enqueue() has one case per kind.
enum class GroupKind {
    ColumnVector,    // k_propagate: one step per alignment column
    TokenVector,     // k_zpropagate: one step per token, operator table in LDS
    BlockedLds,      // register-blocked scan (one 16-lane row per segment), table in LDS: k_zpropagate3 / k_zpropagate2
    BlockedGlobal,   // ... fp64-MFMA scan on the global (hybrid or streamed) table: k_zpropagate4, alphabets beyond LDS
    GemmChain,       // large-N GEMM chain (one workgroup per segment and column slab): k_big_propagate
    MatVecChain,     // ... every chunk is one segment: mat-vec chain (k_big_vector), no operators
};
inline bool is_chain(GroupKind k) { return k == GroupKind::GemmChain || k == GroupKind::MatVecChain; }
inline bool is_blocked(GroupKind k) { return k == GroupKind::BlockedLds || k == GroupKind::BlockedGlobal; }

// What the planner reads: the options record (options_host.hpp; the planner's own fields are its first group), the
// device's size and the per-call variables; build_plan fills one per call and the plan keeps it.
struct PlanOptions : Options {
    int cus = 256;
    int force_level = -1;              // IMC_FORCE_LEVEL (experiments only: pin the dictionary level index), -1 when none
    bool debug = false;                // IMC_DEBUG: the estimates of the families considered, on stderr
    bool debug_levels = false;         // IMC_DEBUG_LEVELS: ... of every dictionary level considered
};

// The numbers and size functions of one kernel-table entry (KernelChoice adds the kernels' addresses).
struct KernelFacts {
    int R = 0, G = 0, NP = 0, VPW = 0, minw = 1;   // R == 0: large-N GEMM-chain path (kernels_big.hpp), NP = 16 * G
    int zwaves = 0;                    // wavefronts per workgroup of the token vector kernel (k_zpropagate)
    int big_nslab = 0;
    size_t big_lds = 0;
    int tok_doubles = 0;               // doubles per table entry of the MFMA kernels
    int z4_waves = 8;                  // wavefronts per workgroup of the blocked scan (Zip4Shape); segments per workgroup = 4 x
    bool wide_blocked = false;         // 25-32 states: of the blocked family only the streamed scan and the one-depth table build exist
    // which kernels the entry has: the register-blocked token kernel (NP = 4 RB <= 24), its fp64-MFMA form, that with the
    // hybrid LDS / L2 table, with the streamed table, and the two-depths-per-launch table build
    bool has_zip2 = false, has_zip3 = false, has_zip4 = false, has_zip4s = false, has_level2 = false;
    // LDS needs by alphabet (the kernel headers keep the geometry; the CPU check puts stand-ins here)
    size_t (*zip_lds)(int) = nullptr;
    size_t (*zip2_lds)(int) = nullptr;
    size_t (*zip3_lds)(int) = nullptr;
    size_t (*zip4_lds)(int, int) = nullptr;
    int (*zip4_max_hot)(int, size_t) = nullptr;
    int z4_slots() const { return z4_waves * 4; }
    // the blocked kernel in use (PlanOptions::blocked_variant) and its LDS need for an alphabet of A tokens
    bool use3(int blocked_variant) const { return has_zip3 && blocked_variant >= 3; }
    size_t blocked_lds(int A, int blocked_variant) const { return use3(blocked_variant) ? zip3_lds(A) : zip2_lds(A); }
};

struct ChunkFacts {
    size_t L = 0;
    int nsym = 0;
    bool wide_raw = false;             // raw alphabet beyond 256 symbols
    int dict = -1;                     // index into the call's DictFacts, -1: not compressed
    struct Level {
        bool stream = false;           // the chunk has a token stream of this level
        bool wide = false;             // ... holding 16-bit ids
        size_t ntok = 0;
        int alphabet = 0;
        const std::vector<uint32_t> *tok_count = nullptr;   // occurrences of every token id (may be empty), never copied
        const std::vector<uint32_t> &counts() const
        {
            static const std::vector<uint32_t> none;
            return tok_count ? *tok_count : none;
        }
    } level[kNumLevels];
};

// Dictionaries are numbered in the order of their first appearance in the chunk list.
struct DictFacts {
    const std::vector<int> *depth = nullptr;   // per token; raw symbols have depth 0
};

struct GroupDecision {     // one propagate launch
    bool tokens = false;   // the group's stream is a token level of its dictionary, not the raw columns (a raw stream can
                           // run the blocked scan and the chains too)
    int level = -1, A = 0;
    int dict = -1;
    std::vector<int> chunks;
    GroupKind kind = GroupKind::ColumnVector;
    size_t seglen = 0;
    bool wide_tokens = false;                    // the token stream holds 16-bit ids
    bool rank1 = false;                          // rank-one hand-off (GEMM chain only) and its checkpoints (token counts)
    std::vector<int> checkpoints;
    double model_us = 0.0, model_tab_us = 0.0;   // the planner's estimate for this group's launches and the table's part of it (dictionary groups; compared by wide_plan_wins)
};

struct PlanDecision {
    std::vector<int> chunk_group;       // chunk -> index into groups
    bool wide_ok = true;                // (wide plans) every dictionary had a level for the blocked scan
    std::vector<GroupDecision> groups;
};


inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// Pick the segment length (in stream elements) that minimises a simple machine model: equal-length
// wavefront tasks run in rounds of `resident` wavefronts at `step_cost` cycles per step; the serial
// stitch adds ~stitch_cost per segment of the longest chunk.
inline size_t choose_seglen(const std::vector<size_t> &lens, int N, int B, int VPW, double resident, double step_cost,
                     double *cost_out = nullptr)
{
    size_t maxlen = 0;
    for (size_t L : lens) maxlen = std::max(maxlen, L);
    if (cost_out) *cost_out = (double)maxlen * step_cost;
    if (maxlen <= 256) return std::max<size_t>(round_up(maxlen, 16), 16);
    const double stitch_cost = 12.0 * N + 300.0;   // cycles per stitched segment
    double best = 1e300;
    size_t best_seg = maxlen;
    for (double s = 128.0;; s *= 1.189207115) {
        const size_t seg = std::min(round_up((size_t)s, 16), round_up(maxlen, 16));
        double vecs = 0.0, kmax = 0.0;
        for (size_t L : lens) {
            if (!L) continue;
            const double K = std::ceil((double)L / (double)seg);
            vecs += 1.0 + (K - 1.0) * N;
            kmax = std::max(kmax, K);
        }
        const double waves = std::ceil(vecs * B / VPW);
        const double rounds = std::ceil(waves / resident);
        const double cost = rounds * (double)seg * step_cost + kmax * stitch_cost;
        if (cost < best) { best = cost; best_seg = seg; }
        if (seg >= maxlen) break;
    }
    if (cost_out) *cost_out = best;
    return best_seg;
}

// Cycles per chain step and CU of the mat-vec chain kernel (k_big_vector): NP^2 doubles streamed per step.
// Measured at N=150, 2048 chains: ~NP^2/3 cycles while one parameter set's table stays within ~6 MB (its share of
// an XCD's L2), growing by ~3 % per further MB as reads fall through to the Infinity Cache, up to the HBM rate.
// GEMM chain: cycles (at ~2.2 GHz) a CU needs to advance ONE segment by one step - all column slabs of the segment, chip
// full.  Measured round 3 on every built tile count below (profiles/r03_e_calib_big.txt: one 1e7-column chunk, all CUs
// busy): 0.55 us at NP = 32, 1.52 at 48, 2.9 at 64, 9.4 at 96, 15.0 at 112, 33 at 160.  Rounds 1-2 used
// 0.027 NP^3 + 20000 cycles, fitted at NP = 160 on round 1's kernel: 1.8x too high there and 16x too high at NP = 32, so
// that 24 < N <= 64 with a handful of chunks x parameter sets took the mat-vec chain (one workgroup per chain, 10-40
// workgroups on 256 CUs) at 3-9x the GEMM chain's time.
inline double gemm_cu_step_cycles(int np)
{
    const int nt = np / 16;
    double us;
    switch (nt) {
    case 2: us = 0.55; break;
    case 3: us = 1.52; break;
    case 4: us = 2.9; break;
    case 6: us = 9.4; break;
    case 7: us = 15.0; break;
    case 8: us = 22.4; break;
    case 9: us = 24.1; break;
    default: us = 33.0 * (nt / 10.0) * (nt / 10.0) * (nt / 10.0); break;
    }
    return us * 2200.0;
}

inline double matvec_step_cycles(double np2, int alphabet)
{
    const double table_mb = (double)alphabet * np2 * 8.0 / 1.0e6;
    return np2 / 3.0 * std::min(2.2, 1.0 + 0.03 * std::max(0.0, table_mb - 6.0));
}

// Rank-one hand-off estimate for a GEMM-chain group whose base plan has `nseg` segments of `seglen` elements (one
// round of workgroups): m times the segments = m rounds of `head`-long GEMM heads, tails 1/m as long on the mat-vec
// chain.  A tail step streams NP^2 doubles; with many chains that is the memory system's bandwidth (measured: 256
// chains of a 1.6 GB table read 7 TB/s), with few it is one workgroup's latency.  Returns the best m (0: not
// worth it) and its cycles.
struct HandoffEstimate { int m; double cycles; };
inline HandoffEstimate estimate_handoff(double seglen, double nseg, int B, double head, double np, int nslab, int alphabet, int cus)
{
    // (a segment's GEMM step is shared by its nslab column-slab workgroups)
    const double np2 = np * np, t_gemm = 1.15 * gemm_cu_step_cycles((int)np) / nslab;   // (a head step of one slab's workgroup)
    const double table_mb = (double)alphabet * np2 * 8.0 / 1.0e6;
    const double bw = table_mb > 128.0 ? 7.0e12 : table_mb > 16.0 ? 8.6e12 : 15.0e12;   // bytes/s: HBM, Infinity Cache, L2
    HandoffEstimate best{0, 1e300};
    for (int m = 1; m <= 6; ++m) {
        const double sl = seglen / m;
        if (sl < 2.0 * head) break;
        const double chains = m * nseg * B, active = std::min(chains, (double)cus);
        const double t_vec = std::max(np2 / 4.5 + 1500.0, active * np2 * 8.0 * 2.1e9 / bw) * std::max(1.0, chains / cus);
        const double est = m * head * t_gemm + (sl - head) * t_vec;
        if (est < best.cycles) best = HandoffEstimate{m, est};
    }
    return best;
}

// k_zpropagate4 on the streamed table (nothing cached in LDS)?  With the XCD-affine grid (enqueue) an XCD reads one or
// two parameter sets' tables at a time whatever B is, and the streamed form then beat the hybrid one at every
// dictionary level and every B measured (profiles/r03_d_affine_levels.txt); without it, while all tables of the launch
// fit the L2s.
inline bool z4_streamed(const PlanOptions &opt, double tables_bytes, int n_sets)
{
    if (opt.z4_stream >= 0) return opt.z4_stream == 1;
    return (opt.xcd_affine && n_sets > 1) || tables_bytes <= Z4_STREAM_MAX_BYTES;
}

// hand-off head of a group whose stream elements span `span` alignment columns each, in stream elements:
// ~R1_HEAD_COLUMNS alignment columns
inline size_t handoff_head(double span) { return round_up(std::max<size_t>(R1_MIN_HEAD, (size_t)(R1_HEAD_COLUMNS / span)), 16); }

// (up to 12 states two workgroups of the global-table kernel can share a CU; the callers add what else they require)
inline bool two_per_cu_possible(const PlanOptions &opt, const KernelFacts &kc, int A, int B)
{
    return kc.NP <= 12 && z4_streamed(opt, (double)B * (A + 1) * kc.tok_doubles * 8.0, B);
}

// decide_groups in two phases; the second reads what the first left in the members.
struct GroupDecider {
    const PlanOptions &opt;
    const KernelFacts &kc;
    // 25-32 states: kc is the vector kernels' entry and every dictionary's chunks run its streamed blocked scan
    // (k_zpropagate4<7 | 8>); chunks without tokens stay on the vector kernels.  wide_ok: every dictionary had a level for it.
    const bool wide;
    const std::vector<ChunkFacts> &chunks;
    const std::vector<DictFacts> &dicts;
    const int N, S, B;
    const bool op_mode;                 // imc_forward_state(as_operator): no segment is a chunk's "first"
    const int n_chunks = (int)chunks.size();
    PlanDecision d;
    std::vector<GroupDecision> &groups = d.groups;
    std::vector<int> &chunk_group = d.chunk_group;
    bool &wide_ok = d.wide_ok;
    bool mfma() const { return kc.use3(opt.blocked_variant) || wide; }      // the blocked kernels of this plan are the fp64-MFMA ones
    // What the first phase knows of a group's kind before choose_segment_lengths() fixes it.
    bool chain_tentative = false;       // the plan's kernel entry is the large-N one: every group ends as GemmChain or MatVecChain
    std::vector<char> global_tentative; // per group: its level was chosen for the global-table scan (alphabet beyond LDS, or 16-bit tokens)
    // a group's stream elements and the alignment columns one of them spans
    struct Span { double toks, span; };
    Span group_span(const GroupDecision &gr) const
    {
        double cols = 0.0, toks = 0.0;
        for (int f : gr.chunks) { cols += (double)chunks[f].L; toks += (double)(gr.tokens ? chunks[f].level[gr.level].ntok : chunks[f].L); }
        return Span{toks, toks > 0.0 ? cols / toks : 1.0};
    }

    void assign_groups()
    {
        // ---- assign chunks to launch groups: plain, or (dictionary, level) ----
        const bool big = chain_tentative = kc.R == 0;
        int a_max = 0;   // largest alphabet whose operator table fits LDS for this N (no limit on the large-N path)
        if (big) a_max = kMaxAlphabet;
        else
            for (int A = 1; A <= kByteAlphabet; ++A)   // (the LDS-table kernels read byte streams only)
                if (kc.zip_lds(A) <= LDS_BUDGET || (kc.has_zip2 && opt.kernel_pref != 1 && kc.blocked_lds(A, opt.blocked_variant) <= LDS_BUDGET)) a_max = A;
        // One dictionary level per dictionary: the deepest level is not always the best - every workgroup rebuilds
        // the operator table per evaluation ((A - S) dependent small products), which dominates on short inputs.
        // Estimate: table build + main loop with all 16-lane rows of the machine busy.
        std::vector<int> dict_level(dicts.size(), -1);
        const bool mfma_blocked = !big && mfma() && opt.kernel_pref != 1;
        const int SL = kc.z4_slots();   // segments per workgroup of the blocked kernels
        std::vector<double> dict_cost(dicts.size(), 0.0), dict_tab(dicts.size(), 0.0);     // per dictionary, microseconds: the chosen level's estimate, its table part
        if (opt.compression) {
            std::vector<std::vector<int>> by_dict(dicts.size());
            for (int f = 0; f < n_chunks; ++f)
                if (chunks[f].dict >= 0 && chunks[f].nsym == S) by_dict[chunks[f].dict].push_back(f);
            for (size_t di = 0; di < by_dict.size(); ++di) {
                const std::vector<int> &members = by_dict[di], &depth = *dicts[di].depth;
                if (members.empty()) continue;
                double best = 1e300;
                int best_l = -1;
                for (int l = 0; l < kNumLevels; ++l) {
                    const ChunkFacts &o0 = chunks[members[0]];
                    if (mfma_blocked) {
                        // Blocked MFMA kernels, estimated in microseconds: the table is built one dictionary depth at
                        // a time (32 tokens per pass), the scan advances cus * 32 segments per wavefront-step.  Levels
                        // that fit LDS run k_zpropagate3; byte levels beyond that can run k_zpropagate4 (hybrid table:
                        // one workgroup builds it in L2, steps on tokens outside the LDS-cached hot set cost ~12 % more).
                        const int A = o0.level[l].alphabet;
                        if (!(A > o0.nsym && A <= HYBRID_MAX_ALPHABET && o0.level[l].stream) || o0.wide_raw) continue;
                        const bool fits = !wide && !o0.level[l].wide && kc.blocked_lds(A, opt.blocked_variant) <= LDS_BUDGET;   // (k_zpropagate3 reads byte streams)
                        const int max_hot = kc.has_zip4 ? kc.zip4_max_hot(A, LDS_BUDGET) : 0;
                        const double table_bytes = (double)B * (A + 1) * kc.tok_doubles * 8.0;
                        // (25-32 states: the streamed form or nothing - a table it does not take stays off this path)
                        const bool hybrid_ok = !fits && !o0.level[l].counts().empty() && table_bytes <= 2.0e9 &&
                                               (wide ? kc.has_zip4s && z4_streamed(opt, table_bytes, B) : kc.has_zip4 && opt.blocked_variant >= 4 && max_hot >= 8);
                        if (!fits && !hybrid_ok) continue;
                        // (the scan's LDS: the fold's exchange area + the exponents and slot map of all A + 1 entries - at 24
                        // states the exchange area alone is 152 KB and levels beyond 768 tokens do not fit)
                        if (!fits && kc.zip4_lds(A, 0) > LDS_BUDGET) continue;
                        int passes = 0;
                        {
                            std::map<int, int> per_depth;
                            for (int z = o0.nsym; z < A; ++z) per_depth[depth[z]]++;
                            for (auto &pd : per_depth) passes += (pd.second + SL - 1) / SL;
                        }
                        // (up to 8 states a step is not MFMA time: measured round 3, 4 and 8 states, 64 sets - 0.08 / 0.14 us from
                        // the LDS table, 0.19 / 0.22 from the global one; from 12 states on both follow the instruction count)
                        const double nt = kc.NP / 4.0;
                        // (a workgroup's step: its wavefronts share the SIMDs' matrix pipes two by two - or, four wavefronts, have one each)
                        const double t_step = nt < 1.5 ? 0.08 : nt < 2.5 ? 0.14 : std::max(0.25, 1.88 * nt * nt * nt / 125.0) * (kc.z4_waves / 8.0);
                        const double t_step_g = nt < 1.5 ? 0.19 : nt < 2.5 ? 0.22 : t_step;
                        // Time of the scan itself: workgroups of 32 segments are dealt PER CHUNK (a chunk of u workgroups is cut
                        // into 32 u segments), and a launch of more workgroups than CUs runs in rounds, each paying the
                        // workgroup's fixed part again.  rounds x (fixed + segment length x step) for the best number of rounds -
                        // not tokens / slots: 100 chunks x 1e6 columns fill 78 % of one round or 98 % of two.
                        double maxtok = 0.0;
                        for (int f : members) maxtok = std::max(maxtok, (double)chunks[f].level[l].ntok);
                        // (up to 12 states two workgroups of the global-table kernel share a CU: twice the slots, 1.85x the step)
                        const bool two_per_cu = !fits && two_per_cu_possible(opt, kc, A, B);
                        const double n_ch = (double)members.size(), slots = (double)opt.cus * SL * (two_per_cu ? 2.0 : 1.0);
                        auto scan_time = [&](double fixed_us, double step_us) {
                            if (two_per_cu) step_us *= 1.85;
                            double best_t = 1e300;
                            for (int r = 1; r <= 6; ++r) {
                                const double units = std::max(1.0, std::floor(slots * r / (n_ch * B) / SL));
                                const double seg = std::max(16.0, std::ceil(maxtok / (SL * units)));
                                const double rounds = std::ceil(n_ch * B * units * SL / slots);
                                best_t = std::min(best_t, rounds * (fixed_us + seg * step_us));
                            }
                            return best_t;
                        };
                        double cost;
                        // LDS table: EVERY workgroup rebuilds it, one barrier-separated pass per 32 tokens of a depth
                        // (measured round 3: ~1.9 us per pass at 10 states, ~2.8 at 20), plus launch and the in-kernel
                        // fold (~14 us).  Round 2 priced a pass at 1.1 us and no fixed part: at 10 states and 100 x 1e6
                        // columns it then preferred the 128-token LDS table (135 us) to the global table (102 us).
                        if (fits) cost = 4.0 + scan_time(10.0 + passes * (1.6 + 1.2 * nt * nt * nt / 125.0), t_step);
                        else {
                            std::vector<uint64_t> cnt((size_t)A, 0);
                            for (int f : members)
                                for (size_t z = 0; z < chunks[f].level[l].counts().size() && z < cnt.size(); ++z) cnt[z] += chunks[f].level[l].counts()[z];
                            std::vector<uint64_t> sorted(cnt);
                            std::sort(sorted.begin(), sorted.end(), std::greater<uint64_t>());
                            uint64_t all = 0, top = 0;
                            for (size_t z = 0; z < sorted.size(); ++z) { all += sorted[z]; if ((int)z < std::min(max_hot, A)) top += sorted[z]; }
                            const double cold = all ? 1.0 - (double)top / (double)all : 0.0;
                            const double depths = (double)std::max<int>(1, (int)std::set<int>(depth.begin() + o0.nsym, depth.begin() + A).size());
                            // one ~4 us launch per depth; a cold step costs ~11 % more while one parameter set's table
                            // stays in an XCD's L2, ~17 % from the Infinity Cache (scratch microbenchmark)
                            // (hybrid form; the streamed form - tables of the launch cache resident - runs every step
                            // from the global table at ~6 % over the LDS-table kernel's step: measured at config[1])
                            const double cold_pen = table_bytes / B <= 3.6e6 ? 0.11 : 0.17;
                            const bool streamed = z4_streamed(opt, table_bytes, B);
                            // (table: one ~4.5 us launch per depth, or one ~5.7 us launch per pair of depths)
                            // (measured round 3: the first launch - it fetches the parameters - ~13 us, the others ~7.5)
                            double t_table = opt.table_pairs && kc.has_level2 ? 13.0 + (std::ceil(depths / 2.0) - 1.0) * 7.5 : 6.0 + depths * 4.9;
                            // ... which is latency; B tables of A operators are also two reads and a write of an operator per
                            // token and parameter set, at ~2.8 TB/s (measured round 3, 64 sets: 4096- against 512-token tables)
                            t_table += std::max(0.0, table_bytes * 3.0 / 2.8e6 - 0.5 * t_table);
                            cost = t_table + scan_time(8.0, t_step_g * (streamed ? 1.06 : 1.0 + cold_pen * cold));
                        }
                        if (cost < best) dict_cost[di] = cost;
                        if (opt.blocked_variant == 5 && !fits) cost *= 1e-3;      // tests: the hybrid table wherever it is possible
                        if (opt.debug_levels)
                            std::fprintf(stderr, "[imc] level %d alphabet %d %s: model %.1f us\n", l, A,
                                         fits ? "LDS table" : two_per_cu ? "global table, 2 per CU" : "global table", cost);
                        if (cost < best) { best = cost; best_l = l; }
                        continue;
                    }
                    if (!(o0.level[l].alphabet <= a_max && o0.level[l].alphabet > o0.nsym && o0.level[l].stream)) continue;
                    if (big && (size_t)B * o0.level[l].alphabet * kc.NP * kc.NP * 8 > CTAB_BUDGET) continue;   // table too large
                    double toks = 0.0;
                    for (int f : members) toks += (double)chunks[f].level[l].ntok;
                    const double n3 = (double)kc.NP * kc.NP * kc.NP;
                    double c_tab, c_main;   // cycles
                    if (big) {   // one GEMM per step per workgroup, table built by depth
                        const double gemm = gemm_cu_step_cycles(kc.NP);
                        c_tab = ((o0.level[l].alphabet - S) / (double)opt.cus + 12.0) * gemm;   // one workgroup per token, ~12 depth launches
                        c_main = std::max(16.0, toks * B / (double)opt.cus) * gemm;
                        double lmax = 0.0;   // or the mat-vec chain kernel, when no chunk needs splitting
                        for (int f : members) lmax = std::max(lmax, (double)chunks[f].level[l].ntok);
                        const double np2 = (double)kc.NP * kc.NP;
                        const double c_vec = std::max(lmax * (np2 / 4.5 + 1500.0), toks * B / (double)opt.cus * matvec_step_cycles(np2, o0.level[l].alphabet));
                        if (!op_mode && (opt.kernel_pref == 1 || (opt.kernel_pref == 0 && c_vec < c_main))) c_main = c_vec;
                    } else {     // ~5200 cycles per row-step at N=20; every workgroup rebuilds the table
                        c_tab = (o0.level[l].alphabet - S) * (400.0 + n3 / 64.0);
                        c_main = std::max(16.0, toks * B / ((double)opt.cus * 32.0)) * 0.65 * n3;
                    }
                    if (c_tab + c_main < best) { best = c_tab + c_main; best_l = l; dict_cost[di] = best / 2200.0; dict_tab[di] = c_tab / 2200.0; }
                }
                if (opt.force_level >= 0) {   // experiments only: pin the dictionary level index
                    const int l = opt.force_level;
                    const ChunkFacts &o0 = chunks[members[0]];
                    const bool hybrid = mfma_blocked && (wide || (kc.has_zip4 && opt.blocked_variant >= 4)) && !o0.wide_raw;
                    const int amax_forced = hybrid ? HYBRID_MAX_ALPHABET : a_max;
                    if (l >= 0 && l < kNumLevels && o0.level[l].alphabet <= amax_forced && !(hybrid && (wide || kc.blocked_lds(o0.level[l].alphabet, opt.blocked_variant) > LDS_BUDGET) && kc.zip4_lds(o0.level[l].alphabet, 0) > LDS_BUDGET) && o0.level[l].alphabet > o0.nsym && o0.level[l].stream &&
                        (hybrid ? !o0.level[l].counts().empty() : !o0.level[l].wide)) best_l = l;
                }
                dict_level[di] = best_l;
                if (wide && best_l < 0) wide_ok = false;
            }
        }
        chunk_group.assign(n_chunks, -1);
        for (int f = 0; f < n_chunks; ++f) {
            const ChunkFacts &o = chunks[f];
            int level = -1;
            if (opt.compression && o.dict >= 0 && o.nsym == S) level = dict_level[o.dict];
            int gi = -1;
            for (size_t q = 0; q < groups.size(); ++q) {
                GroupDecision &gr = groups[q];
                if (level < 0 ? !gr.tokens : (gr.tokens && gr.level == level && gr.dict == o.dict)) gi = (int)q;
            }
            if (gi < 0) {
                GroupDecision gr;
                gr.tokens = level >= 0;
                gr.level = level;
                gr.A = S;
                if (gr.tokens) { gr.dict = o.dict; gr.A = o.level[level].alphabet; }
                // an alphabet beyond LDS can only have been chosen for the hybrid-table kernel
                global_tentative.push_back(gr.tokens && mfma_blocked && (wide || kc.blocked_lds(gr.A, opt.blocked_variant) > LDS_BUDGET || o.level[level].wide));
                if (gr.tokens) { gr.model_us = dict_cost[o.dict]; gr.model_tab_us = dict_tab[o.dict]; }
                gr.wide_tokens = gr.tokens && o.level[level].wide;
                groups.push_back(std::move(gr));
                gi = (int)groups.size() - 1;
            }
            groups[gi].chunks.push_back(f);
            chunk_group[f] = gi;
        }
    }

    void choose_segment_lengths()
    {
        // ---- segment length per group ----
        for (size_t q = 0; q < groups.size(); ++q) {
            GroupDecision &gr = groups[q];
            const bool global = global_tentative[q] != 0;
            bool matvec = false;    // (chain plans) granted by the cost comparison below, revoked if a forced segment length cuts a chunk
            bool blocked = false;   // (other plans) the register-blocked scan instead of the vector kernel
            std::vector<size_t> lens;
            for (int f : gr.chunks) lens.push_back(gr.tokens ? chunks[f].level[gr.level].ntok : chunks[f].L);
            if (chain_tentative) {
                // every segment costs N^3 per step whatever the split (one workgroup = one CU's worth of LDS), so
                // one equal-length segment per CU is both balanced and the fewest operators for the stitch
                size_t total = 0;
                for (size_t L : lens) total += L;
                const size_t per_cu = std::max<size_t>(1, std::min<size_t>(LDS_BUDGET / kc.big_lds, (size_t)32 / (size_t)kc.G));
                const size_t target = std::max<size_t>(1, (size_t)opt.cus * per_cu / ((size_t)B * kc.big_nslab));
                gr.seglen = std::max<size_t>(16, round_up((total + target - 1) / target, 16));
                // Chunks are cut one by one (ceil(L / seglen) segments each): with several chunks the sum can exceed the
                // target by a few segments - and one segment more than the machine holds is a second ROUND of workgroups,
                // twice the time (measured round 3 at 150 states, 3 x 3e6 columns: 129 segments for 128 slots, 201 ms
                // against 103).  Lengthen the segments until the launch fits.
                {
                    auto count = [&](size_t sl) { size_t c = 0; for (size_t L : lens) c += (L + sl - 1) / sl; return c; };
                    size_t nonempty = 0;
                    for (size_t L : lens) nonempty += L > 0;
                    if (nonempty <= target)            // (more chunks than slots: rounds are unavoidable)
                        for (int it = 0; it < 65536 && count(gr.seglen) > target; ++it) gr.seglen += 16;
                }
                // ... unless there are so many (chunk, parameter set) chains that no chunk needs splitting: then
                // the mat-vec chain kernel streams NP^2 doubles per step instead of a GEMM (measured at N=150, 64 x 32
                // chains: 8900 cycles per step per CU, i.e. ~12 TB/s of operator reads over the whole chip)
                size_t lmax = 0;
                for (size_t L : lens) lmax = std::max(lmax, L);
                const double np2 = (double)kc.NP * kc.NP, per_cu_steps = (double)total * B / (double)opt.cus;
                const double cost_vec = std::max((double)lmax * (np2 / 4.5 + 1500.0), per_cu_steps * matvec_step_cycles(np2, gr.A));
                double cost_gemm = std::max(16.0, per_cu_steps) * gemm_cu_step_cycles(kc.NP);
                if (opt.rank1_handoff && !opt.seg_override && gr.seglen >= R1_MIN_SEGLEN) {   // GEMM heads + mat-vec tails
                    const HandoffEstimate he = estimate_handoff((double)gr.seglen, std::max(1.0, (double)total / gr.seglen), B,
                                                                (double)handoff_head(group_span(gr).span), kc.NP, kc.big_nslab, gr.A, opt.cus);
                    if (he.m) cost_gemm = std::min(cost_gemm, he.cycles);
                }
                if (opt.debug)
                    std::fprintf(stderr, "[imc] plan: GEMM chain seg %zu cost %.3g cycles; mat-vec chain cost %.3g cycles\n",
                                 gr.seglen, cost_gemm, cost_vec);
                // (no chunk longer than a segment: there would be no operator segments anyway)
                if (!op_mode && (opt.kernel_pref == 1 || (opt.kernel_pref == 0 && (cost_vec < cost_gemm || lmax <= gr.seglen)))) {
                    matvec = true;
                    gr.seglen = std::max<size_t>(16, round_up(lmax, 16));
                }
                // (build_plan's comparison: the level estimate's table part + this, the refined estimate of the chain that was taken)
                if (gr.tokens) gr.model_us = gr.model_tab_us + (matvec ? cost_vec : cost_gemm) / 2200.0;
            } else {
                // vector kernel (one vector per lane group) ...
                double cost_vec = 0.0;
                size_t seg_vec;
                if (gr.tokens) {
                    // LDS-bound: a workgroup of kc.zwaves wavefronts serialises on one CU's LDS
                    const double lds_cycles = ((double)kc.R * kc.NP / 2 + kc.NP / 2.0) * 4.0 + kc.R * 6.0 + 40.0;
                    seg_vec = choose_seglen(lens, N, B, kc.VPW, (double)opt.cus * kc.zwaves, lds_cycles * kc.zwaves, &cost_vec);   // measured: 4600 cycles per wavefront-step at N=20
                } else {
                    // VALU-bound, minw wavefronts share a SIMD: measured 555 cycles per wavefront-column per SIMD at N=20
                    seg_vec = choose_seglen(lens, N, B, kc.VPW, (double)opt.cus * 4.0 * kc.minw,
                                            kc.minw * 1.7 * (4.0 * kc.R * kc.NP + 16.0), &cost_vec);
                }
                gr.seglen = seg_vec;
                // ... or the register-blocked kernel (one operator per 16-lane row): fill every row of the machine
                // once; first segments waste 1 - 1/N of their row, which the cost comparison accounts for
                if ((kc.has_zip2 || (wide && global)) && opt.kernel_pref != 1 && (global || kc.blocked_lds(gr.A, opt.blocked_variant) <= LDS_BUDGET) && (gr.tokens || (S == gr.A && S <= kByteAlphabet))) {
                    const int SL = kc.z4_slots(), WV = kc.z4_waves;   // segments / wavefronts per workgroup
                    size_t total = 0;
                    for (size_t L : lens) total += L;
                    // Up to 12 states the global-table kernel needs 124 registers and no LDS to speak of: TWO workgroups share a
                    // CU (four wavefronts per SIMD), i.e. the machine has twice the rows, each step taking ~1.85x as long
                    // (measured at 10 states, 100 x 1e6 columns: 500 workgroups of 44-token segments 102 us, 200 workgroups
                    // of 104-token segments 113 us).
                    const bool two_per_cu = global && kc.use3(opt.blocked_variant) && two_per_cu_possible(opt, kc, gr.A, B);
                    const double rows = (double)opt.cus * SL * (two_per_cu ? 2.0 : 1.0);
                    const double rb = kc.NP / 4.0;
                    // per wavefront-step (4 segments): DPP/VALU form measured ~2900 at N=20; the MFMA form issues
                    // (NP/4)^3 v_mfma_f64_4x4x4 at ~25.5 cycles each with two wavefronts per SIMD and nothing else
                    const double step_cycles = (mfma() ? 25.5 * rb * rb * rb * 0.55 : 5.8 * rb * rb * kc.NP) * (two_per_cu ? 1.85 : 1.0);
                    size_t seg_blk = 16;
                    double slots = 0.0, cost_blk = 1e300;
                    // a workgroup takes 32 consecutive segments of ONE chunk: rows are allocated per chunk in 32s
                    // (... except chunks that are ONE segment: those are packed, a row each - plan_geometry)
                    const bool can_pack = mfma() && !op_mode;
                    auto rows_used = [&](size_t sg) {
                        double r = 0.0, singles = 0.0;
                        for (size_t L : lens) {
                            if (!L) continue;
                            const double nseg = std::ceil((double)L / (double)sg);
                            if (nseg <= 1.0 && can_pack) singles += 1.0;
                            else r += std::ceil(nseg / SL) * SL;
                        }
                        return r + std::ceil(singles / SL) * SL;
                    };
                    // Candidates: fill the machine's rows `rounds` times - or, when chunks x parameter sets alone need more
                    // rounds than that (every chunk takes at least one workgroup of 32 rows per parameter set: 100 chunks x 64
                    // sets = 25 rounds), cut every chunk into u workgroups' worth of segments.  (Round 2 only had the first
                    // family, up to 16 rounds; beyond that its search ran into its iteration limit and returned segments of
                    // thousands of tokens with two of a workgroup's 32 rows in use: 100 x 1e6 columns x 64 proposals took
                    // 446 us per proposal at 10 states against 64 us at 8 proposals.)
                    size_t lmax = 0;
                    for (size_t L : lens) lmax = std::max(lmax, L);
                    std::vector<size_t> cands;
                    for (int rounds = 1; rounds <= 16; ++rounds) {
                        const double target = std::max((double)SL, std::floor(rows * rounds / B));
                        // (the blocked kernels take segments of any multiple of 4 tokens - dword-aligned 16-byte
                        // loads - so the machine's rows can be filled to within a per cent, not to within 16 tokens)
                        size_t sg = std::max<size_t>(16, round_up((size_t)std::ceil((double)total / target), Z2GRAN));
                        int it = 0;
                        for (; it < 1024 && rows_used(sg) > target && sg < lmax + 16; ++it) sg += Z2GRAN;
                        if (rows_used(sg) > target) continue;                    // this many rounds cannot hold the launch
                        cands.push_back(sg);
                    }
                    for (size_t u = 1; u <= 8; ++u)
                        cands.push_back(std::max<size_t>(16, round_up((lmax + SL * u - 1) / (SL * u), Z2GRAN)));
                    // ... and, for mixes of one long chunk with many short ones, the same for the MEDIAN chunk plus a few fixed
                    // short lengths: both families above follow the longest chunk, and when the short chunks alone need more
                    // than 16 rounds (each takes a workgroup per parameter set whatever the segment length) every candidate
                    // was hundreds of tokens long - 500 chunks of 1e5 columns beside one of 2.5e7, 8 sets, 20 states: 432-token
                    // segments, two of a workgroup's 32 rows in use on 4000 workgroups, 5.7 ms against 2.5.
                    {
                        std::vector<size_t> sorted(lens);
                        std::sort(sorted.begin(), sorted.end());
                        const size_t med = sorted[sorted.size() / 2];
                        for (size_t u = 1; u <= 4; ++u)
                            cands.push_back(std::max<size_t>(16, round_up((med + SL * u - 1) / (SL * u), Z2GRAN)));
                        for (size_t fixed_len : {16, 32, 48, 64, 96, 128, 192}) cands.push_back(fixed_len);
                        // whole chunks as single segments (packed 32 to a workgroup): the length of the median, the 90 % and the
                        // longest chunk
                        if (can_pack)
                            for (size_t qi : {sorted.size() / 2, sorted.size() * 9 / 10, sorted.size() - 1})
                                cands.push_back(std::max<size_t>(16, round_up(sorted[qi], Z2GRAN)));
                    }
                    for (size_t sg : cands) {
                        // per round of workgroups: the main loop, plus the table rebuild and the 5-level in-kernel fold
                        // (table: the VALU form builds token by token; the MFMA form one dictionary depth per pass,
                        // ~10 depths; with the hybrid table a workgroup only copies its hot set from L2)
                        const double table = !mfma() ? (double)(gr.A - S) * (400.0 + (double)kc.NP * kc.NP * kc.NP / 64.0)
                                             : global ? 9000.0 : 2600.0 * std::min(12.0, (double)(gr.A - S));
                        const double fixed = table + 5.0 * (WV / 4.0) * step_cycles;
                        // A segment length that is not a multiple of 16 ends in a MASKED block (the pipeline is re-primed per
                        // run of it: ~3.5 us; measured at 10 states, 100 x 1e6 columns: 48-token segments 101.9 us, 44-token
                        // ones 109.6) - so the next multiple of 16 is priced beside the exact fit.
                        for (size_t cand : {sg, round_up(sg, 16)}) {
                            const double u = rows_used(cand);
                            double c = std::ceil(u * B / rows) * ((double)cand * (WV / 4.0) * step_cycles + fixed + (cand % 16 ? 7700.0 : 0.0));
                            // (every chunk a single packed segment: measured 10 % behind the best split where the model has a tie)
                            if (can_pack && cand >= lmax) c *= 1.15;
                            if (c < cost_blk) { cost_blk = c; seg_blk = cand; slots = u; }
                        }
                    }
                    if (opt.debug)
                        std::fprintf(stderr, "[imc] plan: vector kernel seg %zu cost %.3g cycles; blocked kernel seg %zu slots %.0f cost %.3g cycles\n",
                                     seg_vec, cost_vec, seg_blk, slots, cost_blk);
                    const bool vec_fits = !gr.tokens || kc.zip_lds(gr.A) <= LDS_BUDGET;   // the table may only fit the blocked kernel
                    if (opt.kernel_pref == 2 || cost_blk < cost_vec || !vec_fits || global) { blocked = true; gr.seglen = seg_blk; }
                }
                if (gr.tokens && !blocked) gr.model_us = gr.model_tab_us + cost_vec / 2200.0;   // (build_plan's comparison)
            }
            if (opt.seg_override) gr.seglen = round_up(std::max<size_t>(opt.seg_override, 16), 16);   // tests: force stitching
            if (matvec)
                for (size_t L : lens) matvec = matvec && L <= gr.seglen && !op_mode;
            // rank-one hand-off: worth a test once segments are much longer than the HMM's memory (tens of thousands
            // of columns); a quarter of the segment on the GEMM chain, then the certified test
            if (chain_tentative && !matvec && opt.rank1_handoff && gr.seglen >= R1_MIN_SEGLEN) {
                // head: ~R1_HEAD_COLUMNS alignment columns on the GEMM chain (the HMM's memory is a property of the
                // model, not of the segmentation).  The tails then cost a mat-vec per step, so MORE, shorter
                // segments pay: m times the segments = m rounds of heads, tails 1/m as long.  Pick m by the model;
                // if the test fails at run time the GEMM chain does the same total work as with m = 1.
                const double toks = group_span(gr).toks, span = group_span(gr).span;
                const size_t head = handoff_head(span);
                const double nseg = std::max(1.0, toks / (double)gr.seglen);
                if (opt.seg_override) {                 // tests: one checkpoint at a quarter of the forced segment length
                    if (gr.seglen >= 4 * R1_MIN_HEAD) {
                        gr.rank1 = true;
                        gr.checkpoints.assign(1, (int)round_up(gr.seglen / 4, 16));
                    }
                } else {
                    const int best_m = estimate_handoff((double)gr.seglen, nseg, B, (double)head, kc.NP, kc.big_nslab, gr.A, opt.cus).m;
                    if (best_m) {
                        gr.rank1 = true;
                        gr.seglen = std::max<size_t>(16, round_up(gr.seglen / best_m, 16));
                        // checkpoints: from ~8k alignment columns, each ~1.125x the previous (multiples of 16 tokens)
                        // up to ~100k columns - where the operators of the measured models collapse; a failing check
                        // is a quick reject and costs two near-empty launches - then 1.5x, while at least an eighth
                        // of the segment would still be left for the mat-vec chain
                        size_t c = round_up(std::max<size_t>(64, (size_t)(R1_HEAD_MIN_COLUMNS / span)), 16);
                        while ((int)gr.checkpoints.size() < R1_MAX_ROUNDS && c + gr.seglen / 8 < gr.seglen) {
                            gr.checkpoints.push_back((int)c);
                            const size_t step = (double)c * span < R1_DENSE_COLUMNS ? c / 8 : c / 2;
                            c = round_up(c + std::max<size_t>(16, step), 16);
                        }
                        if (gr.checkpoints.empty()) gr.rank1 = false;
                    }
                }
            }
            // the one statement of what the group is (a global-table level is always taken by the blocked scan)
            gr.kind = chain_tentative ? (matvec ? GroupKind::MatVecChain : GroupKind::GemmChain)
                      : blocked       ? (global ? GroupKind::BlockedGlobal : GroupKind::BlockedLds)
                      : gr.tokens     ? GroupKind::TokenVector
                                      : GroupKind::ColumnVector;
        }
    }
};

// Launch groups, dictionary levels, kernel families and segment lengths of one call for one kernel entry (host
// arithmetic only).  wide: 25-32 states with kc the vector kernels' entry - the dictionary groups take the blocked scan.
inline PlanDecision decide_groups(const PlanOptions &opt, const KernelFacts &kc, bool wide, const std::vector<ChunkFacts> &chunks,
                                  const std::vector<DictFacts> &dicts, int N, int S, int B, bool op_mode)
{
    GroupDecider x{opt, kc, wide, chunks, dicts, N, S, B, op_mode};
    x.assign_groups();
    x.choose_segment_lengths();
    return std::move(x.d);
}

// ---- the kernel entry: build_plan's choices between entries of the kernel table ----

// 24 < N <= 64: the GEMM-chain kernels beat the vector kernels by 5-100x when chunks are long enough to be
// cut into many operator segments; short-chunk / many-theta launches keep the vector kernels
inline bool prefer_gemm(const PlanOptions &opt, const std::vector<ChunkFacts> &chunks, int N, int S)
{
    const int n_chunks = (int)chunks.size();
    bool prefer = opt.kernel_pref == 2;
    if (opt.kernel_pref == 0 && N > 24 && N <= 64 && n_chunks > 0) {
        double total = 0.0;
        for (int f = 0; f < n_chunks; ++f) total += (double)chunks[f].L;
        bool tokens = opt.compression != 0;   // on the raw column stream the vector kernel still wins up to N=40 (no padding to 16s)
        for (int f = 0; f < n_chunks; ++f) tokens = tokens && chunks[f].dict >= 0 && chunks[f].nsym == S;
        // (round 3: 1e6 columns in all and 5e3 per chunk on average - it used to be 2e5 per chunk, and 100 chunks of 1e5
        // columns then ran on the LDS-table vector kernels at 4-9x the GEMM chain's time, profiles/r03_e_calib_big.txt)
        prefer = total >= 1.0e6 && total / n_chunks >= 5.0e3 && (tokens || N > 40);
    }
    return prefer;
}

// The odd tile counts (NP = 112, 144) pad less, but run one workgroup per segment: their base segments are
// half as long as the next shape's (two column slabs per segment), which on mid-sized inputs can fall below
// what the rank-one hand-off needs.  Take the next shape when it can hand off and this one cannot.
inline bool next_shape_hands_off(const PlanOptions &opt, const KernelFacts &kc, const KernelFacts &next,
                                 const std::vector<ChunkFacts> &chunks, int S, int B)
{
    double toks = 0.0, cols = 0.0;
    for (const ChunkFacts &c : chunks) {
        size_t nt = c.L;
        if (opt.compression && c.dict >= 0 && c.nsym == S)
            for (int l = 0; l < kNumLevels; ++l)
                if (c.level[l].stream) nt = std::min(nt, c.level[l].ntok);
        toks += (double)nt;
        cols += (double)c.L;
    }
    const double head = std::max<double>((double)R1_MIN_HEAD, R1_HEAD_COLUMNS / std::max(1.0, cols / std::max(1.0, toks)));
    auto eligible = [&](const KernelFacts &k) {
        const double per_cu = (double)std::max<size_t>(1, std::min<size_t>(LDS_BUDGET / k.big_lds, (size_t)32 / (size_t)k.G));
        const double target = std::max(1.0, (double)opt.cus * per_cu / ((double)B * k.big_nslab));
        const double seglen = toks / target;
        return seglen >= (double)R1_MIN_SEGLEN && seglen >= 2.0 * head;
    };
    return opt.rank1_handoff && !opt.seg_override && !eligible(kc) && eligible(next);
}

// 25-32 states, automatic mode: the blocked scan (k_zpropagate4<7 | 8>) is one more candidate for the chunks that have a
// dictionary - a second decision on the vector kernels' entry, whose dictionary groups take the scan.  It must take EVERY
// dictionary of the call, and, where the base decision is the GEMM chain's (base_chain), every chunk that has columns: raw
// streams and uncompressed chunks stay on the kernels they have.  A base that runs all of its dictionary groups on the
// mat-vec chain (many short chains) keeps that choice.  Otherwise the two estimates for the dictionary groups decide - the
// scan's is the blocked kernels' own model (assign_groups), with four wavefronts and 16 segments per workgroup.
inline bool wide_plan_wins(const PlanOptions &opt, const PlanDecision &base, bool base_chain, const PlanDecision &wide_plan,
                           const std::vector<ChunkFacts> &chunks, int N)
{
    bool any = false, all = wide_plan.wide_ok;
    double us_wide = 0.0, us_base = 0.0;
    for (const GroupDecision &gr : wide_plan.groups) {
        bool cols = false;
        for (int f : gr.chunks) cols = cols || chunks[f].L > 0;
        if (gr.kind == GroupKind::BlockedGlobal) { any = true; us_wide += gr.model_us; }
        else if (cols && base_chain) all = false;
    }
    bool base_matvec = false, base_other = false;
    for (const GroupDecision &gr : base.groups)
        if (gr.tokens) { us_base += gr.model_us; (gr.kind == GroupKind::MatVecChain ? base_matvec : base_other) = true; }
    base_matvec = base_matvec && !base_other;
    if (opt.debug)
        std::fprintf(stderr, "[imc] plan: blocked scan at %d states %s, model %.1f us; present kernels %.1f us%s\n", N,
                     any && all ? "possible" : "not possible", us_wide, us_base, base_matvec ? " (mat-vec chain)" : "");
    return any && all && (opt.wide_blocked == 1 || (!base_matvec && us_wide < us_base));
}

}  // namespace imc
