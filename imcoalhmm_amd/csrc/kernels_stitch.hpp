// kernels_stitch.hpp - combine the per-segment results of the propagate kernels into per-chunk
// log-likelihoods.  Included by imcoal_fwd.hip only.
//
// A level is a list of segments per chunk; a chunk's first segment is a VECTOR (N values + one
// exponent), every later one an OPERATOR (N x NP block stored state-major [i][c], one exponent per
// column c).  k_chain folds a run of g consecutive segments into one segment of the next level: a
// run that starts the chunk yields a vector (one chain), any other run yields an operator (N chains,
// one per basis vector).  Applied with g ~ sqrt(K) until every chunk holds a single vector, the
// serial depth drops from K steps to ~2 sqrt(K).  k_finish turns the last vectors into log-likelihoods.
#pragma once
#include "kernels_plain.hpp"
#include <utility>

// (ChainDesc, one chain of a level: launch_desc.hpp)

// How a step of k_chain<NP, D > 0> hands the rescaled vector (entry m in lane m) to every lane.
//   CHAIN_LDS   through LDS: one write, a fence, NP/2 broadcast 16-byte reads
//   CHAIN_LANE  two v_readlane_b32 per entry into a scalar pair
//   CHAIN_DPP   rows made whole-wave copies by the gfx950 lane swaps, then one v_mov_b64_dpp row_newbcast per entry
// All three apply the same operations to the same operands in the same order: the results are the same bits.
enum ChainForm { CHAIN_LDS = 0, CHAIN_LANE = 1, CHAIN_DPP = 2 };
// the library's form: the fastest in profiles/mb_chain_step.txt (CHAIN_LDS stays behind IMC_CHAIN_LDS=1)
static constexpr int CHAIN_STEP = CHAIN_DPP;

template <int... M, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, M...>, F &&f) { (f(std::integral_constant<int, M>()), ...); }

// x of lane M in every lane
template <int M>
__device__ __forceinline__ double lane_bcast_f64(double x)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), M), hi = __builtin_amdgcn_readlane(__double2hiint(x), M);
    return __hiloint2double(hi, lo);
}

// rows[r] = the 16-lane row r of x in all four rows (NP <= 16 * NR; rows beyond NR are not produced).  v_permlane32_swap
// exchanges the upper half of its first operand with the lower half of its second, v_permlane16_swap the odd rows of the
// first with the even rows of the second; applied to two copies of x they leave one copy of each half / row in both.
template <int NR>
__device__ __forceinline__ void rows_to_all(double x, double (&rows)[NR])
{
    static_assert(NR >= 1 && NR <= 4, "a wavefront has four rows");
    const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
    if constexpr (NR == 1) {
        rows[0] = x;
    } else if constexpr (NR == 2) {
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        rows[0] = __hiloint2double((int)h[0], (int)l[0]);
        rows[1] = __hiloint2double((int)h[1], (int)l[1]);
    } else {
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        const auto l0 = __builtin_amdgcn_permlane16_swap(l[0], l[0], false, false), h0 = __builtin_amdgcn_permlane16_swap(h[0], h[0], false, false);
        const auto l1 = __builtin_amdgcn_permlane16_swap(l[1], l[1], false, false), h1 = __builtin_amdgcn_permlane16_swap(h[1], h[1], false, false);
        rows[0] = __hiloint2double((int)h0[0], (int)l0[0]);
        rows[1] = __hiloint2double((int)h0[1], (int)l0[1]);
        rows[2] = __hiloint2double((int)h1[0], (int)l1[0]);
        if constexpr (NR == 4) rows[3] = __hiloint2double((int)h1[1], (int)l1[1]);
    }
}

// EMAX[b][seg] = max_c EX[b][vec0(seg)+c]
__global__ void k_emax(const uint32_t *seg_vec0, const uint8_t *seg_first, uint32_t n_segs, uint32_t n_vecs, int N,
                       const int *EX, int *EMAX)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (s >= n_segs) return;
    const int *e = EX + (size_t)b * n_vecs + seg_vec0[s];
    int m = e[0];
    if (!seg_first[s])
        for (int c = 1; c < N; ++c) m = max(m, e[c]);
    EMAX[(size_t)b * n_segs + s] = m;
}

// One workgroup per (chain, parameter set); thread i owns state i:
//     a <- Op_k * (a .* 2^(ex_k - emax_k))      for k in the run, rescaled by exact powers of two.
// The operators of a run are consecutive N-vector blocks, so their addresses are known up front: the
// rows and exponents of the next D operators are kept in flight in a register ring (D-deep prefetch),
// which takes the L2/HBM latency (~0.7 us) off the serial chain.  With D > 0 (one wavefront, NP <= 64) the
// kernel also finds each unit's largest exponent itself and EMin is not read; FORM says how a step's rescaled vector
// reaches every lane (D == 0 always goes through LDS).  Everything a chain needs before its first operand fetch is in
// its descriptor: one load, then the ring's first D fetches.
template <int NP, int D, int FORM = CHAIN_LDS>
__global__ __launch_bounds__(((NP + 63) / 64) * 64) void k_chain(
    const ChainDesc *chains, int N,
    uint32_t in_n_segs, uint32_t in_n_vecs, const double *Pin, const int *EXin, const int *EMin,
    uint32_t out_n_vecs, double *Pout, int *EXout, double *fin_out, int n_chunks)
{
    static_assert(FORM == CHAIN_LDS || (D > 0 && NP <= 64), "the register forms are for one wavefront");
    constexpr int NR = (NP + 15) / 16;   // 16-lane rows that hold entries of the vector
    __shared__ __attribute__((aligned(16))) double w[2][NP];
    // a single-wavefront workgroup needs no s_barrier (LDS is in-order within a wavefront), and a
    // __syncthreads() would drain the prefetch loads with its vmcnt(0)
    constexpr bool ONE_WAVE = NP <= 64;
    auto sync = [&]() { if (ONE_WAVE) wave_fence(); else __syncthreads(); };
    const ChainDesc cd = chains[blockIdx.x];
    const int b = blockIdx.y, i = threadIdx.x;
    const double *Pb = Pin + (size_t)b * in_n_vecs * NP;
    const int *EXb = EXin + (size_t)b * in_n_vecs;
    const int *EMb = EMin + (size_t)b * in_n_segs;
    const bool mine = i < N;
    const int ii = mine ? i : 0;

    double a;
    int etot;
    uint32_t k0 = cd.seg_begin;
    if (cd.first) {
        const uint32_t v = cd.vec_first;
        a = mine ? Pb[(size_t)v * NP + i] : 0.0;
        etot = EXb[v];
        ++k0;
    } else {
        a = (i == (int)cd.c) ? 1.0 : 0.0;
        etot = 0;
    }
    const int nsteps = (int)cd.seg_end - (int)k0;
    // operator k0+t starts at vector vbase + t*N (every segment after a chunk's first is an operator)
    const uint32_t vbase = cd.vbase;

    if constexpr (D == 0) {
        // large NP: no register ring (it would not fit); stream the operator row straight from L2
        int buf = 0;
        for (int t = 0; t < nsteps; ++t) {
            const size_t v0 = (size_t)vbase + (size_t)t * N;
            const int em = EMb[k0 + t];
            if (mine) w[buf][i] = ldexp(a, EXb[v0 + ii] - em);
            else if (i < NP) w[buf][i] = 0.0;
            sync();
            const double2 *row = reinterpret_cast<const double2 *>(Pb + (v0 + ii) * NP);
            const double2 *wv = reinterpret_cast<const double2 *>(&w[buf][0]);
            double acc0 = 0.0, acc1 = 0.0, s0 = 0.0, s1 = 0.0;
#pragma unroll 4
            for (int m = 0; m < NP / 2; ++m) {
                const double2 wc = wv[m], pc = row[m];
                acc0 = fma(pc.x, wc.x, acc0);
                acc1 = fma(pc.y, wc.y, acc1);
                s0 += wc.x;
                s1 += wc.y;
            }
            const double sm = s0 + s1;
            int e = 0;
            (void)frexp(sm, &e);
            e = (sm > 0.0 && sm < INFINITY) ? e : 0;
            a = mine ? ldexp(acc0 + acc1, -e) : 0.0;
            etot += em + e;
            buf ^= 1;
        }
    } else {
    double2 pk[D > 0 ? D : 1][NP / 2];
    int exr[D > 0 ? D : 1] = {};
    auto fetch = [&](int t, int slot) {   // slot is a compile-time constant at every call site
        const size_t v0 = (size_t)vbase + (size_t)t * N;
        // Loads only, D steps ahead of their use.  (Round 2 reduced the exponents to their maximum right here: that
        // waited for the load it had just issued and then ran six ds_bpermute round trips - ~0.5 us in front of every
        // step of the serial chain, most of the 0.65 us a step took.)  Lanes beyond N repeat column 0.
        exr[slot] = EXb[v0 + ii];
        const double2 *row = reinterpret_cast<const double2 *>(Pb + (v0 + ii) * NP);
#pragma unroll
        for (int m = 0; m < NP / 2; ++m) pk[slot][m] = row[m];
    };
#pragma unroll
    for (int s = 0; s < D; ++s)
        if (s < nsteps) fetch(s, s);   // (D > 0 here)
    // The unit's largest column exponent is found here instead of by a k_emax launch per level (seven DPP moves).  It
    // and the shift exr - em depend on prefetched integers only, so those of step t + 1 are taken while the FMAs of
    // step t run, not between two steps of the dependent chain.
    int em = 0, sh = 0;
    if (nsteps > 0) {
        em = wave_max_i32_dpp(exr[0]);
        sh = exr[0] - em;
    }
    int buf = 0;
    for (int t0 = 0; t0 < nsteps; t0 += D) {
#pragma unroll
        for (int s = 0; s < D; ++s) {
            const int t = t0 + s;
            if (t < nsteps) {   // wave-uniform
                const double wi = mine ? ldexp(a, sh) : 0.0;   // entry i of the rescaled vector
                const int em_t = em;
                double2 cur[NP / 2];
#pragma unroll
                for (int m = 0; m < NP / 2; ++m) cur[m] = pk[s][m];
                if (t + D < nsteps) fetch(t + D, s);
                // (slot s + 1 was fetched D - 1 steps ago; at s = D - 1 slot 0 holds step t0 + D by now.  No branch, so that
                // the scheduler may put this among the FMAs: beyond the last step the slot is stale and the result unused.)
                em = wave_max_i32_dpp(exr[(s + 1) % D]);
                sh = exr[(s + 1) % D] - em;
                // acc0 / s0 take the even columns in order, acc1 / s1 the odd ones, whatever the form
                double acc0 = 0.0, acc1 = 0.0, s0 = 0.0, s1 = 0.0;
                auto column = [&](auto M, double wm) {
                    constexpr int m = decltype(M)::value;
                    if constexpr (m & 1) {
                        acc1 = fma(cur[m / 2].y, wm, acc1);
                        s1 += wm;
                    } else {
                        acc0 = fma(cur[m / 2].x, wm, acc0);
                        s0 += wm;
                    }
                };
                if constexpr (FORM == CHAIN_LDS) {
                    if (i < NP) w[buf][i] = wi;
                    sync();
                    const double2 *wv = reinterpret_cast<const double2 *>(&w[buf][0]);
#pragma unroll
                    for (int m = 0; m < NP / 2; ++m) {
                        const double2 wc = wv[m];
                        acc0 = fma(cur[m].x, wc.x, acc0);
                        acc1 = fma(cur[m].y, wc.y, acc1);
                        s0 += wc.x;
                        s1 += wc.y;
                    }
                    buf ^= 1;   // the next step writes the other buffer: one fence per step suffices
                } else if constexpr (FORM == CHAIN_LANE) {
                    static_for(std::make_integer_sequence<int, NP>(), [&](auto M) { column(M, lane_bcast_f64<decltype(M)::value>(wi)); });
                } else {
                    double rows[NR];
                    rows_to_all<NR>(wi, rows);
                    static_for(std::make_integer_sequence<int, NP>(), [&](auto M) {
                        constexpr int m = decltype(M)::value;
                        column(M, __builtin_amdgcn_update_dpp(0.0, rows[m / 16], 0x150 + m % 16, 0xf, 0xf, true));   // row_newbcast:m%16
                    });
                }
                const double sm = s0 + s1;
                int e = 0;
                (void)frexp(sm, &e);
                e = (sm > 0.0 && sm < INFINITY) ? e : 0;
                // (lanes beyond N carry what row 0 gives them: every use of a below selects or stores by `mine`)
                a = ldexp(acc0 + acc1, -e);
                etot += em_t + e;
            }
        }
    }
    }
    // normalise the result by its total and store it as a segment of the next level
    double tot = 0.0;   // entries 0 .. N-1, left to right
    if constexpr (FORM == CHAIN_LDS) {
        sync();
        if (i < NP) w[0][i] = mine ? a : 0.0;
        sync();
        for (int c = 0; c < N; ++c) tot += w[0][c];
    } else if constexpr (FORM == CHAIN_LANE) {
        static_for(std::make_integer_sequence<int, NP>(), [&](auto M) {
            const double am = lane_bcast_f64<decltype(M)::value>(a);
            tot = decltype(M)::value < N ? tot + am : tot;
        });
    } else {
        double rows[NR];
        rows_to_all<NR>(a, rows);
        static_for(std::make_integer_sequence<int, NP>(), [&](auto M) {
            constexpr int m = decltype(M)::value;
            const double am = __builtin_amdgcn_update_dpp(0.0, rows[m / 16], 0x150 + m % 16, 0xf, 0xf, true);
            tot = m < N ? tot + am : tot;
        });
    }
    int e = 0;
    (void)frexp(tot, &e);
    e = (tot > 0.0 && tot < INFINITY) ? e : 0;
    const size_t gv = (size_t)b * out_n_vecs + cd.out_vec;
    if (mine) {
        double *dst = cd.first ? Pout + gv * NP + i : Pout + (gv - cd.c) * NP + (size_t)i * NP + cd.c;
        *dst = ldexp(a, -e);
    }
    if (i == 0) {
        EXout[gv] = etot + e;
        // last level: the chunk's log-likelihood straight from here (what k_finish computes from the stored vector:
        // the sum of the normalised entries is this sum scaled by the same exact power of two)
        if (fin_out && cd.chunk1)
            fin_out[(size_t)b * n_chunks + (cd.chunk1 - 1)] = (double)(etot + e) * 0.693147180559945309417232121458 + log(ldexp(tot, -e));
    }
}

// out[b][f] = log-likelihood of chunk f from its single remaining vector (0.0 for an empty chunk).
__global__ void k_finish(const int32_t *final_vec, int n_chunks, int N, int NP, uint32_t n_vecs, const double *P,
                         const int *EX, double *out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (f >= n_chunks) return;
    const int32_t v = final_vec[f];
    double r = 0.0;
    if (v >= 0) {
        const double *p = P + ((size_t)b * n_vecs + v) * NP;
        double tot = 0.0;
        for (int c = 0; c < N; ++c) tot += p[c];
        r = (double)EX[(size_t)b * n_vecs + v] * 0.693147180559945309417232121458 + log(tot);
    }
    out[(size_t)b * n_chunks + f] = r;
}

// State export: chunk f's single remaining unit, unreduced.  op == 0: its vector a[i] (N doubles, one exponent);
// op == 1: its transfer operator P[i][c] (N x N row-major, one exponent per column c).  Value = stored * 2^exponent.
__global__ void k_export(const int32_t *final_vec, int n_chunks, int N, int NP, uint32_t n_vecs, const double *P,
                         const int *EX, int op, double *out_state, int *out_exp)
{
    const int f = blockIdx.x, b = blockIdx.y;
    const int32_t v = final_vec[f];
    if (v < 0) return;
    const double *src = P + ((size_t)b * n_vecs + v) * NP;
    const int *ex = EX + (size_t)b * n_vecs + v;
    if (op) {
        double *dst = out_state + ((size_t)b * n_chunks + f) * N * N;
        int *de = out_exp + ((size_t)b * n_chunks + f) * N;
        for (int idx = threadIdx.x; idx < N * N; idx += blockDim.x) {
            const int i = idx / N, c = idx - i * N;
            dst[idx] = src[(size_t)i * NP + c];
        }
        for (int c = threadIdx.x; c < N; c += blockDim.x) de[c] = ex[c];
    } else {
        double *dst = out_state + ((size_t)b * n_chunks + f) * N;
        for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = src[i];
        if (threadIdx.x == 0) out_exp[(size_t)b * n_chunks + f] = ex[0];
    }
}

// Parameter upload by kernel: `src` is the device-visible alias of a mapped, pinned staging slot on the host.
__global__ void k_stage_params(const double2 *__restrict__ src, double2 *__restrict__ dst, unsigned n2)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n2) dst[i] = src[i];
}

// partial[b] = sum_f per_chunk[b][f], left to right from 0.0 (likelihood.py:33)
__global__ void k_sum_chunks(const double *per_chunk, int n_chunks, int B, double *partial)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double t = 0.0;
    for (int f = 0; f < n_chunks; ++f) t += per_chunk[(size_t)b * n_chunks + f];
    partial[b] = t;
}
