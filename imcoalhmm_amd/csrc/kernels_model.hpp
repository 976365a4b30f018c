// kernels_model.hpp - (pi, T) of a population of pairwise CoalHMMs on the device: what csrc/model_host.hpp does on the
// CPU for the 4- and 15-state spaces, for the spaces it leaves to numpy (the 94-state migration space; orders up to 128).
// Behind imc_model_transitions_device / imc_model_expm_batch_device (include/imcoal_model.h).
//
//   k_model_expm    one workgroup per SLOT = distinct (system, rate matrix, dt): exp(Q dt) by the algorithm of
//                   imc_model::expm.  The HOST chooses the Pade degree m and the squarings s (imc_model::expm_plan on the
//                   1-norm of Q dt, the function the host path calls too), so a workgroup's control flow is uniform and
//                   the choice is the host path's.  Matrices are row-major np x np, np = 16 ceil(n / 16), zero outside
//                   n x n: the pad stays zero under every product (the identity is added on the first n diagonal
//                   entries only) and the solve (V - U) R = V + U runs on the n x n part alone.  Every n^3 product is
//                   v_mfma_f64_16x16x4_f64 tiles, one 16 x 16 tile of C per wavefront and pass, operands straight from
//                   the slot's (L2-resident) work matrices.  The LU with partial pivoting keeps M and R in LDS when
//                   both fit (np <= 96: 2 x 72 KiB), else in the slot's work matrices.
//   k_model_joint   one workgroup per SYSTEM: through_i = expm (x projection), then the B / L / E recursion of
//                   imc_model::transitions_one in its order of operations - begin, diagonal, the V carry over the L
//                   class, closing sums, symmetrisation, total, pi, T = J / pi.  Plain fp64 FMA.  V ((n - 1) x |L|) lives
//                   in the workspace.  The joint total goes out for the host to check.
//   k_model_unpad   np x np results -> packed n x n (imc_model_expm_batch_device).
//
// Barriers sit only in loops whose trip count is the same for the whole workgroup (n, m, s and the class sizes are
// per-slot / per-system constants).  No atomics: a slot's or system's result is a function of its own inputs alone, so
// it does not depend on the rest of the launch and repeated calls agree bit for bit.
#pragma once
#include "kernels_big.hpp"

constexpr int MODEL_MAX_ORDER = 128;      // largest state space / rate matrix
constexpr int MODEL_MAX_INTERVALS = 256;
constexpr int MODEL_EXPM_THREADS = 512;   // 8 wavefronts
constexpr int MODEL_JOINT_THREADS = 256;
constexpr int MODEL_MATS = 9;             // work matrices of a slot: As A2 A4 A6 A8 U V Tm OUT
constexpr int MODEL_MAT_TM = 7, MODEL_MAT_OUT = 8;

struct ModelSlot {
    long long q_off;      // doubles into Q: the rate matrix, row-major n x n, unpadded
    long long w_off;      // doubles into the workspace: MODEL_MATS matrices of np x np
    long long r_off;      // doubles into the workspace: where exp(Q dt) ends up (OUT, or Tm after an odd number of squarings)
    double dt, scale;     // A = (Q dt) scale, scale = 2^-s
    int n, np, m, s;
};

struct ModelProjJob {     // dst (rows x cols, packed) = src (rows x rows, leading dimension src_ld) x projection (rows x cols)
    long long src_off, dst_off, proj_off;
    int src_ld, rows, cols, pad_;
};

struct ModelJointArgs {
    int n, s0, max_l;                 // intervals; order of interval 0's space; largest L class
    const int *space_size, *cls_off, *cls_idx;
    const double *proj, *start;
    const long long *thr_off;         // [systems][n - 1]: through_i, doubles into work
    const int *thr_ld;                // [systems][n - 1]: its leading dimension
    const ModelProjJob *jobs;
    const int *job_off;               // [systems + 1]
    double *work;
    long long v_off;                  // system b's two V buffers ((n - 1) x max_l each) start at v_off + 2 b (n - 1) max_l
    double *T, *pi, *total;           // [systems][n][n], [systems][n], [systems]
};

// Pade coefficients of imc_model::expm, rows: degree 3, 5, 7, 9, 13
__device__ const double model_pade[5][14] = {
    {120.0, 60.0, 12.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {30240.0, 15120.0, 3360.0, 420.0, 30.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0},
    {17297280.0, 8648640.0, 1995840.0, 277200.0, 25200.0, 1512.0, 56.0, 1.0, 0, 0, 0, 0, 0, 0},
    {17643225600.0, 8821612800.0, 2075673600.0, 302702400.0, 30270240.0, 2162160.0, 110880.0, 3960.0, 90.0, 1.0, 0, 0, 0, 0},
    {64764752532480000.0, 32382376266240000.0, 7771770303897600.0, 1187353796428800.0, 129060195264000.0, 10559470521600.0,
     670442572800.0, 33522128640.0, 1323241920.0, 40840800.0, 960960.0, 16380.0, 182.0, 1.0}};

// C = A B, all np x np row-major in global memory; ends with a barrier.  Wavefront w takes tiles w, w + 8, ...; lane l
// feeds A[row l & 15][k + (l >> 4)] and B[k + (l >> 4)][col l & 15]; D: row = (l >> 4) + 4 reg, col = l & 15.
__device__ __forceinline__ void model_gemm(const double *A, const double *B, double *C, int np, int tid)
{
    const int nt = np >> 4, lane = tid & 63, lm = lane & 15, lg = lane >> 4;
    for (int t = tid >> 6; t < nt * nt; t += MODEL_EXPM_THREADS / 64) {
        const int tr = t / nt, tc = t - tr * nt;
        const double *ap = A + (size_t)(tr * 16 + lm) * np + lg;
        const double *bp = B + (size_t)lg * np + tc * 16 + lm;
        v4f64 acc = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int k = 0; k < np; k += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[k], bp[(size_t)k * np], acc, 0, 0, 0);
        double *cp = C + (size_t)(tr * 16 + lg) * np + tc * 16 + lm;
#pragma unroll
        for (int q = 0; q < 4; ++q) cp[(size_t)(4 * q) * np] = acc[q];
    }
    __syncthreads();
}

// M X = R on the leading n x n parts (leading dimension np), X overwrites R, M is destroyed: imc_model::solve with the
// row operations spread over the workgroup.  false (for every thread): a zero pivot column.
__device__ __forceinline__ bool model_solve(double *M, double *R, int n, int np, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int WAVES = MODEL_EXPM_THREADS / 64;
    for (int k = 0; k < n; ++k) {
        // pivot: every wavefront finds it on its own from the same column (first row of the largest magnitude)
        double big = -1.0;
        int piv = k;
        for (int i = k + lane; i < n; i += 64) {
            const double v = fabs(M[(size_t)i * np + k]);
            if (v > big) { big = v; piv = i; }
        }
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            const double ob = __shfl_xor(big, msk, 64);
            const int op = __shfl_xor(piv, msk, 64);
            if (ob > big || (ob == big && op < piv)) { big = ob; piv = op; }
        }
        if (big == 0.0) return false;
        __syncthreads();                                   // column k has been read by everybody
        if (piv != k)
            for (int j = tid; j < 2 * n; j += MODEL_EXPM_THREADS) {
                double *X = j < n ? M : R;
                const int c = j < n ? j : j - n;
                const double x = X[(size_t)k * np + c];
                X[(size_t)k * np + c] = X[(size_t)piv * np + c];
                X[(size_t)piv * np + c] = x;
            }
        __syncthreads();
        const double inv = 1.0 / M[(size_t)k * np + k];
        const int nr = n - k - 1;                          // columns k + 1 .. n - 1 of M, then all of R
        for (int i = k + 1 + wave; i < n; i += WAVES) {
            const double f = M[(size_t)i * np + k] * inv;
            if (f == 0.0) continue;
            for (int jj = lane; jj < nr + n; jj += 64) {
                if (jj < nr) M[(size_t)i * np + k + 1 + jj] -= f * M[(size_t)k * np + k + 1 + jj];
                else R[(size_t)i * np + jj - nr] -= f * R[(size_t)k * np + jj - nr];
            }
        }
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
        const double inv = 1.0 / M[(size_t)k * np + k];
        for (int j = tid; j < n; j += MODEL_EXPM_THREADS) R[(size_t)k * np + j] *= inv;
        __syncthreads();
        for (int i = wave; i < k; i += WAVES) {
            const double f = M[(size_t)i * np + k];
            for (int j = lane; j < n; j += 64) R[(size_t)i * np + j] -= f * R[(size_t)k * np + j];
        }
        __syncthreads();
    }
    return true;
}

extern __shared__ double model_dyn_lds[];

__global__ __launch_bounds__(MODEL_EXPM_THREADS) void k_model_expm(const ModelSlot *__restrict__ slots, const double *__restrict__ Q,
                                                                   double *work, int *flags, int lds_doubles)
{
    const int tid = threadIdx.x;
    const ModelSlot sl = slots[blockIdx.x];
    const int n = sl.n, np = sl.np, m = sl.m, nn = np * np;
    double *As = work + sl.w_off, *A2 = As + nn, *A4 = A2 + nn, *A6 = A4 + nn, *A8 = A6 + nn, *U = A8 + nn, *V = U + nn,
           *Tm = V + nn, *Out = Tm + nn;
    const double *Qm = Q + sl.q_off;
    for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) {
        const int r = idx / np, c = idx - r * np;
        As[idx] = (r < n && c < n) ? Qm[(size_t)r * n + c] * sl.dt * sl.scale : 0.0;
    }
    if (tid == 0) flags[blockIdx.x] = 0;
    __syncthreads();
    const double *cf = model_pade[m == 3 ? 0 : m == 5 ? 1 : m == 7 ? 2 : m == 9 ? 3 : 4];
    if (m < 13) {
        model_gemm(As, As, A2, np, tid);
        if (m >= 5) model_gemm(A2, A2, A4, np, tid);
        if (m >= 7) model_gemm(A4, A2, A6, np, tid);
        if (m >= 9) model_gemm(A6, A2, A8, np, tid);
        // W = odd coefficients times even powers (U = A W), V = even coefficients times even powers
        for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) {
            const int r = idx / np, c = idx - r * np;
            double w = cf[3] * A2[idx], v = cf[2] * A2[idx];
            if (m >= 5) { w += cf[5] * A4[idx]; v += cf[4] * A4[idx]; }
            if (m >= 7) { w += cf[7] * A6[idx]; v += cf[6] * A6[idx]; }
            if (m >= 9) { w += cf[9] * A8[idx]; v += cf[8] * A8[idx]; }
            if (r == c && r < n) { w += cf[1]; v += cf[0]; }
            Tm[idx] = w;
            V[idx] = v;
        }
        __syncthreads();
        model_gemm(As, Tm, U, np, tid);
    } else {
        model_gemm(As, As, A2, np, tid);
        model_gemm(A2, A2, A4, np, tid);
        model_gemm(A4, A2, A6, np, tid);
        // U = As (A6 (b13 A6 + b11 A4 + b9 A2) + b7 A6 + b5 A4 + b3 A2 + b1 I)
        for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) Tm[idx] = cf[13] * A6[idx] + cf[11] * A4[idx] + cf[9] * A2[idx];
        __syncthreads();
        model_gemm(A6, Tm, V, np, tid);
        for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) {
            const int r = idx / np, c = idx - r * np;
            double v = V[idx] + (cf[7] * A6[idx] + cf[5] * A4[idx] + cf[3] * A2[idx]);
            if (r == c && r < n) v += cf[1];
            V[idx] = v;
        }
        __syncthreads();
        model_gemm(As, V, U, np, tid);
        // V = A6 (b12 A6 + b10 A4 + b8 A2) + b6 A6 + b4 A4 + b2 A2 + b0 I
        for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) Tm[idx] = cf[12] * A6[idx] + cf[10] * A4[idx] + cf[8] * A2[idx];
        __syncthreads();
        model_gemm(A6, Tm, V, np, tid);
        for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) {
            const int r = idx / np, c = idx - r * np;
            double v = V[idx] + (cf[6] * A6[idx] + cf[4] * A4[idx] + cf[2] * A2[idx]);
            if (r == c && r < n) v += cf[0];
            V[idx] = v;
        }
        __syncthreads();
    }
    // (V - U) R = V + U
    const bool in_lds = 2 * nn <= lds_doubles;
    double *Mx = in_lds ? model_dyn_lds : Tm, *Rx = in_lds ? model_dyn_lds + nn : Out;
    for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) {
        const double u = U[idx], v = V[idx];
        Mx[idx] = v - u;
        Rx[idx] = v + u;
    }
    __syncthreads();
    if (!model_solve(Mx, Rx, n, np, tid)) {
        if (tid == 0) flags[blockIdx.x] = 1;
        return;
    }
    if (in_lds) {
        for (int idx = tid; idx < nn; idx += MODEL_EXPM_THREADS) Out[idx] = Rx[idx];
        __syncthreads();
    }
    double *cur = Out, *nxt = Tm;
    for (int q = 0; q < sl.s; ++q) {
        model_gemm(cur, cur, nxt, np, tid);
        double *t = cur; cur = nxt; nxt = t;
    }
}

__global__ __launch_bounds__(256) void k_model_unpad(const ModelSlot *__restrict__ slots, const double *__restrict__ work, double *out)
{
    const ModelSlot sl = slots[blockIdx.x];
    const double *src = work + sl.r_off;
    double *dst = out + (size_t)blockIdx.x * sl.n * sl.n;
    for (int idx = threadIdx.x; idx < sl.n * sl.n; idx += 256) {
        const int r = idx / sl.n, c = idx - r * sl.n;
        dst[idx] = src[(size_t)r * sl.np + c];
    }
}

__global__ __launch_bounds__(MODEL_JOINT_THREADS) void k_model_joint(ModelJointArgs a)
{
    constexpr int TH = MODEL_JOINT_THREADS;
    __shared__ double s_begin[2][MODEL_MAX_ORDER], s_close[MODEL_MAX_ORDER], s_diag[MODEL_MAX_ORDER], s_row[MODEL_MAX_INTERVALS];
    __shared__ int s_rowB[MODEL_MAX_ORDER], s_rowL[MODEL_MAX_ORDER];
    const int tid = threadIdx.x, b = blockIdx.x, n = a.n;
    // ---- through = expm x projection where the state space changes ----
    for (int jb = a.job_off[b]; jb < a.job_off[b + 1]; ++jb) {
        const ModelProjJob jd = a.jobs[jb];
        const double *src = a.work + jd.src_off, *P = a.proj + jd.proj_off;
        double *dst = a.work + jd.dst_off;
        for (int e = tid; e < jd.rows * jd.cols; e += TH) {
            const int r = e / jd.cols, c = e - r * jd.cols;
            double s = 0.0;
            for (int k = 0; k < jd.rows; ++k) s += src[(size_t)r * jd.src_ld + k] * P[(size_t)k * jd.cols + c];
            dst[e] = s;
        }
    }
    double *J = a.T + (size_t)b * n * n;
    double *Vc = a.work + a.v_off + (size_t)b * 2 * (n - 1) * a.max_l, *Vn = Vc + (size_t)(n - 1) * a.max_l;
    {
        const int *B0 = a.cls_idx + a.cls_off[0];
        const int nb = a.cls_off[1] - a.cls_off[0];
        for (int k = tid; k < nb; k += TH) s_begin[0][k] = a.start[(size_t)b * a.s0 + B0[k]];
    }
    __syncthreads();
    for (int t = 0; t + 1 < n; ++t) {
        const double *M = a.work + a.thr_off[(size_t)b * (n - 1) + t];
        const int ld = a.thr_ld[(size_t)b * (n - 1) + t], cur = t & 1;
        const int *Bt = a.cls_idx + a.cls_off[3 * t], *Lt = a.cls_idx + a.cls_off[3 * t + 1];
        const int nb = a.cls_off[3 * t + 1] - a.cls_off[3 * t], nl = a.cls_off[3 * t + 2] - a.cls_off[3 * t + 1];
        const int *Bn = a.cls_idx + a.cls_off[3 * t + 3], *Ln = a.cls_idx + a.cls_off[3 * t + 4], *En = a.cls_idx + a.cls_off[3 * t + 5];
        const int nb1 = a.cls_off[3 * t + 4] - a.cls_off[3 * t + 3], nl1 = a.cls_off[3 * t + 5] - a.cls_off[3 * t + 4],
                  nen = a.cls_off[3 * t + 6] - a.cls_off[3 * t + 5];
        // (the i = 0 diagonal term applies interval 0's E indices to the columns of through_0, as the reference does)
        const int *Ed = t == 0 ? a.cls_idx + a.cls_off[2] : En;
        const int ned = t == 0 ? a.cls_off[3] - a.cls_off[2] : nen;
        // phase 1: per-row end sums (diagonal terms and the closing vector), row offsets of the B and L classes
        for (int k = tid; k < nb; k += TH) {
            const double *row = M + (size_t)Bt[k] * ld;
            double r = 0.0;
            for (int e = 0; e < ned; ++e) r += row[Ed[e]];
            s_diag[k] = s_begin[cur][k] * r;
            s_rowB[k] = Bt[k] * ld;
        }
        if (t >= 1)
            for (int k = tid; k < nl; k += TH) {
                const double *row = M + (size_t)Lt[k] * ld;
                double s = 0.0;
                for (int e = 0; e < nen; ++e) s += row[En[e]];
                s_close[k] = s;
                s_rowL[k] = Lt[k] * ld;
            }
        __syncthreads();
        // phase 2: everything of this interval reads begin_t, V and the sums above, and writes begin_{t+1}, V' and J
        if (tid == TH - 1) {
            double s = 0.0;
            for (int k = 0; k < nb; ++k) s += s_diag[k];
            J[(size_t)t * n + t] = s;
        }
        for (int c = tid; c < nb1 + nl1; c += TH) {          // begin_{t+1} and row t of V' = begin_t through_t[B, L_{t+1}]
            const int col = c < nb1 ? Bn[c] : Ln[c - nb1];
            double s = 0.0;
            for (int k = 0; k < nb; ++k) s += s_begin[cur][k] * M[s_rowB[k] + col];
            if (c < nb1) s_begin[cur ^ 1][c] = s;
            else Vn[(size_t)t * nl1 + c - nb1] = s;
        }
        if (t >= 1) {
            for (int i = tid; i < t; i += TH) {
                const double *v = Vc + (size_t)i * nl;
                double s = 0.0;
                for (int k = 0; k < nl; ++k) s += v[k] * s_close[k];
                J[(size_t)i * n + t] = s;
            }
            for (int e = tid; e < t * nl1; e += TH) {
                const int i = e / nl1, c = e - i * nl1, col = Ln[c];
                const double *v = Vc + (size_t)i * nl;
                double s = 0.0;
                for (int k = 0; k < nl; ++k) s += v[k] * M[s_rowL[k] + col];
                Vn[e] = s;
            }
        }
        __syncthreads();
        double *sw = Vc; Vc = Vn; Vn = sw;
    }
    {   // the last interval's pseudo through matrix: every B state stays, every L state ends in E
        const int t = n - 1, cur = t & 1;
        const int nb = a.cls_off[3 * t + 1] - a.cls_off[3 * t], nl = a.cls_off[3 * t + 2] - a.cls_off[3 * t + 1];
        if (tid == TH - 1) {
            double s = 0.0;
            for (int k = 0; k < nb; ++k) s += s_begin[cur][k];
            J[(size_t)t * n + t] = s;
        }
        for (int i = tid; i < t; i += TH) {
            double s = 0.0;
            for (int k = 0; k < nl; ++k) s += Vc[(size_t)i * nl + k];
            J[(size_t)i * n + t] = s;
        }
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += TH) {
        const int i = e / n, j = e - i * n;
        if (j < i) J[e] = J[(size_t)j * n + i];
    }
    __syncthreads();
    for (int i = tid; i < n; i += TH) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += J[(size_t)i * n + j];
        s_row[i] = s;
        a.pi[(size_t)b * n + i] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += s_row[i];
        a.total[b] = s;
    }
    for (int e = tid; e < n * n; e += TH) J[e] = J[e] / s_row[e / n];
}
