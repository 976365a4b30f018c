// engine_model.hpp - (pi, T) of a population on the device: the host side of kernels_model.hpp.
// Needs: engine_core.hpp; kernels_model.hpp, model_host.hpp, include/imcoal_model.h.
// Lock: the argument checks make no HIP call and need none; the device functions expect g_mu held and the context ready, and
// are synchronous on the library's stream.
#pragma once

// =====================================================================================================
// (pi, T) of a population on the device: host side of csrc/kernels_model.hpp (include/imcoal_model.h)
// =====================================================================================================
namespace {

constexpr size_t MODEL_WORK_CAP = (size_t)256 << 20;   // bytes of work matrices per launch: larger populations go in rounds
constexpr int MODEL_LDS_ORDER = 96;                    // the solve's M and R both fit LDS up to this padded order (2 x 72 KiB)

// The three device buffers of the model path (uploads, work matrices, results): kept between calls, only ever grown.
// Under IMC_GUARD=1 a buffer is re-made at exactly the size a launch needs, so that its end is the guard range's start.
struct ModelBuf { void *p = nullptr; size_t cap = 0; };
struct ModelDev { ModelBuf in, work, out; bool attr_set = false; } g_model;

hipError_t model_reserve(ModelBuf &b, size_t bytes)
{
    bytes = round_up(std::max<size_t>(bytes, 16), 16);
    if (g.opt.guard ? b.cap == bytes : b.cap >= bytes) return hipSuccess;
    dev_free(b.p);
    b.p = nullptr;
    b.cap = 0;
    const hipError_t e = dev_alloc(&b.p, bytes);
    if (e == hipSuccess) b.cap = bytes;
    return e;
}

struct ModelBlob {                                     // one upload: sections at 16-byte boundaries
    std::vector<char> bytes;
    template <class V> size_t put(const V *src, size_t count)
    {
        const size_t off = round_up(bytes.size(), 16);
        bytes.resize(off + count * sizeof(V));
        if (count) std::memcpy(bytes.data() + off, src, count * sizeof(V));
        return off;
    }
};

// Pade degree and squarings of one slot from the 1-norm of Q dt - the numbers imc_model::expm would see
void model_plan_slot(ModelSlot &sl, const double *Qm)
{
    const int n = sl.n;
    double best = 0.0;
    for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += std::fabs(Qm[(size_t)i * n + j] * sl.dt);
        best = std::max(best, s);
    }
    imc_model::expm_plan(best, sl.m, sl.s);
    sl.scale = std::ldexp(1.0, -sl.s);
}

int model_launch_expm(const ModelSlot *d_slots, int n_slots, const double *d_Q, double *d_work, int *d_flags, int lds_np)
{
    if (!g_model.attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void *)k_model_expm, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    2 * MODEL_LDS_ORDER * MODEL_LDS_ORDER * 8));
        g_model.attr_set = true;
    }
    const int lds_doubles = 2 * lds_np * lds_np;
    hipLaunchKernelGGL(k_model_expm, dim3((unsigned)n_slots), dim3(MODEL_EXPM_THREADS), (size_t)lds_doubles * 8, g.stream, d_slots, d_Q,
                       d_work, d_flags, lds_doubles);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

// The argument checks of imc_model_transitions and imc_model_transitions_device (`fn` prefixes the messages): null
// pointers, counts, piece and class indices; fills the offsets of the rate matrices inside one system's Q block.
int model_check_args(const char *fn, int n_systems, int n_intervals, const int32_t *space_size, const int32_t *cls_off,
                     const int32_t *cls_idx, const int32_t *piece_q, const int32_t *piece_proj, int n_q, const int32_t *q_size, int n_proj,
                     const int32_t *proj_off, const double *proj, const double *Q, const double *dt, const double *start,
                     const double *pi, const double *T, std::vector<int32_t> &q_off, int &stride)
{
    const std::string who = std::string(fn) + ": ";
    if (n_systems < 0 || n_intervals < 1 || n_q < 1 || !space_size || !cls_off || !cls_idx || !q_size || !Q || !start || !pi || !T ||
        (n_intervals > 1 && (!piece_q || !piece_proj || !dt)))
        return fail(IMC_ERR_ARG, who + "bad arguments");
    q_off.assign((size_t)n_q, 0);
    stride = 0;
    for (int k = 0; k < n_q; ++k) {
        if (q_size[k] < 1) return fail(IMC_ERR_ARG, who + "rate matrix of order < 1");
        q_off[k] = stride;
        stride += q_size[k] * q_size[k];
    }
    for (int i = 0; i + 1 < n_intervals; ++i) {
        if (piece_q[i] < 0 || piece_q[i] >= n_q || piece_proj[i] >= n_proj || (piece_proj[i] >= 0 && (!proj || !proj_off)))
            return fail(IMC_ERR_ARG, who + "piece index out of range");
    }
    if (cls_off[0] < 0) return fail(IMC_ERR_ARG, who + "class offsets must not decrease");
    for (int i = 0; i < n_intervals; ++i) {
        for (int k = 0; k < 3; ++k)
            if (cls_off[3 * i + k + 1] < cls_off[3 * i + k]) return fail(IMC_ERR_ARG, who + "class offsets must not decrease");
        for (int k = cls_off[3 * i]; k < cls_off[3 * i + 3]; ++k)
            if (cls_idx[k] < 0 || cls_idx[k] >= space_size[i]) return fail(IMC_ERR_ARG, who + "class index outside its state space");
    }
    return IMC_OK;
}

// On top of model_check_args: the limits of the device kernels, and the per-system checks that
// imc_model::transitions_one makes on the way (same messages) - all of it before the first HIP call.
int model_check_device_args(int n_systems, int n_intervals, const int32_t *space_size, const int32_t *cls_off, const int32_t *cls_idx,
                            const int32_t *piece_q, const int32_t *piece_proj, int n_q, const int32_t *q_size, int n_proj,
                            const int32_t *proj_off, const double *proj, const double *Q, const double *dt, const double *start,
                            const double *pi, const double *T, std::vector<int32_t> &q_off, int &stride)
{
    const std::string who = "imc_model_transitions_device: ";
    if (int rc = model_check_args("imc_model_transitions_device", n_systems, n_intervals, space_size, cls_off, cls_idx, piece_q, piece_proj,
                                  n_q, q_size, n_proj, proj_off, proj, Q, dt, start, pi, T, q_off, stride))
        return rc;
    if (n_intervals > MODEL_MAX_INTERVALS) return fail(IMC_ERR_ARG, who + "more than " + std::to_string(MODEL_MAX_INTERVALS) + " intervals");
    for (int k = 0; k < n_q; ++k)
        if (q_size[k] > MODEL_MAX_ORDER)
            return fail(IMC_ERR_ARG, who + "rate matrix of order " + std::to_string(q_size[k]) + " exceeds " + std::to_string(MODEL_MAX_ORDER));
    for (int i = 0; i < n_intervals; ++i)
        if (space_size[i] < 1 || space_size[i] > MODEL_MAX_ORDER)
            return fail(IMC_ERR_ARG, who + "state space of order " + std::to_string(space_size[i]) + " outside [1," + std::to_string(MODEL_MAX_ORDER) + "]");
    for (int i = 0; i + 1 < n_intervals; ++i)
        if (piece_proj[i] >= 0 && proj_off[piece_proj[i]] < 0) return fail(IMC_ERR_ARG, who + "negative projection offset");
    for (int k = 0; k < 3 * n_intervals; ++k)
        if (cls_off[k + 1] - cls_off[k] > MODEL_MAX_ORDER) return fail(IMC_ERR_ARG, who + "a class lists more than " + std::to_string(MODEL_MAX_ORDER) + " states");
    for (int i = 0; i + 1 < n_intervals; ++i) {
        if (q_size[piece_q[i]] != space_size[i]) return fail(IMC_ERR_ARG, "a rate matrix does not match its interval's state space");
        if (piece_proj[i] < 0 && space_size[i + 1] != space_size[i]) return fail(IMC_ERR_ARG, "state space changes without a projection");
    }
    if (n_intervals > 1)
        for (int k = cls_off[2]; k < cls_off[3]; ++k)
            if (cls_idx[k] >= space_size[1]) return fail(IMC_ERR_ARG, "an end-state index exceeds the next interval's state space");
    const int s0 = space_size[0];
    std::vector<char> inB((size_t)s0, 0);
    for (int k = cls_off[0]; k < cls_off[1]; ++k) inB[cls_idx[k]] = 1;
    for (int b = 0; b < n_systems; ++b)
        for (int k = 0; k < s0; ++k)
            if (!inB[k] && start[(size_t)b * s0 + k] != 0.0) return fail(IMC_ERR_ARG, "the start distribution must be supported on the B class");
    return IMC_OK;
}

struct ModelSysPlan {                 // one system: its slots (distinct (rate matrix, dt)) and projected through matrices
    std::vector<ModelSlot> slots;     // q_off: inside the system's Q block; w_off / r_off: set per round
    std::vector<int> slot_q;          // which rate matrix
    std::vector<std::pair<int, int>> jobs;   // (slot, projection)
    std::vector<int> piece_slot, piece_job;  // per interval but the last; piece_job -1: the exponential itself
    size_t work_doubles = 0;
};

int model_transitions_device(int n_systems, int n, const int32_t *space_size, const int32_t *cls_off, const int32_t *cls_idx,
                             const int32_t *piece_q, const int32_t *piece_proj, const int32_t *q_size, const std::vector<int32_t> &q_off,
                             int stride, const int32_t *proj_off, const double *proj, const double *Q, const double *dt,
                             const double *start, double *pi, double *T)
{
    const int np1 = n - 1, s0 = space_size[0];
    int max_l = 1;
    for (int i = 0; i < n; ++i) max_l = std::max(max_l, (int)(cls_off[3 * i + 2] - cls_off[3 * i + 1]));
    size_t proj_doubles = 0;
    for (int i = 0; i < np1; ++i)
        if (piece_proj[i] >= 0) proj_doubles = std::max(proj_doubles, (size_t)proj_off[piece_proj[i]] + (size_t)space_size[i] * space_size[i + 1]);
    // ---- plan every system: slots de-duplicated on (rate matrix, dt) as transitions_one does, degree and squarings per slot ----
    std::vector<ModelSysPlan> plans((size_t)n_systems);
    for (int b = 0; b < n_systems; ++b) {
        ModelSysPlan &sp = plans[b];
        const double *dtb = dt + (size_t)b * np1;
        sp.piece_slot.assign((size_t)np1, -1);
        sp.piece_job.assign((size_t)np1, -1);
        for (int i = 0; i < np1; ++i) {
            int k = -1;
            for (size_t c = 0; c < sp.slots.size() && k < 0; ++c)
                if (sp.slot_q[c] == piece_q[i] && sp.slots[c].dt == dtb[i]) k = (int)c;
            if (k < 0) {
                ModelSlot sl{};
                sl.n = q_size[piece_q[i]];
                sl.np = (sl.n + 15) / 16 * 16;
                sl.dt = dtb[i];
                sl.q_off = q_off[piece_q[i]];
                model_plan_slot(sl, Q + (size_t)b * stride + q_off[piece_q[i]]);
                k = (int)sp.slots.size();
                sp.slots.push_back(sl);
                sp.slot_q.push_back(piece_q[i]);
                sp.work_doubles += (size_t)MODEL_MATS * sl.np * sl.np;
            }
            sp.piece_slot[i] = k;
            if (piece_proj[i] >= 0) {
                int j = -1;
                for (size_t c = 0; c < sp.jobs.size() && j < 0; ++c)
                    if (sp.jobs[c].first == k && sp.jobs[c].second == piece_proj[i]) j = (int)c;
                if (j < 0) {
                    j = (int)sp.jobs.size();
                    sp.jobs.emplace_back(k, piece_proj[i]);
                    sp.work_doubles += (size_t)space_size[i] * space_size[i + 1];
                }
                sp.piece_job[i] = j;
            }
        }
        sp.work_doubles += (size_t)2 * np1 * max_l;
    }
    HIP_TRY(hipSetDevice(g.device));
    for (int b0 = 0; b0 < n_systems;) {
        // ---- one round: as many systems as the work cap takes (at least one) ----
        int b1 = b0;
        size_t work_doubles = 0;
        while (b1 < n_systems && (b1 == b0 || (work_doubles + plans[b1].work_doubles) * 8 <= MODEL_WORK_CAP)) work_doubles += plans[b1++].work_doubles;
        const int ns = b1 - b0;
        std::vector<ModelSlot> slots;
        std::vector<ModelProjJob> jobs;
        std::vector<int> job_off((size_t)ns + 1, 0), thr_ld((size_t)ns * np1 + 1, 0);
        std::vector<long long> thr_off((size_t)ns * np1 + 1, 0);
        long long off = 0;
        int lds_np = 0;
        for (int b = b0; b < b1; ++b) {
            const ModelSysPlan &sp = plans[b];
            const size_t first_slot = slots.size(), first_job = jobs.size();
            for (ModelSlot sl : sp.slots) {
                sl.q_off += (long long)(b - b0) * stride;
                sl.w_off = off;
                sl.r_off = off + (long long)((sl.s & 1) ? MODEL_MAT_TM : MODEL_MAT_OUT) * sl.np * sl.np;
                off += (long long)MODEL_MATS * sl.np * sl.np;
                if (sl.np <= MODEL_LDS_ORDER) lds_np = std::max(lds_np, sl.np);
                slots.push_back(sl);
            }
            std::vector<int> job_cols(sp.jobs.size(), 0);
            for (int i = 0; i < np1; ++i) {
                const ModelSlot &sl = slots[first_slot + sp.piece_slot[i]];
                const int j = sp.piece_job[i];
                if (j >= 0 && first_job + j >= jobs.size()) {       // (jobs were numbered in order of first use)
                    ModelProjJob jd{};
                    jd.src_off = sl.r_off;
                    jd.src_ld = sl.np;
                    jd.rows = space_size[i];
                    jd.cols = space_size[i + 1];
                    jd.proj_off = proj_off[piece_proj[i]];
                    jd.dst_off = off;
                    off += (long long)jd.rows * jd.cols;
                    jobs.push_back(jd);
                }
                thr_off[(size_t)(b - b0) * np1 + i] = j < 0 ? sl.r_off : jobs[first_job + j].dst_off;
                thr_ld[(size_t)(b - b0) * np1 + i] = j < 0 ? sl.np : jobs[first_job + j].cols;
            }
            job_off[(size_t)(b - b0) + 1] = (int)jobs.size();
        }
        const long long v_off = off;
        off += (long long)ns * 2 * np1 * max_l;
        const int n_slots = (int)slots.size();
        // ---- upload ----
        ModelBlob blob;
        const size_t o_space = blob.put(space_size, (size_t)n), o_coff = blob.put(cls_off, (size_t)3 * n + 1),
                     o_cidx = blob.put(cls_idx, (size_t)cls_off[3 * n]), o_proj = blob.put(proj, proj_doubles),
                     o_start = blob.put(start + (size_t)b0 * s0, (size_t)ns * s0), o_slots = blob.put(slots.data(), slots.size()),
                     o_toff = blob.put(thr_off.data(), thr_off.size()), o_tld = blob.put(thr_ld.data(), thr_ld.size()),
                     o_jobs = blob.put(jobs.data(), jobs.size()), o_joff = blob.put(job_off.data(), job_off.size());
        const size_t o_Q = round_up(blob.bytes.size(), 16), q_bytes = (size_t)ns * stride * 8;
        const size_t o_pi = round_up((size_t)ns * n * n * 8, 16), o_total = round_up(o_pi + (size_t)ns * n * 8, 16),
                     o_flags = round_up(o_total + (size_t)ns * 8, 16), out_bytes = o_flags + (size_t)std::max(n_slots, 1) * 4;
        HIP_TRY(model_reserve(g_model.in, o_Q + q_bytes));
        HIP_TRY(model_reserve(g_model.work, (size_t)std::max<long long>(off, 2) * 8));
        HIP_TRY(model_reserve(g_model.out, out_bytes));
        char *d_in = (char *)g_model.in.p, *d_out = (char *)g_model.out.p;
        double *d_work = (double *)g_model.work.p;
        HIP_TRY(hipMemcpyAsync(d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(d_in + o_Q, Q + (size_t)b0 * stride, q_bytes, hipMemcpyHostToDevice, g.stream));
        // ---- exponentials (one workgroup per slot), then projection + recursion (one workgroup per system) ----
        if (n_slots > 0)
            if (int rc = model_launch_expm((const ModelSlot *)(d_in + o_slots), n_slots, (const double *)(d_in + o_Q), d_work,
                                           (int *)(d_out + o_flags), lds_np))
                return rc;
        ModelJointArgs ja{};
        ja.n = n; ja.s0 = s0; ja.max_l = max_l;
        ja.space_size = (const int *)(d_in + o_space); ja.cls_off = (const int *)(d_in + o_coff); ja.cls_idx = (const int *)(d_in + o_cidx);
        ja.proj = (const double *)(d_in + o_proj); ja.start = (const double *)(d_in + o_start);
        ja.thr_off = (const long long *)(d_in + o_toff); ja.thr_ld = (const int *)(d_in + o_tld);
        ja.jobs = (const ModelProjJob *)(d_in + o_jobs); ja.job_off = (const int *)(d_in + o_joff);
        ja.work = d_work; ja.v_off = v_off;
        ja.T = (double *)d_out; ja.pi = (double *)(d_out + o_pi); ja.total = (double *)(d_out + o_total);
        hipLaunchKernelGGL(k_model_joint, dim3((unsigned)ns), dim3(MODEL_JOINT_THREADS), 0, g.stream, ja);
        HIP_TRY(hipGetLastError());
        // ---- results ----
        std::vector<double> totals((size_t)ns);
        std::vector<int> flags((size_t)std::max(n_slots, 1), 0);
        HIP_TRY(hipMemcpyAsync(T + (size_t)b0 * n * n, d_out, (size_t)ns * n * n * 8, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(pi + (size_t)b0 * n, d_out + o_pi, (size_t)ns * n * 8, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(totals.data(), d_out + o_total, (size_t)ns * 8, hipMemcpyDeviceToHost, g.stream));
        if (n_slots > 0) HIP_TRY(hipMemcpyAsync(flags.data(), d_out + o_flags, (size_t)n_slots * 4, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        for (int f : flags)
            if (f) return fail(IMC_ERR_ARG, "expm: singular Pade denominator");
        for (int b = 0; b < ns; ++b)
            if (!(std::fabs(totals[b] - 1.0) < 1.5e-7))            // transitions.py:237, as imc_model::transitions_one
                return fail(IMC_ERR_ARG, "joint probabilities sum to " + std::to_string(totals[b]) + ", not 1 (system " + std::to_string(b0 + b) + ")");
        b0 = b1;
    }
    return IMC_OK;
}

int model_expm_batch_device(int n, int count, const double *A, double *out)
{
    const int np = (n + 15) / 16 * 16;
    const size_t nn = (size_t)n * n, slot_doubles = (size_t)MODEL_MATS * np * np;
    const int per_round = (int)std::max<size_t>(1, MODEL_WORK_CAP / 8 / slot_doubles);
    HIP_TRY(hipSetDevice(g.device));
    for (int r0 = 0; r0 < count; r0 += per_round) {
        const int nr = std::min(per_round, count - r0);
        std::vector<ModelSlot> slots((size_t)nr);
        for (int k = 0; k < nr; ++k) {
            ModelSlot &sl = slots[k];
            sl = ModelSlot{};
            sl.n = n;
            sl.np = np;
            sl.dt = 1.0;
            sl.q_off = (long long)k * nn;
            model_plan_slot(sl, A + (size_t)(r0 + k) * nn);
            sl.w_off = (long long)k * slot_doubles;
            sl.r_off = sl.w_off + (long long)((sl.s & 1) ? MODEL_MAT_TM : MODEL_MAT_OUT) * np * np;
        }
        ModelBlob blob;
        const size_t o_slots = blob.put(slots.data(), slots.size());
        const size_t o_Q = round_up(blob.bytes.size(), 16), q_bytes = (size_t)nr * nn * 8;
        const size_t o_flags = round_up(q_bytes, 16), out_bytes = o_flags + (size_t)nr * 4;
        HIP_TRY(model_reserve(g_model.in, o_Q + q_bytes));
        HIP_TRY(model_reserve(g_model.work, (size_t)nr * slot_doubles * 8));
        HIP_TRY(model_reserve(g_model.out, out_bytes));
        char *d_in = (char *)g_model.in.p, *d_out = (char *)g_model.out.p;
        HIP_TRY(hipMemcpyAsync(d_in, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(d_in + o_Q, A + (size_t)r0 * nn, q_bytes, hipMemcpyHostToDevice, g.stream));
        if (int rc = model_launch_expm((const ModelSlot *)(d_in + o_slots), nr, (const double *)(d_in + o_Q), (double *)g_model.work.p,
                                       (int *)(d_out + o_flags), np <= MODEL_LDS_ORDER ? np : 0))
            return rc;
        hipLaunchKernelGGL(k_model_unpad, dim3((unsigned)nr), dim3(256), 0, g.stream, (const ModelSlot *)(d_in + o_slots),
                           (const double *)g_model.work.p, (double *)d_out);
        HIP_TRY(hipGetLastError());
        std::vector<int> flags((size_t)nr, 0);
        HIP_TRY(hipMemcpyAsync(out + (size_t)r0 * nn, d_out, q_bytes, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(flags.data(), d_out + o_flags, (size_t)nr * 4, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        for (int k = 0; k < nr; ++k)
            if (flags[k]) return fail(IMC_ERR_ARG, "imc_model_expm_batch_device: singular Pade denominator (matrix " + std::to_string(r0 + k) + ")");
    }
    return IMC_OK;
}

void model_release()
{
    for (ModelBuf *b : {&g_model.in, &g_model.work, &g_model.out}) {
        dev_free(b->p);
        b->p = nullptr;
        b->cap = 0;
    }
    g_model.attr_set = false;
}

}  // namespace
