// engine_core.hpp - what the rest of the engine stands on: the error text and HIP_TRY, the library's lock (g_mu, g_cv),
// device memory (dev_alloc / dev_free with the guard ranges of IMC_GUARD=1, DevBuf), DictDev, the context `g` with
// ensure_ctx(), the device switches, and the two handles of the C ABI (imc_obs, imc_aln).  Three things stand here because
// they stood in this block and the move is verbatim: the using-declarations of the planner's constants ("this file" in their
// comment is the engine as a whole), STAGE_KERNEL_MAX_BYTES, which only enqueue reads, and g_cv, which Plan::busy explains.
// Needs: the HIP runtime, include/imcoal_fwd.h, options_host.hpp and pair_dict.hpp, included by imcoal_fwd.hip before it.
// Lock: ensure_ctx(), device_mode() and dev_alloc() read the context and expect g_mu held; set_device_mode() takes it.
// Part of imcoal_fwd.hip's one translation unit, included there once; the ABI itself is in imcoal_fwd.hip.
#pragma once

static_assert(sizeof(imc::Desc4) == sizeof(int4) && alignof(imc::Desc4) == alignof(int4), "descriptor entries are uploaded as int4");

namespace {

thread_local std::string g_err;
std::mutex g_mu;
std::condition_variable g_cv;   // signalled when a plan stops being busy (see Plan::busy)

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return fail(_e == hipErrorOutOfMemory ? IMC_ERR_OOM : IMC_ERR_HIP,                          \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                             \
    } while (0)

// the planner's constants and helpers that the rest of this file uses too (planner_host.hpp)
using imc::HYBRID_MAX_ALPHABET;
using imc::LDS_BUDGET;
using imc::Z2GRAN;
using imc::round_up;

constexpr size_t STAGE_KERNEL_MAX_BYTES = 1u << 20;   // parameter sets up to this size are fetched by k_stage_params (enqueue)

// ---- device memory -----------------------------------------------------------------------------------
// Every device buffer of the library comes from here.  Normal mode: hipMalloc / hipFree.  Guard mode (IMC_GUARD=1, a
// test facility): each buffer is its own virtual-memory reservation with NO mapping behind its last 16-byte unit, so
// a kernel that reads or writes even one vector load past a buffer's declared size faults deterministically instead of
// silently touching whatever the allocator happened to place next (tests/test_gpu_guard.py runs the create / free /
// compression-flip / create sequence of round 1's unexplained fault this way).  dev_free stands here, in front of DictDev, whose
// destructor calls it; dev_alloc reads the context and follows ensure_ctx().
struct GuardRec { hipDeviceptr_t va; size_t va_size; hipMemGenericAllocationHandle_t handle; hipDeviceptr_t map; size_t map_size; };
// (never destroyed: the context `g` - whose dictionaries free device buffers in their destructors - outlives every
// other static at process exit, and dev_free must still find the guard records then; a plain static map is destroyed
// first and the lookup walked freed nodes: "malloc_consolidate(): invalid chunk size" at exit under IMC_GUARD=1)
std::map<void *, GuardRec> &g_guard = *new std::map<void *, GuardRec>();

void dev_free(void *p)
{
    if (!p) return;
    auto it = g_guard.find(p);
    if (it == g_guard.end()) { (void)hipFree(p); return; }
    (void)hipDeviceSynchronize();
    (void)hipMemUnmap(it->second.map, it->second.map_size);
    (void)hipMemRelease(it->second.handle);
    // The address range is NOT given back (hipMemAddressFree): a freed guard buffer stays unmapped for the rest of the
    // process, so a use after free faults too - and no later buffer can be mapped at an address some CU may still hold a
    // translation for.  (Round 3: with the ranges recycled, a Forwarder created right after another had been freed
    // sometimes evaluated to a wrong value in every plan - 3 of 4 processes, under IMC_GUARD=1 only, never with hipMalloc -
    // and a later launch faulted at an address nobody had computed; with the ranges kept, neither was seen again.)
    g_guard.erase(it);
}

struct DictDev : imc::TrainedDict {                // one trained dictionary (dict, depth, order: pair_dict.hpp) + its device copy
    uint16_t *d_left = nullptr, *d_right = nullptr;
    uint16_t *d_order = nullptr;                   // device copy of order
    uint64_t trained_on = 0;                       // columns of the chunk(s) the training sample was drawn from
    pid_t pid = 0;
    DictDev(imc::TrainedDict t, uint64_t columns) : imc::TrainedDict(std::move(t)), trained_on(columns) {}
    ~DictDev()
    {
        if (pid == getpid()) { dev_free(d_left); dev_free(d_right); dev_free(d_order); }
    }
};

struct Ev3 { hipEvent_t a, b, c; };   // a: before propagate, b: after propagate, c: after stitch

struct Ctx {
    pid_t pid = 0;
    int device = -1;          // -1: use the thread's current device at first use
    bool ready = false;
    hipStream_t stream = nullptr;
    int cus = 256;
    uint64_t next_obs_id = 1, next_dict_id = 1;
    imc::Options opt;         // the knobs (options_host.hpp): set by the ABI's setters and by the table of variables
    bool profile = false;
    std::vector<Ev3> events;
    std::map<int, std::shared_ptr<DictDev>> dicts;   // by raw alphabet size
    uint64_t last_plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t last_ingest[4] = {0, 0, 0, 0};      // imc_last_ingest: path, bytes sent to the device, slabs, columns
    uint64_t last_training[4] = {0, 0, 0, 0};    // imc_last_training: path, symbols in the sample, byte-phase attempts, 16-bit rounds
    uint64_t r1_checked = 0, r1_collapsed = 0;   // last call: operator segments tested / certified rank one
    std::string last_kernels;   // propagate kernels of the last enqueue, e.g. "k_zpropagate2<5>[tokens]"
    std::vector<const void *> lds_opted;   // kernels of this device that may use LDS_BUDGET bytes of dynamic LDS (allow_lds_budget)
} g;

int ensure_ctx()
{
    const pid_t me = getpid();
    if (g.ready && g.pid == me) return IMC_OK;
    if (g.ready && g.pid != me)
        // A forked child of a process that had already used the GPU: the parent's HIP state (context, streams, every
        // device pointer held by cached plans and dictionaries) is not usable here and HIP cannot be re-initialised
        // after fork().  Refuse instead of guessing; nothing of the parent's is freed or touched.  Children that
        // build their own Forwarders (mcmc.py:112-121) must be forked BEFORE the parent's first library call.
        return fail(IMC_ERR_HIP, "libimcoal_fwd was initialised in the parent process before fork(): fork the chain "
                                 "processes before the first imc_* call of the parent, or use the spawn start method");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(IMC_ERR_NODEVICE, "no HIP device available (libimcoal_fwd has no CPU fallback)");
    if (g.device < 0) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) cur = 0;
        g.device = cur;
    }
    if (g.device >= n) return fail(IMC_ERR_NODEVICE, "requested device index out of range");
    HIP_TRY(hipSetDevice(g.device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, g.device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(IMC_ERR_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    g.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    imc::read_options(g.opt, imc::ReadAt::Context, imc::process_env);
    g.pid = me;
    g.ready = true;
    return IMC_OK;
}

// A device switch of the record (device_encode, device_ingest, device_train; g_mu held, no device needed): its variable
// decides until the API has set it.
int device_mode(int imc::Options::*field) { return imc::device_switch(g.opt, field, imc::process_env); }

// ... and its setter (imc_set_device_encoding / _ingest / _training; takes g_mu): 0 or 1, anything else is `refusal`.
int set_device_mode(int imc::Options::*field, int mode, const char *refusal)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (mode != 0 && mode != 1) return fail(IMC_ERR_ARG, refusal);
    g.opt.*field = mode;
    return IMC_OK;
}

// (device memory, continued)
hipError_t dev_alloc(void **p, size_t bytes)
{
    bytes = std::max<size_t>(bytes, 16);
    if (!g.opt.guard) return hipMalloc(p, bytes);
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = g.device;
    size_t gran = 0;
    hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
    if (e != hipSuccess || gran == 0) return e != hipSuccess ? e : hipErrorUnknown;
    GuardRec r{};
    r.map_size = (bytes + gran - 1) / gran * gran;
    r.va_size = r.map_size + 2 * gran;              // one unmapped granule before, one after
    e = hipMemAddressReserve(&r.va, r.va_size, gran, nullptr, 0);
    if (e != hipSuccess) return e;
    e = hipMemCreate(&r.handle, r.map_size, &prop, 0);
    if (e != hipSuccess) { (void)hipMemAddressFree(r.va, r.va_size); return e; }
    r.map = (hipDeviceptr_t)((char *)r.va + gran);
    e = hipMemMap(r.map, r.map_size, 0, r.handle, 0);
    if (e == hipSuccess) {
        hipMemAccessDesc ad{};
        ad.location = prop.location;
        ad.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(r.map, r.map_size, &ad, 1);
        if (e != hipSuccess) (void)hipMemUnmap(r.map, r.map_size);
    }
    if (e != hipSuccess) { (void)hipMemRelease(r.handle); (void)hipMemAddressFree(r.va, r.va_size); return e; }
    void *user = (char *)r.map + (r.map_size - (bytes + 15) / 16 * 16);   // the buffer's end is the mapping's end
    g_guard[user] = r;
    *p = user;
    return hipSuccess;
}

// One device buffer and its owner: allocated by dev_alloc (so guard mode applies), freed by dev_free when the owner
// is destroyed, re-assigned or reset().  Every device pointer of Plan, Level and Group is one of these, so erasing a
// plan releases it.  NOT used for imc_obs (its token levels alias each other, and it checks the process id before it
// frees), DictDev (its destructor runs at exit behind the same process-id check) and g_model (a static whose buffers
// are released explicitly): those keep raw pointers.
template <class T>
class DevBuf {
    T *p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t bytes)
    {
        reset();
        return dev_alloc((void **)&p_, bytes);
    }
    void reset()
    {
        dev_free(p_);
        p_ = nullptr;
    }
    T *get() const { return p_; }
    T *release()                  // the caller owns the buffer from now on (dev_free)
    {
        T *p = p_;
        p_ = nullptr;
        return p;
    }
    explicit operator bool() const { return p_ != nullptr; }
};

}  // namespace

struct imc_obs {
    uint64_t id = 0;
    pid_t pid = 0;
    int device = 0;
    int nsym = 0;
    size_t L = 0;
    uint8_t *d_sym = nullptr;              // L raw symbols + zero padding (bytes, or 16-bit values when wide_raw)
    bool wide_raw = false;                 // raw alphabet beyond 256 symbols
    std::shared_ptr<DictDev> dict;         // null: not compressed
    uint8_t *d_tok[imc::kNumLevels] = {};  // token streams per level (aliases allowed), null if none
    bool owns[imc::kNumLevels] = {};       // ... in a buffer of the level's own: release_tokens() frees exactly these
    bool wide[imc::kNumLevels] = {};       // ... holding 16-bit ids (alphabets beyond 256)
    size_t ntok[imc::kNumLevels] = {};
    int alphabet[imc::kNumLevels] = {};
    std::vector<uint32_t> tok_count[imc::kNumLevels];   // byte levels: occurrences of every token id (hot-set choice of the hybrid table)
};

// An alignment whose sequences are resident on the device: all records' bases back to back in one buffer (not word
// aligned), names and the record table on the host.
struct imc_aln {
    pid_t pid = 0;
    int device = 0;
    std::vector<std::string> names;
    std::vector<uint64_t> start, length;   // of every record, in bytes of d_bases
    uint8_t *d_bases = nullptr;            // the file's size rounded up to 16 (device parser) / the bases' (host reader)
    uint64_t info[4] = {0, 0, 0, 0};       // imc_aln_info
};
