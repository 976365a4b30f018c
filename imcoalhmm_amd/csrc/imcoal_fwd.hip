// imcoal_fwd.hip - MI355X (gfx950 / CDNA4) HMM forward log-likelihood engine behind the C ABI of
// include/imcoal_fwd.h.  Replaces ziphmm.preprocess_raw_observations / ziphmm.zip_forward as called
// from the reference at src/IMCoalHMM/hmm.py:16,20-21 and the sum at likelihood.py:33.
//
// Algorithm (see DESIGN.md for the derivation and the roofline accounting)
// ---------------------------------------------------------------------
// The forward recursion  a_t = (T' a_{t-1}) .* E[:,o_t]  is a serial chain per alignment file, so a
// file is cut into K segments ("parallel in time").  A chunk's first segment propagates the single vector
// pi .* E[:,o_0]; every later segment yields the segment's exact N x N transfer operator.  The stitch
// (kernels_stitch.hpp, or the blocked scan's fused tail) applies the operators in order.  All rescaling is by
// exact powers of two (integer exponents are summed), so the only difference from the textbook recursion is
// fp64 rounding order.
//
// Which kernels run a segment - per alignment column or per token of the pair-compressed stream (pair_dict.hpp),
// on the VALU or on fp64 MFMA, with the operator table in LDS or in global memory - is decided per launch group
// (imc::GroupKind) by the host-only planner in planner_host.hpp; the kernel families themselves are described in
// DESIGN.md section 5.
//
// Host side, in the order of this file and of the engine_*.hpp it includes (every function stands behind what it calls; the
// run-time options are options_host.hpp's record): context and device memory (dev_alloc, DevBuf: engine_core.hpp); chunks and dictionaries (padded buffers, obs_new
// and the owner of a chunk under construction, the level loop install_levels with its host and device sources, the device
// trainer, dictionary_for, obs_upload / obs_from_device, device ingestion of files and sequence pairs, resident alignments; the
// training policy is pair_dict.hpp's, the level rule encode_tiles.hpp's, the parses ingest_tiles.hpp's and align_tiles.hpp's);
// the kernel table, the launch plan (Group / Level / Plan own their device buffers; a Group holds its imc::GroupDecision and its
// part of the geometry), the plan list with recompress_alphabet behind it, the plan builder, one enqueue function per kernel
// family, the model layer (engine_model.hpp), the sampler (engine_sample.hpp), the C ABI.  A plan is made by host-only functions - imc::decide_groups
// (planner_host.hpp), then imc::plan_geometry and imc::group_schedules (plan_host.hpp: segments, stitch units, vectors, block
// lists, fused-tail records, the stitch hierarchy; workgroup lists, table schedules, hot set, phase table) - and build_plan adds
// the one step that needs the chunk handles, a segment's device pointer; PlanBuilder::upload() then only evicts, allocates,
// copies and registers the plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <atomic>
#include <chrono>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "../../include/imcoal_fwd.h"
#include "kernels_plain.hpp"
#include "kernels_stitch.hpp"
#include "kernels_zip.hpp"
#include "kernels_big.hpp"
#include "kernels_zip2.hpp"
#include "kernels_zip3.hpp"
#include "kernels_zip4.hpp"
#include "options_host.hpp"
#include "pair_dict.hpp"
#include "kernels_encode.hpp"
#include "kernels_train.hpp"
#include "kernels_ingest.hpp"
#include "kernels_align.hpp"
#include "kernels_phylip.hpp"
#include "slab_stream.hpp"
#include "plan_host.hpp"
#include "planner_host.hpp"
#include "model_host.hpp"
#include "kernels_model.hpp"
#include "../../include/imcoal_model.h"
#include "kernels_sample.hpp"
#include "../../include/imcoal_sample.h"
#include "obs_io.hpp"
#include "fasta_io.hpp"

#include "engine_core.hpp"

namespace {

// ---- chunks and dictionaries --------------------------------------------------------------------------
// What is compressed, what a dictionary is trained on and how (pair_dict.hpp: compressible, train_dictionary,
// training_head, recompress_share / recompress_sample) and how a chunk stores each level (encode_tiles.hpp: level_rules)
// are host-only rules checked on the CPU; here they meet the device.  Lock discipline: dictionary training and the host
// encoder run WITHOUT g_mu (O(L) host work, ~1.4 s at 1e8 columns, while other threads keep evaluating); HIP calls and
// the dictionary map g.dicts are touched only under it.

constexpr size_t OBS_PAD = 256;

// A device buffer for n bytes of symbols or tokens: rounded up to OBS_PAD plus OBS_PAD, all of it zeroed (queued on
// g.stream).  *dptr is set as soon as the allocation succeeded, also when the call then fails.
hipError_t alloc_padded(size_t n, uint8_t **dptr)
{
    const size_t bytes = ((n + OBS_PAD - 1) / OBS_PAD) * OBS_PAD + OBS_PAD;
    const hipError_t e = dev_alloc((void **)dptr, bytes);
    return e != hipSuccess ? e : hipMemsetAsync(*dptr, 0, bytes, g.stream);
}

// ... as level l of chunk o, in a buffer of the level's own
hipError_t alloc_level(imc_obs *o, int l, size_t n)
{
    const hipError_t e = alloc_padded(n, &o->d_tok[l]);
    o->owns[l] = o->d_tok[l] != nullptr;
    return e;
}

hipError_t upload_padded(const uint8_t *host, size_t n, uint8_t **dptr)
{
    hipError_t e = alloc_padded(n, dptr);
    if (e == hipSuccess && n) e = hipMemcpyAsync(*dptr, host, n, hipMemcpyHostToDevice, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    return e;
}

// n symbols on the host: bytes (alphabets up to 256), or 16-bit values (larger alphabets) - exactly one pointer is set when n > 0
struct HostSymbols {
    const uint8_t *bytes;
    const imc::tok_t *wide;
    size_t n;
};

HostSymbols symbols_in(const std::vector<uint8_t> &raw, bool wide_raw)   // (raw: what a chunk's d_sym holds)
{
    if (wide_raw) return {nullptr, reinterpret_cast<const imc::tok_t *>(raw.data()), raw.size() / sizeof(imc::tok_t)};
    return {raw.data(), nullptr, raw.size()};
}

// IMC_DEBUG_HOST (diagnostics): host time per phase of a chunk creation / a re-compression
struct PhaseTimer {
    using clock = std::chrono::steady_clock;
    clock::time_point t[5];
    int n = 0;
    PhaseTimer() { mark(); }
    void mark() { if (n < 5) t[n++] = clock::now(); }
    double ms(int phase) const { return std::chrono::duration<double, std::milli>(t[phase + 1] - t[phase]).count(); }
    static bool enabled() { static const bool on = std::getenv("IMC_DEBUG_HOST") != nullptr; return on; }
};

void release_tokens(imc_obs *o)          // the chunk falls back to its raw symbols
{
    for (int l = 0; l < imc::kNumLevels; ++l)
        if (o->owns[l]) dev_free(o->d_tok[l]);
    for (int l = 0; l < imc::kNumLevels; ++l) {
        o->d_tok[l] = nullptr; o->owns[l] = false; o->wide[l] = false; o->ntok[l] = 0; o->alphabet[l] = o->nsym; o->tok_count[l].clear();
    }
    o->dict.reset();
}

void obs_release(imc_obs *o)
{
    dev_free(o->d_sym);
    release_tokens(o);
}

// One owner for a chunk under construction: whatever the chunk holds on the device goes with it.
struct ObsDeleter {
    void operator()(imc_obs *o) const
    {
        obs_release(o);
        delete o;
    }
};
using ObsOwner = std::unique_ptr<imc_obs, ObsDeleter>;

constexpr const char *kHostAllocFailed = "host allocation failed";

// A chunk that holds nothing on the device yet (g_mu held, context ready); null: out of host memory (kHostAllocFailed).
ObsOwner obs_new(size_t L, int nsym)
{
    ObsOwner o(new (std::nothrow) imc_obs());
    if (!o) return o;
    o->id = g.next_obs_id++;
    o->pid = g.pid;
    o->device = g.device;
    o->nsym = nsym;
    o->L = L;
    o->wide_raw = nsym > imc::kByteAlphabet;
    std::fill(o->alphabet, o->alphabet + imc::kNumLevels, nsym);
    return o;
}

// The end of every creation (g_mu held): the finished chunk goes to the caller; a failed one keeps the first error's
// text, waits until nothing of it is in flight on g.stream, and is released with its owner.
int obs_finish(int rc, ObsOwner &o, imc_obs **out)
{
    if (rc != IMC_OK) {
        const std::string msg = g_err;
        (void)hipStreamSynchronize(g.stream);
        o.reset();
        return fail(rc, msg);
    }
    *out = o.release();
    return IMC_OK;
}

// A chunk holds fewer than 2^31 columns (every creation checks its length before any HIP call).
int check_columns(uint64_t L)
{
    return L >= (uint64_t)1 << 31 ? fail(IMC_ERR_ARG, "chunk too long (limit 2^31-1 columns per chunk)") : IMC_OK;
}

// Train a pair dictionary on host symbols; host work only, called without g_mu.  The two experiment variables are read at
// every training (imcoal_fwd.h).
struct TrainKnobs {
    size_t forced_min_count;
    int max_depth;
};

TrainKnobs train_knobs()
{
    const char *min_count = std::getenv("IMC_DICT_MIN_COUNT"), *max_depth = std::getenv("IMC_DICT_MAX_DEPTH");
    return {min_count ? (size_t)std::max(1, std::atoi(min_count)) : 0, max_depth ? std::atoi(max_depth) : imc::TrainLimits().max_depth};
}

std::shared_ptr<DictDev> make_dictionary(const HostSymbols &sym, int nsym, uint64_t trained_on, imc::TrainStats *stats)
{
    const TrainKnobs kn = train_knobs();
    return std::make_shared<DictDev>(imc::train_dictionary(sym.bytes, sym.wide, sym.n, nsym, kn.forced_min_count, kn.max_depth, imc::TrainLimits(), stats),
                                     trained_on);
}

// imc_last_training (g_mu held)
void note_training(uint64_t path, const imc::TrainStats &st)
{
    g.last_training[0] = path; g.last_training[1] = st.sample; g.last_training[2] = st.attempts; g.last_training[3] = st.rounds;
}

// n symbols (`unit` bytes each: 1, or 2 beyond 256 symbols) in device memory: a chunk's d_sym or its head.  A training
// sample on the device is the concatenation of such pieces.
struct TrainPiece {
    const void *d;
    int unit;
    size_t n;
};

// Device copy of a freshly trained dictionary (g_mu held, context ready).
int upload_dictionary(const std::shared_ptr<DictDev> &nd)
{
    HIP_TRY(hipSetDevice(g.device));
    nd->pid = g.pid;
    nd->dict.id = g.next_dict_id++;
    const size_t abytes = (size_t)nd->dict.alphabet * sizeof(uint16_t);
    hipError_t e2 = dev_alloc((void **)&nd->d_left, abytes);
    if (e2 == hipSuccess) e2 = dev_alloc((void **)&nd->d_right, abytes);
    if (e2 == hipSuccess) e2 = hipMemcpy(nd->d_left, nd->dict.left.data(), abytes, hipMemcpyHostToDevice);
    if (e2 == hipSuccess) e2 = hipMemcpy(nd->d_right, nd->dict.right.data(), abytes, hipMemcpyHostToDevice);
    if (e2 == hipSuccess) e2 = dev_alloc((void **)&nd->d_order, std::max<size_t>(abytes, 16));
    if (e2 == hipSuccess && !nd->order.empty())
        e2 = hipMemcpy(nd->d_order, nd->order.data(), nd->order.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e2 != hipSuccess) return fail(IMC_ERR_HIP, std::string("dictionary upload: ") + hipGetErrorString(e2));
    return IMC_OK;
}

// nd becomes the dictionary that later chunks of the alphabet share (g_mu held, context ready).
int publish_dictionary(int nsym, const std::shared_ptr<DictDev> &nd)
{
    if (int rc = upload_dictionary(nd)) return rc;
    g.dicts[nsym] = nd;
    return IMC_OK;
}

// ---- token streams of a chunk -----------------------------------------------------------------------------
// The levels of K chunks of one alphabet, stored by imc::level_rules (g_mu held; the chunks hold no token streams: new,
// or after release_tokens).  A level that is the raw stream or the level before it is settled here; for a level with a
// buffer of its own, materialise(l, rule) sets d_tok / owns / ntok - and tok_count where rule.counted - of every chunk:
// the host encoder uploads what imc::encode_levels gave, the device encoder takes a snapshot between two passes; the
// results are the same level for level and bit for bit (tests/test_gpu_device_encode.py).  On failure no chunk of the
// call keeps token streams (they evaluate on their raw symbols).
template <class Materialise>
int install_levels(const std::shared_ptr<DictDev> &dd, imc_obs *const *obs, size_t K, const std::array<imc::LevelRule, imc::kNumLevels> &rules,
                   Materialise &&materialise)
{
    int rc = IMC_OK;
    for (int l = 0; l < imc::kNumLevels && rc == IMC_OK; ++l) {
        const imc::LevelRule &r = rules[l];
        for (size_t k = 0; k < K; ++k) {
            imc_obs *o = obs[k];
            o->alphabet[l] = r.alphabet;
            o->wide[l] = r.is_wide;
            o->ntok[l] = o->L;                                   // (raw stream: d_sym, d_tok stays null)
            if (r.kind == imc::kLevelSame) { o->d_tok[l] = o->d_tok[l - 1]; o->ntok[l] = o->ntok[l - 1]; o->tok_count[l] = o->tok_count[l - 1]; }
        }
        if (r.kind == imc::kLevelOwn) rc = materialise(l, r);
    }
    if (rc != IMC_OK) {
        const std::string msg = g_err;
        (void)hipStreamSynchronize(g.stream);
        for (size_t k = 0; k < K; ++k) release_tokens(obs[k]);
        return fail(rc, msg);
    }
    for (size_t k = 0; k < K; ++k) obs[k]->dict = dd;
    return IMC_OK;
}

// Host encoder: the token streams of `enc` (imc::encode_levels with dd's dictionary) become chunk o's.
int install_encoding(imc_obs *o, const std::shared_ptr<DictDev> &dd, const imc::EncodedLevels &enc)
{
    const auto rules = imc::level_rules(imc::encode_schedule(dd->dict), o->nsym, HYBRID_MAX_ALPHABET);
    return install_levels(dd, &o, 1, rules, [&](int l, const imc::LevelRule &r) -> int {
        o->ntok[l] = enc.length[l];
        if (r.counted) {
            o->tok_count[l].assign((size_t)r.alphabet, 0u);
            for (size_t t = 1; t < enc.length[l]; ++t) o->tok_count[l][r.is_wide ? enc.wide[l][t] : enc.bytes[l][t]]++;   // (position 0 is a raw symbol)
        }
        const hipError_t e = r.is_wide ? upload_padded(reinterpret_cast<const uint8_t *>(enc.wide[l].data()), enc.length[l] * sizeof(imc::tok_t), &o->d_tok[l])
                                       : upload_padded(enc.bytes[l].data(), enc.length[l], &o->d_tok[l]);
        o->owns[l] = o->d_tok[l] != nullptr;
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? IMC_ERR_OOM : IMC_ERR_HIP, std::string("token stream upload: ") + hipGetErrorString(e));
        return IMC_OK;
    });
}

// Device encoder (kernels_encode.hpp): the token streams of K chunks of one alphabet from their raw symbols (d_sym),
// without the symbols leaving the device.  g_mu held, context ready.  Every launch and copy is on g.stream.  The
// concatenated chunks (first elements marked) go through the passes of imc::encode_schedule in two ping-pong scratch
// streams; a level with a buffer of its own is a snapshot between two passes.  The new length comes back once per pass,
// the chunk starts once per snapshot.  The scratch streams and tile tables are freed before the call returns.
constexpr size_t ENC_RUN_MAX_ELEMENTS = (size_t)1 << 30;   // per run of passes; a set beyond it goes in groups of whole chunks
constexpr size_t ENC_RUN_MAX_CHUNKS = 4096;                // (the histogram's grid and count buffer are per chunk)
static_assert(ENC_HIST_BINS >= HYBRID_MAX_ALPHABET, "every counted level must fit the histogram's LDS bins");

// The encoder's stream and what a pass over it needs: two 16-bit ping-pong scratch streams of whole tiles, the flag words
// and the tile tables.  stream() holds n elements.  Used by the encoder and by training, g_mu held.
struct EncWorkspace {
    size_t capacity = 0;                             // elements a stream holds (whole tiles)
    DevBuf<uint16_t> buf[2], flags;
    DevBuf<imc::TileSummary> sums;
    DevBuf<uint2> tile_in;
    uint32_t n = 0;
    int cur = 0;

    hipError_t alloc(size_t max_elements)
    {
        const size_t tiles = (max_elements + TILE_SIZE - 1) / TILE_SIZE;
        capacity = tiles * TILE_SIZE;
        hipError_t e = hipSuccess;
        for (int b = 0; b < 2 && e == hipSuccess; ++b) e = buf[b].alloc((capacity + TILE_ITEMS) * sizeof(uint16_t));
        if (e == hipSuccess) e = flags.alloc(tiles * TILE_THREADS * sizeof(uint16_t));
        if (e == hipSuccess) e = sums.alloc(tiles * sizeof(imc::TileSummary));
        if (e == hipSuccess) e = tile_in.alloc(tiles * sizeof(uint2));
        return e;
    }
    uint16_t *stream() { return buf[cur].get(); }
    uint32_t tiles() const { return (n + TILE_SIZE - 1) / TILE_SIZE; }
    // One pass, queued on g.stream: stream() -> the other buffer, the new length lands at d_new_n.  The owner reads it
    // back by its own protocol and then calls flip().
    void launch_pass(const EncPass &ps, uint32_t *d_new_n)
    {
        hipLaunchKernelGGL(k_enc_summary, dim3(tiles()), dim3(TILE_THREADS), 0, g.stream, stream(), n, ps, flags.get(), sums.get());
        hipLaunchKernelGGL(k_enc_scan, dim3(1), dim3(TILE_SCAN_THREADS), 0, g.stream, sums.get(), tiles(), tile_in.get(), d_new_n);
        hipLaunchKernelGGL(k_enc_scatter, dim3(tiles()), dim3(TILE_THREADS), 0, g.stream, stream(), n, ps, flags.get(), tile_in.get(), buf[cur ^ 1].get());
    }
    void flip(uint32_t new_n)
    {
        cur ^= 1;
        n = new_n;
    }
};

int device_encode_run(const std::shared_ptr<DictDev> &dd, imc_obs *const *obs, size_t K)
{
    const imc::EncodeSchedule sch = imc::encode_schedule(dd->dict);
    const auto rules = imc::level_rules(sch, dd->dict.nsym, HYBRID_MAX_ALPHABET);
    size_t total = 0;
    int max_counted = 1;
    for (size_t k = 0; k < K; ++k) total += obs[k]->L;
    for (const imc::LevelRule &r : rules)
        if (r.counted) max_counted = std::max(max_counted, r.alphabet);
    if (K == 0 || total == 0) return IMC_OK;
    if (total >= (size_t)1 << 31 || K > ENC_RUN_MAX_CHUNKS) return fail(IMC_ERR_ARG, "device encoder: too many elements or chunks in one run");
    EncWorkspace ws;
    DevBuf<uint32_t> new_n, pos, counts;
    DevBuf<uint8_t *> dptr;
    std::vector<uint32_t> hpos(K + 1), hcounts;
    std::vector<uint8_t *> hptr(K);
    size_t applied = 0;

    auto setup = [&]() -> int {
        HIP_TRY(hipSetDevice(g.device));
        HIP_TRY(ws.alloc(total));
        ws.n = (uint32_t)total;
        HIP_TRY(new_n.alloc(sizeof(uint32_t)));
        HIP_TRY(pos.alloc((K + 1) * sizeof(uint32_t)));
        HIP_TRY(dptr.alloc(K * sizeof(uint8_t *)));
        HIP_TRY(counts.alloc(K * (size_t)max_counted * sizeof(uint32_t)));
        size_t off = 0;
        for (size_t k = 0; k < K; ++k) {
            const uint32_t L = (uint32_t)obs[k]->L;
            if (!L) return fail(IMC_ERR_ARG, "device encoder: empty chunk");
            hipLaunchKernelGGL(k_enc_load, dim3((L + TILE_THREADS - 1) / TILE_THREADS), dim3(TILE_THREADS), 0, g.stream, (const void *)obs[k]->d_sym,
                               obs[k]->wide_raw ? 2 : 1, L, ws.stream() + off);
            off += L;
        }
        HIP_TRY(hipGetLastError());
        return IMC_OK;
    };
    auto run_pass = [&](const imc::EncodeSchedule::Pass &p) -> int {
        ws.launch_pass(EncPass{dd->d_left, dd->d_right, p.z0, p.nz}, new_n.get());
        HIP_TRY(hipGetLastError());
        uint32_t hn = 0;
        HIP_TRY(hipMemcpyAsync(&hn, new_n.get(), sizeof hn, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (hn == 0 || hn > ws.n) return fail(IMC_ERR_HIP, "device encoder: a pass returned an impossible length");
        ws.flip(hn);
        return IMC_OK;
    };
    auto snapshot = [&](int l, const imc::LevelRule &r) -> int {
        const uint32_t n = ws.n, tiles = ws.tiles();
        hipLaunchKernelGGL(k_enc_mark_summary, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, ws.stream(), n, ws.sums.get());
        hipLaunchKernelGGL(k_enc_scan, dim3(1), dim3(TILE_SCAN_THREADS), 0, g.stream, ws.sums.get(), tiles, ws.tile_in.get(), new_n.get());
        hipLaunchKernelGGL(k_enc_mark_scatter, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, ws.stream(), n, ws.tile_in.get(), pos.get(), (uint32_t)K);
        HIP_TRY(hipGetLastError());
        uint32_t marks = 0;
        HIP_TRY(hipMemcpyAsync(&marks, new_n.get(), sizeof marks, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(hpos.data(), pos.get(), (K + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        bool sane = marks == K && hpos[0] == 0 && hpos[K] == n;
        for (size_t k = 0; k < K && sane; ++k) sane = hpos[k] < hpos[k + 1];
        if (!sane) return fail(IMC_ERR_HIP, "device encoder: chunk starts lost");
        for (size_t k = 0; k < K; ++k) {
            const size_t len = hpos[k + 1] - hpos[k];
            HIP_TRY(alloc_level(obs[k], l, len * (r.is_wide ? sizeof(imc::tok_t) : 1)));
            obs[k]->ntok[l] = len;
            hptr[k] = obs[k]->d_tok[l];
        }
        HIP_TRY(hipMemcpyAsync(dptr.get(), hptr.data(), K * sizeof(uint8_t *), hipMemcpyHostToDevice, g.stream));
        hipLaunchKernelGGL(k_enc_snapshot, dim3((n + TILE_THREADS - 1) / TILE_THREADS), dim3(TILE_THREADS), 0, g.stream, ws.stream(), n, pos.get(),
                           (uint32_t)K, dptr.get(), r.is_wide ? 0 : 1);
        HIP_TRY(hipGetLastError());
        if (r.counted) {
            uint32_t longest = 1;
            for (size_t k = 0; k < K; ++k) longest = std::max(longest, hpos[k + 1] - hpos[k]);
            const uint32_t bx = std::max<uint32_t>(1, std::min<uint32_t>(128, (longest + 8 * TILE_THREADS - 1) / (8 * TILE_THREADS)));
            HIP_TRY(hipMemsetAsync(counts.get(), 0, K * (size_t)r.alphabet * sizeof(uint32_t), g.stream));
            hipLaunchKernelGGL(k_enc_histogram, dim3(bx, (uint32_t)K), dim3(TILE_THREADS), 0, g.stream, ws.stream(), pos.get(), r.alphabet, counts.get());
            HIP_TRY(hipGetLastError());
            hcounts.resize(K * (size_t)r.alphabet);
            HIP_TRY(hipMemcpyAsync(hcounts.data(), counts.get(), hcounts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
        }
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (r.counted)
            for (size_t k = 0; k < K; ++k)
                obs[k]->tok_count[l].assign(hcounts.begin() + k * (size_t)r.alphabet, hcounts.begin() + (k + 1) * (size_t)r.alphabet);
        return IMC_OK;
    };
    if (int rc = setup()) {
        (void)hipStreamSynchronize(g.stream);        // (the scratch streams are freed on return)
        return rc;
    }
    return install_levels(dd, obs, K, rules, [&](int l, const imc::LevelRule &r) -> int {
        for (; applied < (size_t)sch.after[l]; ++applied)
            if (int rc = run_pass(sch.passes[applied])) return rc;
        return snapshot(l, r);
    });
}

int device_encode(const std::shared_ptr<DictDev> &dd, imc_obs *const *obs, size_t K)
{
    for (size_t first = 0; first < K;) {
        size_t last = first, sum = 0;
        while (last < K && last - first < ENC_RUN_MAX_CHUNKS && (last == first || sum + obs[last]->L <= ENC_RUN_MAX_ELEMENTS)) sum += obs[last++]->L;
        if (int rc = device_encode_run(dd, obs + first, last - first)) {
            const std::string msg = g_err;
            for (size_t k = 0; k < first; ++k) release_tokens(obs[k]);
            return fail(rc, msg);
        }
        first = last;
    }
    return IMC_OK;
}

// ---- dictionary training on the device ----------------------------------------------------------------------
// imc::train_with (train_tiles.hpp) decides; this is its backend (kernels_train.hpp).  g_mu held, context ready, every
// launch and copy on g.stream.  The stream is the encoder's pair of ping-pong scratch streams without chunk marks; the
// device dictionary (left / right / depth) grows as training goes - k_trn_argmax appends a byte merge, a round's tokens
// are uploaded - and the encoder's pass kernels read it.  One synchronisation per merge (winner and new length
// together: the pass runs before the host has seen the winner, and is dropped if the host stops there), two per round
// (candidates, new length).  Every buffer is released on return.
struct DeviceTrainer {
    const TrainPiece *pieces;
    std::vector<size_t> piece_len;
    EncWorkspace ws;
    DevBuf<uint16_t> left, right, depth;
    DevBuf<uint2> list;
    DevBuf<uint32_t> scalars, counts, tkeys, tcounts;   // scalars: [0] new length, [1..3] winner {a, b, count}, [4] candidates, [5] table overflow
    uint32_t table_capacity = 0, list_capacity = 0;
    uint32_t pending_n = 0;

    int init(const TrainPiece *p, size_t n_pieces, size_t max_stream)
    {
        pieces = p;
        for (size_t k = 0; k < n_pieces; ++k) piece_len.push_back(p[k].n);
        if (max_stream == 0 || max_stream >= (size_t)1 << 31) return fail(IMC_ERR_ARG, "device training: impossible sample size");
        HIP_TRY(hipSetDevice(g.device));
        HIP_TRY(ws.alloc(max_stream));
        HIP_TRY(scalars.alloc(8 * sizeof(uint32_t)));
        HIP_TRY(counts.alloc((size_t)imc::kByteAlphabet * imc::kByteAlphabet * sizeof(uint32_t)));
        for (DevBuf<uint16_t> *d : {&left, &right, &depth}) {
            HIP_TRY(d->alloc((size_t)imc::kMaxAlphabet * sizeof(uint16_t)));
            HIP_TRY(hipMemsetAsync(d->get(), 0, (size_t)imc::kMaxAlphabet * sizeof(uint16_t), g.stream));
        }
        HIP_TRY(hipMemsetAsync(scalars.get(), 0, 8 * sizeof(uint32_t), g.stream));
        return IMC_OK;
    }
    int load(size_t first, size_t count)
    {
        if (count > ws.capacity) return fail(IMC_ERR_HIP, "device training: sample beyond the scratch stream");
        for (const imc::SampleRange &r : imc::sample_ranges(piece_len, first, count))
            hipLaunchKernelGGL(k_trn_load, dim3((uint32_t)((r.count + TILE_THREADS - 1) / TILE_THREADS)), dim3(TILE_THREADS), 0, g.stream,
                               pieces[r.piece].d, pieces[r.piece].unit, (uint32_t)r.src_first, (uint32_t)r.count, ws.buf[0].get() + r.dst_first);
        HIP_TRY(hipGetLastError());
        ws.cur = 0;
        ws.n = (uint32_t)count;
        return IMC_OK;
    }
    void launch_pass(int z0, int nz) { ws.launch_pass(EncPass{left.get(), right.get(), z0, nz}, scalars.get()); }   // scalars[0] = new length
    int byte_step(int A, int max_depth, imc::ByteStep *s)
    {
        if (ws.n < 2 || A >= imc::kByteAlphabet) return fail(IMC_ERR_HIP, "device training: impossible byte step");
        HIP_TRY(hipMemsetAsync(counts.get(), 0, (size_t)A * A * sizeof(uint32_t), g.stream));
        const dim3 grid((ws.n + TRN_HIST_TILE - 1) / TRN_HIST_TILE);
        if (imc::pair_bins_in_lds((uint32_t)A))
            hipLaunchKernelGGL(k_trn_pair_hist<true>, grid, dim3(TILE_THREADS), 0, g.stream, ws.stream(), ws.n, (uint32_t)A, counts.get());
        else
            hipLaunchKernelGGL(k_trn_pair_hist<false>, grid, dim3(TILE_THREADS), 0, g.stream, ws.stream(), ws.n, (uint32_t)A, counts.get());
        hipLaunchKernelGGL(k_trn_argmax, dim3(1), dim3(TRN_ARGMAX_THREADS), 0, g.stream, counts.get(), (uint32_t)A, max_depth, left.get(), right.get(),
                           depth.get(), scalars.get() + 1);
        launch_pass(A, 1);                           // (with no winner token A is a stale pair: the output is dropped)
        HIP_TRY(hipGetLastError());
        uint32_t h[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(h, scalars.get(), sizeof h, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        *s = imc::ByteStep{h[1], h[2], h[3], h[0]};
        if (s->count && (s->a >= (uint32_t)A || s->b >= (uint32_t)A || s->count >= ws.n || s->new_n == 0 || s->new_n > ws.n))
            return fail(IMC_ERR_HIP, "device training: a merge returned an impossible winner or length");
        pending_n = s->new_n;
        return IMC_OK;
    }
    void accept() { ws.flip(pending_n); }
    void truncate(size_t keep) { ws.n = (uint32_t)std::min<size_t>(ws.n, keep); }
    int count_round(size_t threshold, std::vector<imc::RoundCandidate> &found)
    {
        if (ws.n < 2) return fail(IMC_ERR_HIP, "device training: impossible round");
        const uint32_t cap = imc::count_table_capacity(ws.n);
        if (!tkeys) {                                // the first round is the longest stream the rounds see
            table_capacity = cap;
            list_capacity = ws.n;
            HIP_TRY(tkeys.alloc((size_t)cap * sizeof(uint32_t)));
            HIP_TRY(tcounts.alloc((size_t)cap * sizeof(uint32_t)));
            HIP_TRY(list.alloc((size_t)list_capacity * sizeof(uint2)));
        }
        if (cap > table_capacity) return fail(IMC_ERR_HIP, "device training: the stream grew");
        HIP_TRY(hipMemsetAsync(tkeys.get(), 0xff, (size_t)cap * sizeof(uint32_t), g.stream));
        HIP_TRY(hipMemsetAsync(tcounts.get(), 0, (size_t)cap * sizeof(uint32_t), g.stream));
        HIP_TRY(hipMemsetAsync(scalars.get() + 4, 0, 2 * sizeof(uint32_t), g.stream));
        hipLaunchKernelGGL(k_trn_pair_count, dim3((ws.n + TILE_SIZE - 1) / TILE_SIZE), dim3(TILE_THREADS), 0, g.stream, ws.stream(), ws.n, cap, tkeys.get(),
                           tcounts.get(), scalars.get() + 5);
        hipLaunchKernelGGL(k_trn_candidates, dim3((cap + TILE_THREADS - 1) / TILE_THREADS), dim3(TILE_THREADS), 0, g.stream, tkeys.get(), tcounts.get(), cap,
                           (uint32_t)std::min<size_t>(threshold, 0xffffffffu), list.get(), list_capacity, scalars.get() + 4);
        HIP_TRY(hipGetLastError());
        uint32_t h[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h, scalars.get() + 4, sizeof h, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (h[1] || h[0] > list_capacity) return fail(IMC_ERR_HIP, "device training: impossible - the pair table overflowed");
        std::vector<uint2> got(h[0]);
        if (h[0]) HIP_TRY(hipMemcpy(got.data(), list.get(), (size_t)h[0] * sizeof(uint2), hipMemcpyDeviceToHost));
        found.reserve(got.size());
        for (const uint2 &c : got) found.push_back({(uint64_t)c.x, c.y});
        return IMC_OK;
    }
    int apply(const imc::PairDict &d, int z0, int nz, size_t *new_n)
    {
        if (ws.n < 1 || nz < 1 || nz > 256 || z0 + nz > imc::kMaxAlphabet || z0 + nz > d.alphabet) return fail(IMC_ERR_HIP, "device training: impossible pass");
        HIP_TRY(hipMemcpyAsync(left.get() + z0, d.left.data() + z0, (size_t)nz * sizeof(uint16_t), hipMemcpyHostToDevice, g.stream));
        HIP_TRY(hipMemcpyAsync(right.get() + z0, d.right.data() + z0, (size_t)nz * sizeof(uint16_t), hipMemcpyHostToDevice, g.stream));
        launch_pass(z0, nz);
        HIP_TRY(hipGetLastError());
        uint32_t hn = 0;
        HIP_TRY(hipMemcpyAsync(&hn, scalars.get(), sizeof hn, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (hn == 0 || hn > ws.n) return fail(IMC_ERR_HIP, "device training: a pass returned an impossible length");
        ws.flip(hn);
        *new_n = hn;
        return IMC_OK;
    }
};

int device_train(const TrainPiece *pieces, size_t n_pieces, int nsym, size_t L, uint64_t trained_on, std::shared_ptr<DictDev> *out)
{
    const imc::TrainLimits lim;
    const TrainKnobs kn = train_knobs();             // the two experiment variables are read at every training (imcoal_fwd.h)
    if (L < 2) return fail(IMC_ERR_ARG, "device training: empty sample");
    const size_t max_stream = nsym > imc::kByteAlphabet ? std::min(L - 1, lim.wide_train_tokens * 8)
                                                        : std::max(std::min(L - 1, lim.train_max), std::min(L, lim.wide_train_tokens * 96) - 1);
    imc::TrainedDict t;
    imc::TrainStats st;
    int rc;
    {
        DeviceTrainer be;
        rc = be.init(pieces, n_pieces, max_stream);
        if (rc == IMC_OK) rc = imc::train_with(be, L, nsym, kn.forced_min_count, kn.max_depth, lim, t, st);
        if (rc != IMC_OK) {
            const std::string msg = g_err;
            (void)hipStreamSynchronize(g.stream);    // (the scratch streams are freed on return)
            return fail(rc, msg);
        }
    }
    note_training(1, st);
    *out = std::make_shared<DictDev>(std::move(t), trained_on);
    return IMC_OK;
}

// The dictionary a new chunk of L columns is encoded with (the preprocess_raw_observations analogue, hmm.py:16): the
// one published for its alphabet; else, for the first chunk long enough, one trained now; else none (*dd stays null).
// Called and left with lk (g_mu) held and the context ready; the lock is released while training runs.  head(&symbols)
// supplies the training symbols - at least imc::training_head() of the chunk - and is called, under the lock, only when
// a dictionary has to be trained.  With imc_set_device_training(1) and the chunk's symbols on the device (`dev`, all L
// of them; else null) the dictionary is trained there instead, with the lock held, and nothing comes back to the host.
// must_train(): whether a call now would train one.
bool must_train(size_t L, int nsym)
{
    return g.opt.compression && imc::compressible(L, nsym) && g.dicts.find(nsym) == g.dicts.end() && L >= imc::TrainLimits().train_min;
}

template <class Head>
int dictionary_for(std::unique_lock<std::mutex> &lk, size_t L, int nsym, Head &&head, const TrainPiece *dev, std::shared_ptr<DictDev> *dd)
{
    if (!g.opt.compression || !imc::compressible(L, nsym)) return IMC_OK;
    auto it = g.dicts.find(nsym);
    if (it != g.dicts.end()) { *dd = it->second; return IMC_OK; }
    if (L < imc::TrainLimits().train_min) return IMC_OK;
    std::shared_ptr<DictDev> nd;
    if (dev && device_mode(&imc::Options::device_train) == 1) {
        if (int rc = device_train(dev, 1, nsym, L, L, &nd)) return rc;
    } else {
        HostSymbols sym{};
        if (int rc = head(&sym)) return rc;
        imc::TrainStats st;
        lk.unlock();
        nd = make_dictionary(sym, nsym, L, &st);                         // host only, unlocked
        lk.lock();
        note_training(0, st);
    }
    it = g.dicts.find(nsym);
    if (it != g.dicts.end()) { *dd = it->second; return IMC_OK; }        // another thread published one meanwhile: use that
    if (int rc = publish_dictionary(nsym, nd)) return rc;
    *dd = nd;
    return IMC_OK;
}

// The host symbols into the chunk's own padded buffer.
int upload_symbols(imc_obs *o, const HostSymbols &sym)
{
    const hipError_t e = o->wide_raw ? upload_padded(reinterpret_cast<const uint8_t *>(sym.wide), sym.n * sizeof(imc::tok_t), &o->d_sym)
                                     : upload_padded(sym.bytes, sym.n, &o->d_sym);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? IMC_ERR_OOM : IMC_ERR_HIP, std::string("observation upload: ") + hipGetErrorString(e));
    return IMC_OK;
}

// obs_upload for the creation that trains its alphabet's dictionary, with imc_set_device_training(1): the symbols go up
// first and the dictionary is trained from the chunk's own buffer; the encoder is the one imc_set_device_encoding names.
// lk (g_mu) held, context ready.
int obs_upload_and_train(std::unique_lock<std::mutex> &lk, const HostSymbols &sym, int nsym, bool on_device, imc_obs **out)
{
    PhaseTimer tm;
    HIP_TRY(hipSetDevice(g.device));
    ObsOwner o = obs_new(sym.n, nsym);
    if (!o) return fail(IMC_ERR_OOM, kHostAllocFailed);
    if (int rc = upload_symbols(o.get(), sym)) return obs_finish(rc, o, out);
    tm.mark();
    std::shared_ptr<DictDev> dd;
    const TrainPiece piece{o->d_sym, o->wide_raw ? 2 : 1, sym.n};
    if (int rc = dictionary_for(lk, sym.n, nsym, [](HostSymbols *) -> int { return IMC_OK; }, &piece, &dd)) return obs_finish(rc, o, out);
    tm.mark();
    if (dd && dd->dict.alphabet > nsym) {
        int rc;
        imc_obs *const chunk = o.get();
        if (on_device) rc = device_encode(dd, &chunk, 1);
        else {
            imc::EncodedLevels enc;
            lk.unlock();                             // host only, unlocked (a published dictionary is immutable; nobody else holds o)
            imc::encode_levels(dd->dict, sym.bytes, sym.wide, sym.n, enc);
            lk.lock();
            (void)hipSetDevice(g.device);
            rc = install_encoding(chunk, dd, enc);
        }
        if (rc != IMC_OK) return obs_finish(rc, o, out);
    }
    tm.mark();
    if (PhaseTimer::enabled())
        std::fprintf(stderr, "[imc host] create %zu columns: upload %.1f ms, train %.1f ms, encode + install %.1f ms (%s encoder, device trainer)\n", sym.n,
                     tm.ms(0), tm.ms(1), tm.ms(2), on_device ? "device" : "host");
    g.last_ingest[0] = g.last_ingest[1] = g.last_ingest[2] = 0;   // (imc_last_ingest: parsed and validated on the host)
    g.last_ingest[3] = sym.n;
    return obs_finish(IMC_OK, o, out);
}

// Build a chunk from validated host symbols (exactly one of host / host16 is non-null when L > 0).  Called WITHOUT g_mu.
int obs_upload(const uint8_t *host, const imc::tok_t *host16, size_t L, int nsym, imc_obs **out)
{
    const HostSymbols sym{host, host16, L};
    PhaseTimer tm;
    std::shared_ptr<DictDev> dd;
    std::unique_lock<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    const bool on_device = g.opt.device_encode == 1;
    if (device_mode(&imc::Options::device_train) == 1 && must_train(L, nsym)) return obs_upload_and_train(lk, sym, nsym, on_device, out);
    if (int rc = dictionary_for(lk, L, nsym, [&](HostSymbols *s) -> int { *s = sym; return IMC_OK; }, nullptr, &dd)) return rc;
    lk.unlock();
    tm.mark();
    imc::EncodedLevels enc;
    const bool zipped = dd && dd->dict.alphabet > nsym;
    // host only, unlocked (a published dictionary is immutable) - or, with imc_set_device_encoding(1), on the device below
    if (zipped && !on_device) imc::encode_levels(dd->dict, host, host16, L, enc);
    tm.mark();

    lk.lock();
    if (int rc = ensure_ctx()) return rc;
    HIP_TRY(hipSetDevice(g.device));
    ObsOwner o = obs_new(L, nsym);
    if (!o) return fail(IMC_ERR_OOM, kHostAllocFailed);
    if (int rc = upload_symbols(o.get(), sym)) return obs_finish(rc, o, out);
    tm.mark();
    if (zipped) {
        imc_obs *const chunk = o.get();
        if (int rc = on_device ? device_encode(dd, &chunk, 1) : install_encoding(chunk, dd, enc)) return obs_finish(rc, o, out);
    }
    tm.mark();
    if (PhaseTimer::enabled())   // (host encoder: "encode" is encode_levels and "install" the upload of its streams; device encoder: all of it is "install")
        std::fprintf(stderr, "[imc host] create %zu columns: train %.1f ms, encode %.1f ms, upload %.1f ms, install %.1f ms (%s encoder, host trainer)\n", L,
                     tm.ms(0), tm.ms(1), tm.ms(2), tm.ms(3), on_device ? "device" : "host");
    g.last_ingest[0] = g.last_ingest[1] = g.last_ingest[2] = 0;   // (imc_last_ingest: parsed and validated on the host)
    g.last_ingest[3] = L;
    return obs_finish(IMC_OK, o, out);
}

// d_sym must be device memory of the library's device, `bytes` long: an error, never a fault (g_mu held, context ready).
int check_device_range(const void *p, size_t bytes)
{
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(IMC_ERR_ARG, "d_sym is not device memory (hipPointerGetAttributes)");
    }
    if (at.type != hipMemoryTypeDevice) return fail(IMC_ERR_ARG, "d_sym is not device memory");
    if (at.device != g.device) return fail(IMC_ERR_ARG, "d_sym is memory of device " + std::to_string(at.device) + ", the library runs on device " + std::to_string(g.device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess) {
        if ((const char *)p + bytes > (const char *)base + size) return fail(IMC_ERR_ARG, "d_sym: the allocation ends before L symbols");
    } else (void)hipGetLastError();
    return IMC_OK;
}

// ---- chunks from symbols in device memory -------------------------------------------------------------------
// The pieces every creation that has its symbols on the device is made of (imc_obs_create_device and the device
// ingestion below); g_mu held, context ready, everything on g.stream.

// First column of d[0..L) (sym_bytes per symbol) that is not below nsym: IMC_ERR_SYMBOL "symbol V at column T <tail>".
int validate_device_symbols(const void *d, int sym_bytes, size_t L, int nsym, const char *tail)
{
    if (!L) return IMC_OK;
    DevBuf<uint32_t> first_bad;
    HIP_TRY(first_bad.alloc(sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(first_bad.get(), 0xff, sizeof(uint32_t), g.stream));
    const dim3 grid((uint32_t)((L + TILE_THREADS - 1) / TILE_THREADS));
    hipLaunchKernelGGL(k_enc_validate, grid, dim3(TILE_THREADS), 0, g.stream, d, sym_bytes, (uint32_t)L, (uint32_t)nsym, first_bad.get());
    HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, first_bad.get(), sizeof bad, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    if (bad == 0xffffffffu) return IMC_OK;
    int32_t v = 0;
    uint8_t raw[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(raw, (const char *)d + (size_t)bad * sym_bytes, sym_bytes, hipMemcpyDeviceToHost));
    if (sym_bytes == 1) v = raw[0];
    else if (sym_bytes == 2) { uint16_t u; std::memcpy(&u, raw, 2); v = u; }
    else std::memcpy(&v, raw, 4);
    return fail(IMC_ERR_SYMBOL, "symbol " + std::to_string(v) + " at column " + std::to_string(bad) + " " + tail);
}

// The chunk's own padded symbol buffer (all zeros; nothing has waited for the memset yet).
int alloc_symbols(imc_obs *o)
{
    HIP_TRY(alloc_padded(o->L * (o->wide_raw ? sizeof(imc::tok_t) : 1), &o->d_sym));
    return IMC_OK;
}

// d_src[0..o->L) validated against nsym and copied into the chunk's own buffer (narrowed to bytes, or to 16 bits).
int adopt_device_symbols(imc_obs *o, const void *d_src, int sym_bytes, const char *tail)
{
    if (int rc = alloc_symbols(o)) return rc;
    if (!o->L) return IMC_OK;
    if (int rc = validate_device_symbols(d_src, sym_bytes, o->L, o->nsym, tail)) return rc;
    const dim3 grid((uint32_t)((o->L + TILE_THREADS - 1) / TILE_THREADS));
    hipLaunchKernelGGL(k_enc_narrow, grid, dim3(TILE_THREADS), 0, g.stream, d_src, sym_bytes, (uint32_t)o->L, o->d_sym, o->wide_raw ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    return IMC_OK;
}

// The chunk's symbols are in its buffer: its dictionary (only the head that training looks at comes back to the host,
// and only when the alphabet has no dictionary yet) and its token streams, encoded on the device.
int finish_device_chunk(std::unique_lock<std::mutex> &lk, imc_obs *o)
{
    HIP_TRY(hipStreamSynchronize(g.stream));
    if (!o->L) return IMC_OK;
    const bool wide_raw = o->wide_raw;
    const size_t unit = wide_raw ? sizeof(imc::tok_t) : 1;
    std::shared_ptr<DictDev> dd;
    std::vector<uint8_t> head;
    auto copy_head = [&](HostSymbols *s) -> int {
        head.resize(imc::training_head(o->L, wide_raw) * unit);
        HIP_TRY(hipMemcpy(head.data(), o->d_sym, head.size(), hipMemcpyDeviceToHost));
        *s = symbols_in(head, wide_raw);
        return IMC_OK;
    };
    const TrainPiece piece{o->d_sym, (int)unit, o->L};   // (with imc_set_device_training(1) no head comes back)
    if (int rc = dictionary_for(lk, o->L, o->nsym, copy_head, &piece, &dd)) return rc;
    std::vector<uint8_t>().swap(head);
    HIP_TRY(hipSetDevice(g.device));
    return dd && dd->dict.alphabet > o->nsym ? device_encode(dd, &o, 1) : IMC_OK;
}

void note_ingest(uint64_t path, uint64_t bytes, uint64_t slabs, uint64_t columns)
{
    g.last_ingest[0] = path; g.last_ingest[1] = bytes; g.last_ingest[2] = slabs; g.last_ingest[3] = columns;
}

// Build a chunk from symbols in device memory (imc_obs_create_device; arguments already checked).  The device work is on
// the library's stream under g_mu.
int obs_from_device(const void *d_src, size_t L, int nsym, int sym_bytes, hipStream_t user_stream, imc_obs **out)
{
    std::unique_lock<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    HIP_TRY(hipSetDevice(g.device));
    if (L)
        if (int rc = check_device_range(d_src, L * (size_t)sym_bytes)) return rc;
    HIP_TRY(hipStreamSynchronize(user_stream));   // what the caller queued on its stream has produced the symbols
    ObsOwner o = obs_new(L, nsym);
    if (!o) return fail(IMC_ERR_OOM, kHostAllocFailed);
    int rc = adopt_device_symbols(o.get(), d_src, sym_bytes, "outside [0,nsym)");
    if (rc == IMC_OK) rc = finish_device_chunk(lk, o.get());
    if (rc == IMC_OK) note_ingest(0, 0, 0, L);
    return obs_finish(rc, o, out);
}

// ---- device ingestion -------------------------------------------------------------------------------------
// imc_obs_create_from_text with imc_set_device_ingest(1), and imc_obs_create_pairwise: the bytes of the file (of the two
// sequences) go to the device in slabs of at most IMC_INGEST_SLAB_BYTES through two pinned staging buffers, so host memory
// is bounded by the slab size, and the symbols are made there (kernels_ingest.hpp; the rules and the slab cut are
// ingest_tiles.hpp's).  From the symbols on, the chunk is built by the pieces above.  The file is read WITHOUT g_mu, and
// slab k + 1 is read while slab k is on the device; launches and copies are on g.stream with g_mu held.  Device memory
// beyond the chunk itself: the two slabs, and for text one symbol buffer of the file's upper bound (max_tokens_in), both
// released before the token streams are encoded.
constexpr size_t INGEST_SLAB_DEFAULT = (size_t)4 << 20;    // (profiles/device_ingest_ab.txt: the sweep over 1 .. 256 MiB)

size_t ingest_slab_bytes() { return imc::slab_bytes_setting(std::getenv("IMC_INGEST_SLAB_BYTES"), INGEST_SLAB_DEFAULT); }

struct IngestStage {             // created, used for HIP calls and destroyed with g_mu held
    size_t slab = 0;
    uint8_t *host[2] = {nullptr, nullptr};
    DevBuf<uint8_t> dev[2];
    hipEvent_t done[2] = {nullptr, nullptr};
    void *pinned = nullptr;          // pinned, as many bytes as the caller asked for: one verdict per buffer, and what it keeps behind them

    IngestStage() = default;
    IngestStage(const IngestStage &) = delete;
    IngestStage &operator=(const IngestStage &) = delete;
    int alloc(size_t slab_bytes, int buffers, size_t pinned_bytes = 0)
    {
        slab = slab_bytes;
        if (pinned_bytes) HIP_TRY(hipHostMalloc(&pinned, pinned_bytes, hipHostMallocDefault));
        for (int b = 0; b < buffers; ++b) {
            HIP_TRY(hipHostMalloc((void **)&host[b], slab, hipHostMallocDefault));
            HIP_TRY(dev[b].alloc(ing_slab_alloc(slab)));
            HIP_TRY(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        }
        return IMC_OK;
    }
    void release()
    {
        (void)hipStreamSynchronize(g.stream);
        for (int b = 0; b < 2; ++b) {
            if (host[b]) (void)hipHostFree(host[b]);
            if (done[b]) (void)hipEventDestroy(done[b]);
            dev[b].reset();
            host[b] = nullptr;
            done[b] = nullptr;
        }
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr;
    }
    ~IngestStage() { release(); }
};

// g_mu for the length of a callback of imc::slab_stream, which runs without it.
struct Relock {
    std::unique_lock<std::mutex> &lk;
    explicit Relock(std::unique_lock<std::mutex> &l) : lk(l) { lk.lock(); }
    ~Relock() { lk.unlock(); }
};

// `total` units go to the device in pieces of at most `piece` units, alternating between the stage's two buffers:
// fill(b, off, len) - called WITHOUT g_mu - puts the piece into st.host[b] (IMC_OK, or a fail()), consume(b, off, len)
// queues its upload and its kernels on g.stream.  Piece k + 1 is filled while piece k is on the device.
template <class Fill, class Consume>
int ingest_pump(std::unique_lock<std::mutex> &lk, IngestStage &st, uint64_t total, uint64_t piece, uint64_t *pieces, Fill &&fill, Consume &&consume)
{
    bool used[2] = {false, false};
    int b = 0;
    for (uint64_t off = 0; off < total; off += piece, b ^= 1) {
        const uint64_t len = std::min(piece, total - off);
        lk.unlock();
        int rc = IMC_OK;
        if (used[b] && hipEventSynchronize(st.done[b]) != hipSuccess) rc = fail(IMC_ERR_HIP, "ingest: waiting for a staging buffer failed");
        if (rc == IMC_OK) rc = fill(b, off, len);
        lk.lock();
        if (rc != IMC_OK) return rc;
        HIP_TRY(hipSetDevice(g.device));
        if (int rc2 = consume(b, off, len)) return rc2;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(st.done[b], g.stream));
        used[b] = true;
        ++*pieces;
    }
    HIP_TRY(hipStreamSynchronize(g.stream));
    return IMC_OK;
}

// One pass of a regular file of file_bytes bytes, fp at its start, through the device parser of its format: ingest_pump's
// counterpart for inputs that must be cut.  The slab is sized from the setting and the file, the stage gets its two
// buffers and pinned room for two totals (and pinned_behind bytes behind them), and the file goes through
// imc::slab_stream - read, and the carry copied, WITHOUT g_mu; uploads, launches and copies on g.stream with g_mu held;
// slab k's total is looked at before slab k + 1 is cut.  The format says the rest:
//   buffers(slab)                 allocate what is sized from the slab, total among it (once, in front of the loop)
//   first(h_slab, cut)            what the first slab's bytes decide, in front of its upload (IMC_OK, kSlabDeclined, a fail())
//   cut_of(buf, fill, last)       the format's slab rule
//   launch(d_slab, n, tiles)      the kernels over the n bytes (tiles tiles) of the slab; they leave its Total in total
//   accept(t, h_slab, cut)        the format's rules on that Total, an imc::IoResult; its errors become fail()
// prefix words a failed wait.  *declined: the device parser does not take this file and the caller's host reader reads it
// from its start; pass says how far the device got.
struct SlabPass {
    uint64_t sent = 0, slabs = 0;
};

int no_first_slab_work(const uint8_t *, size_t) { return IMC_OK; }

static_assert(imc::kRuleSymbol == IMC_ERR_SYMBOL && imc::kRuleHip == IMC_ERR_HIP && imc::kRuleIo == IMC_ERR_IO && imc::kSlabDone == IMC_OK,
              "the rules' codes are the library's");

template <class Total, class Buffers, class First, class Cut, class Launch, class Accept>
int slab_pass(std::unique_lock<std::mutex> &lk, FILE *fp, uint64_t file_bytes, const char *prefix, IngestStage &st, size_t pinned_behind, const DevBuf<Total> &total,
              Buffers &&buffers, First &&first, Cut &&cut_of, Launch &&launch, Accept &&accept, SlabPass &pass, bool *declined)
{
    const size_t slab = (size_t)std::min<uint64_t>(ingest_slab_bytes(), std::max<uint64_t>(file_bytes, imc::kMinSlabBytes));
    if (int rc = st.alloc(slab, file_bytes > slab ? 2 : 1, 2 * sizeof(Total) + pinned_behind)) return rc;
    if (int rc = buffers(slab)) return rc;
    Total *verdict = static_cast<Total *>(st.pinned);
    lk.unlock();                                                        // the file is read and the carry copied WITHOUT g_mu
    const int end = imc::slab_stream(
        st.host, slab, imc::FileSlabReader{fp, file_bytes}, cut_of,
        [&](int cur, size_t cut) -> int {
            Relock held(lk);
            HIP_TRY(hipSetDevice(g.device));
            if (!pass.slabs)
                if (int rc = first(st.host[cur], cut)) return rc;
            HIP_TRY(hipMemcpyAsync(st.dev[cur].get(), st.host[cur], cut, hipMemcpyHostToDevice, g.stream));
            launch((const uint8_t *)st.dev[cur].get(), (uint32_t)cut, (uint32_t)((cut + TILE_SIZE - 1) / TILE_SIZE));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&verdict[cur], total.get(), sizeof(Total), hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipEventRecord(st.done[cur], g.stream));
            pass.sent += cut;
            ++pass.slabs;
            return IMC_OK;
        },
        [&](int cur, size_t cut) -> int {
            const hipError_t waited = hipEventSynchronize(st.done[cur]);
            Relock held(lk);
            if (waited != hipSuccess) return fail(IMC_ERR_HIP, std::string(prefix) + hipGetErrorString(waited));
            const imc::IoResult r = accept(verdict[cur], st.host[cur], cut);
            return r.code == IMC_OK || r.code == imc::kSlabDeclined ? r.code : fail(r.code, r.msg);
        });
    lk.lock();
    *declined = end == imc::kSlabDeclined;
    return *declined ? IMC_OK : end;
}

// Text file of file_bytes bytes, fp at its start.  *declined: the device parser does not take this file (a slab without
// whitespace, a digit run beyond 16) - nothing was created, the host parser reads it from its start.  Errors are the host
// parser's, in file order (imc::TextSession).
int ingest_text(std::unique_lock<std::mutex> &lk, FILE *fp, uint64_t file_bytes, const char *path, int nsym, imc_obs **out, bool *declined)
{
    const bool wide = nsym > imc::kByteAlphabet;
    const size_t unit = wide ? sizeof(imc::tok_t) : 1;
    imc::TextSession ses(file_bytes);
    IngestStage st;
    DevBuf<uint8_t> symbols;
    DevBuf<uint16_t> flags;
    DevBuf<imc::IngestSummary> sums, total;
    DevBuf<uint32_t> tile_off;
    SlabPass pass;
    const int passed = slab_pass(
        lk, fp, file_bytes, "ingest: ", st, 0, total,
        [&](size_t slab) -> int {
            const size_t tiles_max = (slab + TILE_SIZE - 1) / TILE_SIZE;
            HIP_TRY(symbols.alloc(ses.room * unit));
            HIP_TRY(flags.alloc(tiles_max * TILE_THREADS * sizeof(uint16_t)));
            HIP_TRY(sums.alloc(tiles_max * sizeof(imc::IngestSummary)));
            HIP_TRY(total.alloc(sizeof(imc::IngestSummary)));
            HIP_TRY(tile_off.alloc(tiles_max * sizeof(uint32_t)));
            return IMC_OK;
        },
        no_first_slab_work, [&](const uint8_t *buf, size_t fill, bool last) { return ses.cut(buf, fill, last); },
        [&](const uint8_t *d_slab, uint32_t n, uint32_t tiles) {
            hipLaunchKernelGGL(k_ing_text_summary, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, d_slab, n, (uint32_t)nsym, flags.get(), sums.get());
            hipLaunchKernelGGL(k_ing_scan, dim3(1), dim3(TILE_SCAN_THREADS), 0, g.stream, (const imc::IngestSummary *)sums.get(), tiles, tile_off.get(), total.get());
            hipLaunchKernelGGL(k_ing_text_scatter, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, d_slab, n, (const uint16_t *)flags.get(), (const uint32_t *)tile_off.get(),
                               symbols.get() + ses.cols * unit, (uint32_t)std::min<uint64_t>(ses.room - ses.cols, 0xffffffffu), wide ? 1 : 0);
        },
        [&](const imc::IngestSummary &all, const uint8_t *, size_t cut) { return ses.accept(all, cut, path); }, pass, declined);
    if (passed != IMC_OK || *declined) return passed;
    const uint64_t cols = ses.cols;
    if (int rc = check_columns(cols)) return rc;
    HIP_TRY(hipSetDevice(g.device));
    ObsOwner o = obs_new((size_t)cols, nsym);
    if (!o) return fail(IMC_ERR_OOM, kHostAllocFailed);
    int rc = adopt_device_symbols(o.get(), symbols.get(), (int)unit, ">= nsym");
    st.release();
    symbols.reset();
    if (rc == IMC_OK) rc = finish_device_chunk(lk, o.get());
    if (rc == IMC_OK) note_ingest(1, pass.sent, pass.slabs, cols);
    return obs_finish(rc, o, out);
}

// Cache file, fp behind its header h (checked).  The payload goes up packed: 2-bit files are unpacked by the device into the
// chunk's buffer, 8- and 16-bit payloads are validated and copied as symbols in device memory are.
int ingest_cache(std::unique_lock<std::mutex> &lk, FILE *fp, const imc::CacheHeader &h, const char *path, int nsym, imc_obs **out)
{
    const uint64_t L = h.L, payload = h.bits == 2 ? (L + 3) / 4 : L * (h.bits / 8);
    const size_t slab = (size_t)std::min<uint64_t>(ingest_slab_bytes() & ~(size_t)15, std::max<uint64_t>((payload + 15) & ~(uint64_t)15, imc::kMinSlabBytes));
    IngestStage st;
    DevBuf<uint8_t> raw;
    if (int rc = st.alloc(slab, payload > slab ? 2 : 1)) return rc;
    ObsOwner o = obs_new((size_t)L, nsym);
    if (!o) return fail(IMC_ERR_OOM, kHostAllocFailed);
    const size_t unit = o->wide_raw ? sizeof(imc::tok_t) : 1;
    uint64_t slabs = 0;
    auto fill = [&](int b, uint64_t, uint64_t len) -> int {
        return std::fread(st.host[b], 1, (size_t)len, fp) == (size_t)len ? IMC_OK : fail(IMC_ERR_IO, std::string("truncated cache ") + path);
    };
    auto work = [&]() -> int {
        if (h.bits == 2) {
            if (int rc = alloc_symbols(o.get())) return rc;
            if (int rc = ingest_pump(lk, st, payload, slab, &slabs, fill, [&](int b, uint64_t off, uint64_t len) -> int {
                    const uint32_t columns = (uint32_t)std::min<uint64_t>(4 * len, L - 4 * off);
                    HIP_TRY(hipMemcpyAsync(st.dev[b].get(), st.host[b], (size_t)len, hipMemcpyHostToDevice, g.stream));
                    hipLaunchKernelGGL(k_ing_unpack2, dim3((uint32_t)((len + TILE_THREADS - 1) / TILE_THREADS)), dim3(TILE_THREADS), 0, g.stream,
                                       (const uint8_t *)st.dev[b].get(), columns, o->d_sym + 4 * off * unit, o->wide_raw ? 1 : 0);
                    return IMC_OK;
                }))
                return rc;
            st.release();
            return validate_device_symbols(o->d_sym, (int)unit, (size_t)L, nsym, ">= nsym");
        }
        HIP_TRY(raw.alloc((size_t)payload));
        if (int rc = ingest_pump(lk, st, payload, slab, &slabs, fill, [&](int b, uint64_t off, uint64_t len) -> int {
                HIP_TRY(hipMemcpyAsync(raw.get() + off, st.host[b], (size_t)len, hipMemcpyHostToDevice, g.stream));
                return IMC_OK;
            }))
            return rc;
        st.release();
        const int rc = adopt_device_symbols(o.get(), raw.get(), (int)(h.bits / 8), ">= nsym");
        raw.reset();
        return rc;
    };
    int rc = work();
    if (rc == IMC_OK) rc = finish_device_chunk(lk, o.get());
    if (rc == IMC_OK) note_ingest(2, payload, slabs, L);
    return obs_finish(rc, o, out);
}

// A file the device parsers read: open for the length of the object; only a regular file has a size and can be read a
// second time by the host reader that takes what the device parser declines (a pipe cannot).
struct InputFile {
    FILE *fp = nullptr;
    bool regular = false;
    uint64_t bytes = 0;

    InputFile() = default;
    InputFile(const InputFile &) = delete;
    InputFile &operator=(const InputFile &) = delete;
    int open(const char *path)
    {
        fp = std::fopen(path, "rb");
        if (!fp) return fail(IMC_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
        struct stat sb;
        regular = fstat(fileno(fp), &sb) == 0 && S_ISREG(sb.st_mode);
        bytes = regular ? (uint64_t)sb.st_size : 0;
        return IMC_OK;
    }
    void close()
    {
        if (fp) std::fclose(fp);
        fp = nullptr;
    }
    ~InputFile() { close(); }
};

// imc_obs_create_from_text on the device path (arguments checked).  Opening the file, its size, the magic and the cache
// header are the host's business and need no device.
int obs_from_file_device(const char *path, int nsym, imc_obs **out, bool *declined)
{
    InputFile in;
    if (int rc = in.open(path)) return rc;
    if (!in.regular) { *declined = true; return IMC_OK; }
    FILE *fp = in.fp;
    char head[8];
    const size_t nh = std::fread(head, 1, 8, fp);
    const bool cache = nh == 8 && std::memcmp(head, imc::kCacheMagic, 8) == 0;
    imc::CacheHeader h;
    if (cache) {
        const imc::IoResult hr = imc::read_cache_header(fp, path, nsym, h);
        if (hr.code) return fail(hr.code, hr.msg);
        if (h.bits == 16 && nsym <= imc::kByteAlphabet) { *declined = true; return IMC_OK; }   // (the host reader narrows before it validates)
        if (int rc = check_columns(h.L)) return rc;
    } else
        std::rewind(fp);
    std::unique_lock<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    HIP_TRY(hipSetDevice(g.device));
    return cache ? ingest_cache(lk, fp, h, path, nsym, out) : ingest_text(lk, fp, in.bytes, path, nsym, out, declined);
}

// imc_obs_create_pairwise (arguments checked): the rule of imc::encode_pairwise on the device, nsym = 3.
int obs_from_pairwise(const char *seq1, const char *seq2, size_t L, imc_obs **out)
{
    std::unique_lock<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    HIP_TRY(hipSetDevice(g.device));
    const size_t columns = std::min<size_t>(ingest_slab_bytes() / 2, std::max<size_t>(L, imc::kMinSlabBytes / 2)), half = (columns + 15) & ~(size_t)15;
    IngestStage st;
    if (int rc = st.alloc(2 * half, L > half ? 2 : 1)) return rc;
    ObsOwner o = obs_new(L, 3);
    if (!o) return fail(IMC_ERR_OOM, kHostAllocFailed);
    uint64_t slabs = 0;
    int rc = alloc_symbols(o.get());
    if (rc == IMC_OK)
        rc = ingest_pump(lk, st, L, half, &slabs,
                         [&](int b, uint64_t off, uint64_t len) -> int {
                             std::memcpy(st.host[b], seq1 + off, (size_t)len);
                             std::memcpy(st.host[b] + half, seq2 + off, (size_t)len);
                             return IMC_OK;
                         },
                         [&](int b, uint64_t off, uint64_t len) -> int {
                             HIP_TRY(hipMemcpyAsync(st.dev[b].get(), st.host[b], half + (size_t)len, hipMemcpyHostToDevice, g.stream));
                             hipLaunchKernelGGL(k_ing_pairwise, dim3((uint32_t)((len + 4 * TILE_THREADS - 1) / (4 * TILE_THREADS))), dim3(TILE_THREADS), 0, g.stream,
                                                (const uint8_t *)st.dev[b].get(), (const uint8_t *)st.dev[b].get() + half, (uint32_t)len, o->d_sym + off);
                             return IMC_OK;
                         });
    st.release();
    if (rc == IMC_OK) rc = finish_device_chunk(lk, o.get());
    if (rc == IMC_OK) note_ingest(3, 2 * (uint64_t)L, slabs, L);
    return obs_finish(rc, o, out);
}

// ---- resident alignments ------------------------------------------------------------------------------------
// imc_aln_open_fasta: the file's bytes go up through the same slabs and staging buffers as a text observation file and
// are parsed there (kernels_align.hpp; the rules and the slab cut are align_tiles.hpp's): the kept bases of all slabs
// land back to back in one buffer of the file's size, every header reports where it stands, and the host takes the names
// from the pinned slab.  The state, the record count and the base count at the end of slab k are read from its total
// before slab k + 1 is queued.  A file the device parser declines is read by imc::read_fasta and its sequences uploaded.
void aln_release(imc_aln *a)
{
    if (a->pid == getpid()) dev_free(a->d_bases);
    a->d_bases = nullptr;
}

// FASTA file of file_bytes bytes, fp at its start, into a (empty).  *declined: the device parser does not take this file;
// a holds nothing then.
int aln_parse_device(std::unique_lock<std::mutex> &lk, FILE *fp, uint64_t file_bytes, imc_aln *a, bool *declined)
{
    const uint64_t room = (file_bytes + 15) & ~(uint64_t)15;
    imc::AlnSession ses;
    IngestStage st;
    DevBuf<uint8_t> bases;
    DevBuf<imc::AlnSummary> sums;
    DevBuf<AlnTileIn> tile_in;
    DevBuf<imc::AlnTotal> total;
    DevBuf<imc::AlnRecord> table;
    SlabPass pass;
    // a slab's records come back into pinned memory behind the two totals: the host takes the names from the slab's bytes
    auto fetch = [&](uint32_t have, uint32_t count, const imc::AlnRecord *&recs) {
        imc::AlnRecord *pinned = reinterpret_cast<imc::AlnRecord *>(static_cast<imc::AlnTotal *>(st.pinned) + 2);
        const int rc = [&]() -> int {
            HIP_TRY(hipSetDevice(g.device));
            HIP_TRY(hipMemcpyAsync(pinned, table.get() + have, count * sizeof(imc::AlnRecord), hipMemcpyDeviceToHost, g.stream));
            HIP_TRY(hipStreamSynchronize(g.stream));
            return IMC_OK;
        }();
        recs = pinned;
        return rc == IMC_OK ? imc::IoResult() : imc::io_fail(rc, g_err);
    };
    const int passed = slab_pass(
        lk, fp, file_bytes, "alignment: ", st, imc::kMaxAlnRecords * sizeof(imc::AlnRecord), total,
        [&](size_t slab) -> int {
            const size_t tiles_max = (slab + TILE_SIZE - 1) / TILE_SIZE;
            HIP_TRY(bases.alloc((size_t)room));
            HIP_TRY(sums.alloc(tiles_max * sizeof(imc::AlnSummary)));
            HIP_TRY(tile_in.alloc(tiles_max * sizeof(AlnTileIn)));
            HIP_TRY(total.alloc(sizeof(imc::AlnTotal)));
            HIP_TRY(table.alloc(imc::kMaxAlnRecords * sizeof(imc::AlnRecord)));
            return IMC_OK;
        },
        no_first_slab_work, [&](const uint8_t *buf, size_t fill, bool last) { return ses.cut(buf, fill, last); },
        [&](const uint8_t *d_slab, uint32_t n, uint32_t tiles) {
            hipLaunchKernelGGL(k_aln_summary, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, d_slab, n, ses.prev, sums.get());
            hipLaunchKernelGGL(k_aln_scan, dim3(1), dim3(TILE_SCAN_THREADS), 0, g.stream, (const imc::AlnSummary *)sums.get(), tiles, ses.state, tile_in.get(), total.get());
            hipLaunchKernelGGL(k_aln_scatter, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, d_slab, n, ses.prev, (const AlnTileIn *)tile_in.get(), bases.get(), ses.kept, room,
                               table.get(), (uint32_t)ses.names.size(), imc::kMaxAlnRecords);
        },
        [&](const imc::AlnTotal &t, const uint8_t *h_slab, size_t cut) { return ses.accept(t, fetch, h_slab, cut, room); }, pass, declined);
    if (passed != IMC_OK || *declined) return passed;
    if (ses.finish(a->length).code) { *declined = true; return IMC_OK; }
    a->names = std::move(ses.names);
    a->start = std::move(ses.start);
    a->d_bases = bases.release();                                       // the alignment owns the buffer now
    a->info[0] = 1; a->info[1] = pass.sent; a->info[2] = pass.slabs; a->info[3] = a->names.size();
    return IMC_OK;
}

// imc_aln_open_phylip: the same slabs and staging buffers, parsed by kernels_phylip.hpp (the rules: phylip_tiles.hpp).
// PHYLIP file of file_bytes bytes, fp at its start, into a (empty).  The host parses the header line from the first slab's
// staged bytes and sizes the resident buffer (n * length, record r at r * length), the line table and the name table from
// it; a slab is cut anywhere, and the cursor at the end of slab k is read from its total before slab k + 1 is queued.
// After the last slab the name lengths, the names and the last n lines of the line table come back: every record's kept
// bytes must be the header's length.  *declined: the device parser does not take this file; a holds nothing then.
int phy_parse_device(std::unique_lock<std::mutex> &lk, FILE *fp, uint64_t file_bytes, imc_aln *a, bool *declined)
{
    imc::PhySession ses(file_bytes);
    IngestStage st;
    DevBuf<uint8_t> bases, names;
    DevBuf<imc::PhySummary> sums;
    DevBuf<imc::PhyCursor> tile_in;
    DevBuf<imc::PhyTotal> total;
    DevBuf<uint32_t> cnt, off, nlen, part;
    imc::PhySizes sz{};
    SlabPass pass;
    bool at_eof = false;
    const int passed = slab_pass(
        lk, fp, file_bytes, "alignment: ", st, 0, total,
        [&](size_t slab) -> int {
            const size_t tiles_max = (slab + TILE_SIZE - 1) / TILE_SIZE;
            HIP_TRY(sums.alloc(tiles_max * sizeof(imc::PhySummary)));
            HIP_TRY(tile_in.alloc(tiles_max * sizeof(imc::PhyCursor)));
            HIP_TRY(total.alloc(sizeof(imc::PhyTotal)));
            HIP_TRY(cnt.alloc((size_t)ses.cap * sizeof(uint32_t)));
            HIP_TRY(off.alloc((size_t)ses.cap * sizeof(uint32_t)));
            return IMC_OK;
        },
        [&](const uint8_t *h_slab, size_t cut) -> int {                 // the header, and what is sized from it
            if (ses.begin(h_slab, cut, at_eof, st.slab, sz).code) return imc::kSlabDeclined;
            HIP_TRY(bases.alloc(sz.bases));
            HIP_TRY(names.alloc(sz.names));
            HIP_TRY(nlen.alloc(sz.nlen));
            HIP_TRY(part.alloc(sz.part));
            HIP_TRY(hipMemsetAsync(cnt.get(), 0, (size_t)ses.cap * sizeof(uint32_t), g.stream));
            HIP_TRY(hipMemsetAsync(nlen.get(), 0, sz.nlen, g.stream));
            HIP_TRY(hipMemsetAsync(names.get(), 0, sz.names, g.stream));
            HIP_TRY(hipMemsetAsync(total.get(), 0, sizeof(imc::PhyTotal), g.stream));
            return IMC_OK;
        },
        [&](const uint8_t *, size_t fill, bool last) { at_eof = last; return fill; },
        [&](const uint8_t *d_slab, uint32_t n, uint32_t tiles) {
            const uint32_t cap = ses.cap, nrec = ses.nrec, units = (uint32_t)(((uint64_t)sz.pieces * nrec + TILE_THREADS - 1) / TILE_THREADS);
            hipLaunchKernelGGL(k_phy_summary, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, d_slab, n, ses.prev, sums.get());
            hipLaunchKernelGGL(k_phy_scan, dim3(1), dim3(TILE_SCAN_THREADS), 0, g.stream, (const imc::PhySummary *)sums.get(), tiles, ses.at, tile_in.get(), total.get());
            hipLaunchKernelGGL(k_phy_count, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, d_slab, n, ses.prev, (const imc::PhyCursor *)tile_in.get(), nrec, cnt.get(),
                               nlen.get(), cap);
            hipLaunchKernelGGL(k_phy_partial, dim3(units), dim3(TILE_THREADS), 0, g.stream, (const uint32_t *)cnt.get(), (const imc::PhyTotal *)total.get(), ses.at.lines, cap,
                               nrec, sz.rows, sz.pieces, part.get());
            hipLaunchKernelGGL(k_phy_offsets, dim3(units), dim3(TILE_THREADS), 0, g.stream, (const uint32_t *)cnt.get(), off.get(), (const uint32_t *)part.get(),
                               (const imc::PhyTotal *)total.get(), ses.at.lines, cap, nrec, sz.rows, sz.pieces);
            hipLaunchKernelGGL(k_phy_scatter, dim3(tiles), dim3(TILE_THREADS), 0, g.stream, d_slab, n, ses.prev, (const imc::PhyCursor *)tile_in.get(), nrec, ses.length,
                               (const uint32_t *)off.get(), cap, bases.get(), names.get(), total.get());
        },
        [&](const imc::PhyTotal &t, const uint8_t *h_slab, size_t cut) { return ses.accept(t, h_slab[cut - 1]); }, pass, declined);
    if (passed != IMC_OK || *declined) return passed;
    // the names and every record's kept bytes: the last n lines of the table hold one line of every record
    uint32_t line = 0;
    if (ses.tail(line).code) { *declined = true; return IMC_OK; }
    const uint32_t nrec = ses.nrec;
    std::vector<uint32_t> name_len(nrec), tail_cnt(nrec), tail_off(nrec);
    std::vector<char> name_bytes(sz.names);
    HIP_TRY(hipSetDevice(g.device));
    HIP_TRY(hipStreamSynchronize(g.stream));
    HIP_TRY(hipMemcpy(name_len.data(), nlen.get(), (size_t)nrec * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(name_bytes.data(), names.get(), name_bytes.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tail_cnt.data(), cnt.get() + line, (size_t)nrec * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tail_off.data(), off.get() + line, (size_t)nrec * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ses.finish(name_len.data(), name_bytes.data(), tail_cnt.data(), tail_off.data(), a->names, a->start, a->length).code) { *declined = true; return IMC_OK; }
    a->d_bases = bases.release();                                       // the alignment owns the buffer now
    a->info[0] = 1; a->info[1] = pass.sent; a->info[2] = pass.slabs; a->info[3] = nrec;
    return IMC_OK;
}

// The records of the host reader into a: one buffer of the bases' size, uploaded record by record.
int aln_upload_host(const imc::FastaRecords &r, imc_aln *a)
{
    uint64_t total = 0;
    for (size_t k = 0; k < r.names.size(); ++k) {
        a->names.push_back(r.names[k]);
        a->start.push_back(total);
        a->length.push_back(r.seqs[k].size());
        total += r.seqs[k].size();
    }
    HIP_TRY(hipSetDevice(g.device));
    HIP_TRY(dev_alloc((void **)&a->d_bases, (size_t)((total + 15) & ~(uint64_t)15)));
    for (size_t k = 0; k < r.names.size(); ++k)
        if (!r.seqs[k].empty()) HIP_TRY(hipMemcpy(a->d_bases + a->start[k], r.seqs[k].data(), r.seqs[k].size(), hipMemcpyHostToDevice));
    a->info[0] = 0; a->info[1] = 0; a->info[2] = 0; a->info[3] = a->names.size();
    return IMC_OK;
}

// imc_aln_open_fasta, imc_aln_open_phylip: the format says which device parser runs and which host reader takes a file it
// declines.  Opening the file needs no device.
enum AlnFormat { kAlnFasta, kAlnPhylip };

imc::IoResult aln_read_host(AlnFormat format, const char *path, imc::FastaRecords &records)
{
    return format == kAlnFasta ? imc::read_fasta(path, records) : imc::read_phylip(path, records);
}

int aln_open(const char *path, AlnFormat format, imc_aln **out)
{
    if (!out || !path) return fail(IMC_ERR_ARG, "null argument");
    InputFile in;
    if (int rc = in.open(path)) return rc;
    std::unique_ptr<imc_aln> a(new (std::nothrow) imc_aln());
    if (!a) return fail(IMC_ERR_OOM, kHostAllocFailed);
    bool declined = !in.regular;
    {
        std::unique_lock<std::mutex> lk(g_mu);
        if (int rc = ensure_ctx()) return rc;
        HIP_TRY(hipSetDevice(g.device));
        a->pid = g.pid;
        a->device = g.device;
        if (in.regular) {
            const int rc = (format == kAlnFasta ? aln_parse_device : phy_parse_device)(lk, in.fp, in.bytes, a.get(), &declined);
            if (rc != IMC_OK) { (void)hipStreamSynchronize(g.stream); return rc; }
        }
    }
    in.close();
    if (declined) {                                     // the host reader, from the start of the file, without g_mu
        a->names.clear(); a->start.clear(); a->length.clear();
        imc::FastaRecords records;
        const imc::IoResult r = aln_read_host(format, path, records);
        if (r.code) return fail(r.code, r.msg);
        std::unique_lock<std::mutex> lk(g_mu);
        if (int rc = aln_upload_host(records, a.get())) {
            const std::string msg = g_err;
            aln_release(a.get());
            return fail(rc, msg);
        }
    }
    *out = a.release();
    return IMC_OK;
}

// imc_obs_create_from_alignment (arguments checked): K sequences of L bases each, resident at the given offsets.
int obs_from_alignment(const imc_aln *a, const uint64_t *offsets, int k, size_t L, imc_obs **out)
{
    std::unique_lock<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    if (a->pid != g.pid) return fail(IMC_ERR_HIP, "alignment was opened in another process");
    HIP_TRY(hipSetDevice(g.device));
    ObsOwner o = obs_new(L, k == 2 ? 3 : 65);
    if (!o) return fail(IMC_ERR_OOM, kHostAllocFailed);
    int rc = alloc_symbols(o.get());
    if (rc == IMC_OK && L) {
        const dim3 grid((uint32_t)((L + (size_t)ALN_COLUMNS * TILE_THREADS - 1) / ((size_t)ALN_COLUMNS * TILE_THREADS)));
        if (k == 2)
            hipLaunchKernelGGL(k_aln_columns<2>, grid, dim3(TILE_THREADS), 0, g.stream, (const uint8_t *)a->d_bases, offsets[0], offsets[1], (uint64_t)0, (uint32_t)L, o->d_sym);
        else
            hipLaunchKernelGGL(k_aln_columns<3>, grid, dim3(TILE_THREADS), 0, g.stream, (const uint8_t *)a->d_bases, offsets[0], offsets[1], offsets[2], (uint32_t)L, o->d_sym);
        if (hipGetLastError() != hipSuccess) rc = fail(IMC_ERR_HIP, "alignment: the column kernel could not be launched");
    }
    if (rc == IMC_OK) rc = finish_device_chunk(lk, o.get());
    if (rc == IMC_OK) note_ingest(4, 0, 0, L);
    return obs_finish(rc, o, out);
}

// The deepest level within alphabet_limit at which the chunk holds a token stream; -1: none, its raw symbols
// (the imc_obs_* read-outs).
int token_level(const imc_obs *obs, int alphabet_limit)
{
    int level = -1;
    if (obs->dict)
        for (int l = 0; l < imc::kNumLevels; ++l)
            if (obs->alphabet[l] <= alphabet_limit && obs->alphabet[l] > obs->nsym && obs->d_tok[l]) level = l;
    return level;
}

// ---- kernel table ---------------------------------------------------------------------------------

using ChainFn = void (*)(const ChainDesc *, int, uint32_t, uint32_t, const double *, const int *,
                         const int *, uint32_t, double *, int *, double *, int);

struct KernelChoice : imc::KernelFacts {   // the planner's facts of the entry (planner_host.hpp) + the kernels themselves
    void (*plain)(PropArgs) = nullptr;
    void (*zip)(PropArgs) = nullptr;
    ChainFn chain = nullptr;
    ChainFn chain_lds = nullptr;       // the same kernel with the step's vector handed round through LDS (IMC_CHAIN_LDS=1)
    void (*big_table_raw)(BigArgs) = nullptr;
    void (*big_table_level)(BigArgs, const uint16_t *, int) = nullptr;
    void (*big_prop)(BigArgs, const BigBlock *) = nullptr;
    int big_prop_waves = 0;        // wavefronts per workgroup of big_prop (NT, or 8 for the dealt-tiles variant)
    void (*big_vec)(BigArgs, const BigBlock *, int, int) = nullptr;
    void (*big_vec_tail)(BigArgs, const BigBlock *, int, int) = nullptr;   // rank-one hand-off: mat-vec chain over segment tails
    int big_vec_waves = 0;
    void (*zip2)(BigArgs) = nullptr;   // register-blocked token kernel (NP = 4 RB <= 24), else null
    void (*zip3)(BigArgs) = nullptr;   // ... its fp64-MFMA form (same launch geometry and block list)
    void (*zip4)(BigArgs) = nullptr;   // ... with the hybrid LDS / L2 operator table, and the kernels that build that table
    void (*zip4w)(BigArgs) = nullptr;  // ... on 16-bit token streams (dictionary levels beyond 256 tokens)
    void (*zip4s)(BigArgs) = nullptr, (*zip4sw)(BigArgs) = nullptr;   // ... with the STREAMED table (nothing cached in LDS)
    void (*zip4_raw)(BigArgs) = nullptr;
    void (*zip4_level)(BigArgs, int, int) = nullptr;
    void (*zip4_level2)(BigArgs, const int4 *, int, int, const double *) = nullptr;   // two dictionary depths per launch
    void (*zip4_level2_first)(BigArgs, const int4 *, int, int, const double *) = nullptr;   // ... the first one: parameters + raw operators too
    void (*zip4_level2_split)(BigArgs, const int4 *, int, int, const double *) = nullptr;         // ... column-split form, one token per wavefront
    void (*zip4_level2_split_first)(BigArgs, const int4 *, int, int, const double *) = nullptr;
    void (*zip4_level3)(BigArgs, const int4 *, int, int, const double *) = nullptr;        // three dictionary depths per launch
    void (*zip4_level3_first)(BigArgs, const int4 *, int, int, const double *) = nullptr;
    size_t (*zip4_level3_lds)(size_t) = nullptr;
    bool chain_self_emax = false;      // the stitch kernel finds the units' largest exponents itself (no k_emax launch)
    // (KernelFacts' flags say which of the planner's kernels the entry has)
    void note_kernels()
    {
        has_zip2 = zip2 != nullptr; has_zip3 = zip3 != nullptr; has_zip4 = zip4 != nullptr; has_zip4s = zip4s != nullptr;
        has_level2 = zip4_level2 != nullptr;
    }
};

template <int R, int G, int MW>
KernelChoice make_kc()
{
    constexpr int NP = R * G;
    KernelChoice k;
    k.R = R; k.G = G; k.NP = NP; k.VPW = 64 / G; k.minw = MW;
    k.zwaves = ZWAVES;
    k.z4_waves = Z2WAVES;
    k.plain = k_propagate<R, G, MW>;
    k.zip = k_zpropagate<R, G>;
    k.zip_lds = &ZipGeom<R, G>::lds_bytes;
    constexpr int CHAIN_D = NP <= 12 ? 6 : NP <= 24 ? 4 : NP <= 32 ? 3 : NP <= 64 ? 2 : 1;
    k.chain = k_chain<NP, CHAIN_D, CHAIN_STEP>;
    k.chain_lds = k_chain<NP, CHAIN_D, CHAIN_LDS>;
    k.chain_self_emax = true;          // (k_chain<NP, D > 0>: one wavefront, prefetch ring)
    if constexpr (NP % 4 == 0 && NP <= 24) {
        k.zip2 = k_zpropagate2<NP / 4>;
        k.zip2_lds = &Zip2Geom<NP / 4>::lds_bytes;
        k.zip3 = k_zpropagate3<NP / 4>;
        k.zip3_lds = &Zip3Geom<NP / 4>::lds_bytes;
        k.tok_doubles = Zip3Geom<NP / 4>::TOK;
        if constexpr (NP <= 24) {   // (NP = 24: 27-29 registers of the streamed form spill, 35-72 of the hybrid one)
            k.zip4 = k_zpropagate4<NP / 4, false, true>;
            k.zip4w = k_zpropagate4<NP / 4, true, true>;
            k.zip4s = k_zpropagate4<NP / 4, false, false>;
            k.zip4sw = k_zpropagate4<NP / 4, true, false>;
            k.zip4_raw = k_z4_raw<NP / 4>;
            k.zip4_level = k_z4_level<NP / 4>;
            k.zip4_level2 = k_z4_level2<NP / 4, false>;
            k.zip4_level2_first = k_z4_level2<NP / 4, true>;
            k.zip4_level2_split = k_z4_level2<NP / 4, false, Z4_SPLIT_WAVES>;
            k.zip4_level2_split_first = k_z4_level2<NP / 4, true, Z4_SPLIT_WAVES_FIRST>;
            k.zip4_level3 = k_z4_level3<NP / 4, false>;
            k.zip4_level3_first = k_z4_level3<NP / 4, true>;
            k.zip4_level3_lds = &Z4L3Geom<NP / 4>::lds_bytes;
            k.zip4_lds = &Zip4Geom<NP / 4>::lds_bytes;
            k.zip4_max_hot = &Zip4Geom<NP / 4>::max_hot;
        }
    }
    if constexpr (NP == 28 || NP == 32) {   // streamed scan only, four wavefronts per workgroup (build_plan: wide)
        k.tok_doubles = Zip3Geom<NP / 4>::TOK;
        k.zip4s = k_zpropagate4<NP / 4, false, false>;
        k.zip4sw = k_zpropagate4<NP / 4, true, false>;
        k.zip4_raw = k_z4_raw<NP / 4>;
        k.zip4_level = k_z4_level<NP / 4>;
        k.zip4_lds = &Zip4Geom<NP / 4>::lds_bytes;
        k.z4_waves = Zip4Shape<NP / 4>::WAVES;
        k.wide_blocked = true;
    }
    k.note_kernels();
    return k;
}

template <int NT, int NSLAB>
KernelChoice make_big()
{
    // NT = 6, 10, 14: one tile-row per wavefront would load the SIMDs unevenly -> tiles dealt over 8 wavefronts
    constexpr bool dealt = NT > 4 && NT % 4 != 0;
    KernelChoice k;
    k.G = NT; k.NP = 16 * NT;          // NT wavefronts per workgroup
    k.z4_waves = Z2WAVES;
    k.chain = k.chain_lds = k_chain<16 * NT, 0>;
    k.big_table_raw = k_big_table_raw<NT>;
    k.big_table_level = k_big_table_level<NT>;
    k.big_prop = k_big_propagate<NT, NSLAB>;
    if constexpr (dealt) k.big_prop = k_big_propagate_s<NT, NSLAB>;
    k.big_prop_waves = dealt ? BS_WAVES : NT;
    k.big_vec = k_big_vector<NT, false>;
    k.big_vec_tail = k_big_vector<NT, true>;
    k.big_vec_waves = BigVec<NT>::WAVES;
    k.big_nslab = NSLAB;
    k.big_lds = BigSlab<NT, NSLAB>::bytes;
    return k;
}

KernelChoice kChoices[] = {
    make_kc<4, 1, 2>(), make_kc<4, 2, 2>(), make_kc<4, 3, 2>(), make_kc<4, 4, 2>(), make_kc<4, 5, 2>(),
    make_kc<3, 8, 2>(), make_kc<2, 14, 2>(), make_kc<2, 16, 2>(), make_kc<2, 20, 1>(), make_kc<1, 48, 1>(),
    make_kc<1, 56, 1>(), make_kc<1, 64, 1>(),
    make_big<6, 1>(), make_big<7, 1>(), make_big<8, 2>(), make_big<9, 3>(), make_big<10, 2>(), make_big<12, 3>(), make_big<14, 7>(),
    make_big<16, 8>(),
};
constexpr int IMC_MAX_N = 256;

// MFMA GEMM-chain variants for 24 < N <= 64 (small workgroups, several per CU): used instead of the vector
// kernels when a launch is dominated by operator segments (long chunks).
KernelChoice kMidChoices[] = {make_big<2, 1>(), make_big<3, 1>(), make_big<4, 1>()};   // NP = 32, 48, 64

KernelChoice *choose_kernel(int N, bool prefer_gemm)
{
    if (prefer_gemm && N > 24 && N <= 64)
        for (auto &k : kMidChoices)
            if (k.NP >= N) return &k;
    for (auto &k : kChoices)
        if (k.NP >= N) return &k;
    return nullptr;
}

// ---- launch plan ----------------------------------------------------------------------------------

struct Group {             // one propagate launch
    // What imc::decide_groups decided (planner_host.hpp): the kernel family (`kind`, which everything reads directly or
    // through the predicates below), the stream (raw columns or a token level of the dictionary) and its alphabet, the
    // chunks, the segment length, the rank-one hand-off's checkpoints, the planner's estimates.
    using Kind = imc::GroupKind;
    imc::GroupDecision dec;
    imc::GroupGeometry geo;    // its vectors, chain segments, blocks and fused-tail records (imc::plan_geometry)
    imc::GroupSchedules sch;   // its workgroup lists, table-build schedules, hot set and phase table (imc::group_schedules)
    bool is_chain() const { return imc::is_chain(dec.kind); }
    bool is_blocked() const { return imc::is_blocked(dec.kind); }
    bool global_table() const { return dec.kind == Kind::BlockedGlobal; }
    std::shared_ptr<DictDev> dict;

    // operator table in global memory and its exponents: the chain families and the global-table scan
    DevBuf<double> d_Ctab;
    DevBuf<int> d_cex;

    struct Chain {         // ---- GemmChain / MatVecChain ----
        DevBuf<BigBlock> d_big_blocks;
        DevBuf<double> d_Cpack;                   // groups that run the mat-vec chain: packed copy of the table ([B][A][N][TS])
        // rank-one hand-off (GEMM chain only): operator segments run on the GEMM chain in rounds that end at the
        // checkpoints (token counts); after each round k_rank1_check tests the segments still on the chain, and those
        // that collapsed to u alpha^T finish on the mat-vec chain from that checkpoint.  The schedule is fixed per plan,
        // the decision per segment comes from the data of the evaluation: nothing is carried from call to call.
        DevBuf<BigBlock> d_tail_blocks;
        DevBuf<int> d_r1flag, d_r1at;
        DevBuf<double> d_r1u, d_r1alpha;
    } chain;

    struct Blocked {       // ---- BlockedLds / BlockedGlobal ----
        DevBuf<Z2Block> d_blocks;
        DevBuf<uint16_t> d_tab_order;             // merged tokens of the alphabet by dictionary depth
        DevBuf<int> d_tab_lvl;
        DevBuf<int4> d_tab_desc, d_tab_desc2, d_tab_desc3;   // global table: the descriptor lists of its build (GroupSchedules)
        DevBuf<uint16_t> d_hot;
        // fused tail (zip3_tail): the records; published operators, exponents, arrival counters
        DevBuf<Z2Tail> d_tails;
        DevBuf<double> d_tailX;
        DevBuf<int> d_tailE, d_tail_arrive;
    } blk;
};

struct Level {             // one level of the stitch hierarchy (level 0 = propagate output)
    uint32_t n_segs = 0, n_vecs = 0, n_chains = 0;
    DevBuf<uint32_t> d_vec0;
    DevBuf<uint8_t> d_first;
    DevBuf<ChainDesc> d_chains;      // chains that produce THIS level from the previous one
    DevBuf<double> d_P;
    DevBuf<int> d_EX, d_EMAX;
};

// What a cached plan answers to: the call's chunks and shape, and the options it was built under (opt: the context's
// record of that moment, the device's size and the per-call variables).  Two keys are equal when a plan of one may be
// replayed for the other: imc::same_plan_options decides it for the record, and the debug flags do not count.
struct PlanKey {
    std::vector<uint64_t> chunk_ids;
    int N = 0, S = 0, B = 0;
    bool op_mode = false;               // imc_forward_state(as_operator)
    imc::PlanOptions opt;
    bool operator==(const PlanKey &o) const
    {
        return chunk_ids == o.chunk_ids && N == o.N && S == o.S && B == o.B && op_mode == o.op_mode && opt.force_level == o.opt.force_level &&
               imc::same_plan_options(opt, o.opt);
    }
};

struct Plan {
    const PlanKey key;               // (key.opt: what the builder and every launch of this plan read their options from)
    KernelChoice *kc = nullptr;
    bool wide = false;               // 25-32 states on the blocked scan (build_plan: wide)
    const int &N = key.N, &S = key.S, &B = key.B;   // the key holds the call's shape: one copy (a Plan is neither copied nor moved)
    const int n_chunks = (int)key.chunk_ids.size();
    uint32_t n_segs = 0, n_vecs = 0;
    std::vector<Group> groups;
    size_t pstride = 0;
    DevBuf<SegDesc> d_segs;
    DevBuf<VecDesc> d_vecs;
    std::vector<Level> levels;       // levels[0] holds the propagate output
    DevBuf<int32_t> d_final_vec;     // per chunk: vector index in the last level, -1 for an empty chunk
    uint64_t chain_steps = 0;        // serial depth of the stitch (sum over levels of the longest chain)
    bool finish_fused = false;       // the last chain level writes the log-likelihoods itself (no k_finish launch)
    DevBuf<double> d_params, d_out;
    // pinned staging of the caller's parameters: two slots used alternately, each guarded by an event recorded behind
    // the call that read it, so a call only waits when the call issued two calls earlier is still running
    double *h_params[2] = {nullptr, nullptr};
    hipEvent_t ev_params[2] = {nullptr, nullptr};
    bool ev_used[2] = {false, false};
    int slot = 0;
    double *h_out = nullptr;                        // pinned, mapped: the synchronous path's k_finish writes results straight to the host
    double *h_out_dev = nullptr;                    // its device-visible alias
    double *h_params_dev[2] = {nullptr, nullptr};   // device-visible aliases of the staging slots (k_stage_params)
    // The plan's device buffers are shared by every call on these chunks.  Calls may arrive on different streams (the
    // library's own for the synchronous entry points, the caller's for imc_forward_batch_device): ev_params[slot] is
    // recorded behind each call, and a call on another stream than its predecessor's first waits for it.
    hipStream_t last_stream = nullptr;
    int last_slot = 0;
    bool have_last = false;
    // A synchronous call (run_batch) enqueues under g_mu, then waits for its results WITHOUT it, so that other threads can
    // enqueue their own evaluations behind it (round 2 held the one mutex across the wait: two Python threads with
    // distinct chunk sets serialised completely).  While it waits the plan is `busy`: a second synchronous call on the
    // SAME plan (they share the mapped result slots) waits on g_cv, and nothing releases a busy plan.
    bool busy = false;
    hipGraphExec_t graph = nullptr;                 // captured enqueue(), replayed by run_batch
    uint64_t calls = 0;
    uint64_t lp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::string kernels;
    explicit Plan(PlanKey k) : key(std::move(k)) {}
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    // The device buffers free themselves (DevBuf members: after this body, so the pinned slots and events now go
    // first where release() freed them last - no plan is busy or in flight when it is erased).
    ~Plan()
    {
        if (graph) (void)hipGraphExecDestroy(graph);
        for (int k = 0; k < 2; ++k) {
            if (h_params[k]) (void)hipHostFree(h_params[k]);
            if (ev_params[k]) (void)hipEventDestroy(ev_params[k]);
        }
        if (h_out) (void)hipHostFree(h_out);      // (a plan that never reached upload() makes no HIP call here)
    }
};

// Most recent first.  Erasing a plan from the list releases everything it holds.  The list itself is never destroyed
// (the idiom of g_guard): a static's destructor would free device memory at process exit - and in a forked child of an
// initialised parent, where a HIP call can hang; as before, no plan is released on either path.
std::list<std::unique_ptr<Plan>> &g_plans = *new std::list<std::unique_ptr<Plan>>();
constexpr size_t MAX_PLANS = 4;

// Wait (g_mu held through `lk`) until no synchronous call is waiting on any plan: callers that release plans.
void wait_all_idle(std::unique_lock<std::mutex> &lk)
{
    g_cv.wait(lk, [] {
        for (auto &p : g_plans)
            if (p->busy) return false;
        return true;
    });
}

void drop_plans() { g_plans.clear(); }

// Drop every plan that uses one of these chunks - plans hold raw pointers into the chunks' device buffers (g_mu held,
// no plan busy: wait_all_idle).
void drop_plans_using(imc_obs *const *obs, size_t n)
{
    for (auto it = g_plans.begin(); it != g_plans.end();) {
        bool uses = false;
        for (uint64_t id : (*it)->key.chunk_ids)
            for (size_t q = 0; q < n; ++q) uses |= id == obs[q]->id;
        it = uses ? g_plans.erase(it) : std::next(it);
    }
}

// Joint re-compression of the chunks of one alphabet (imc_obs_recompress; chunk work, but behind the plan list, whose plans it drops), called without g_mu: a new dictionary is
// trained on a sample drawn evenly from ALL the chunks, they are re-encoded with it, and it replaces the alphabet's
// dictionary.
int recompress_alphabet(int nsym, std::vector<imc_obs *> &obs, bool on_device)
{
    // (in creation order, not in address order: the training sample is the concatenation of the chunks' heads, and with
    // pointer order the dictionary - alphabet, token counts, now and then whether the byte phase filled its 256 entries
    // at all - changed from run to run of the same program)
    std::sort(obs.begin(), obs.end(), [](const imc_obs *x, const imc_obs *y) { return x->id < y->id; });
    obs.erase(std::unique(obs.begin(), obs.end()), obs.end());
    const bool wide_raw = nsym > imc::kByteAlphabet;
    const size_t unit = wide_raw ? sizeof(imc::tok_t) : 1;
    PhaseTimer tm;
    size_t total = 0;
    for (imc_obs *o : obs) total += o->L;
    if (total < imc::TrainLimits().train_min) return IMC_OK;
    // ---- sample: the raw symbols come back to the host (the chunks keep them on the device) - all of them for the host
    //      encoder, only the training heads when the device encodes ----
    //      With imc_set_device_training(1) the sample stays where it is: the heads are the pieces of a device training,
    //      and with the device encoder nothing comes back at all.
    const size_t share = imc::recompress_share(obs.size(), wide_raw);
    std::vector<std::vector<uint8_t>> raw(obs.size());
    bool train_on_device = false;
    size_t copied = 0;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        train_on_device = device_mode(&imc::Options::device_train) == 1;
        // nothing to gain if these chunks already share a dictionary trained on at least this much data
        // (a second Likelihood over the same forwarders, a subset of a recompressed set)
        bool same = obs[0]->dict != nullptr;
        for (imc_obs *o : obs) same = same && o->dict == obs[0]->dict;
        if (same && obs[0]->dict->trained_on >= total) return IMC_OK;
        HIP_TRY(hipSetDevice(g.device));
        for (size_t k = 0; k < obs.size() && !(train_on_device && on_device); ++k) {
            raw[k].resize((on_device ? std::min(obs[k]->L, share) : obs[k]->L) * unit);
            HIP_TRY(hipMemcpy(raw[k].data(), obs[k]->d_sym, raw[k].size(), hipMemcpyDeviceToHost));
            copied += raw[k].size();
        }
    }
    std::vector<uint8_t> sample;
    if (!train_on_device) sample = imc::recompress_sample(raw, share, unit);
    tm.mark();
    // ---- train (host, unlocked - or on the device, under the lock) ----
    std::shared_ptr<DictDev> nd;
    if (train_on_device) {
        std::vector<TrainPiece> pieces;
        size_t sample_len = 0;
        for (imc_obs *o : obs) {
            pieces.push_back({o->d_sym, (int)unit, std::min(o->L, share)});
            sample_len += pieces.back().n;
        }
        std::lock_guard<std::mutex> lk(g_mu);
        HIP_TRY(hipSetDevice(g.device));
        if (int rc = device_train(pieces.data(), pieces.size(), nsym, sample_len, total, &nd)) return rc;
    } else {
        imc::TrainStats st;
        nd = make_dictionary(symbols_in(sample, wide_raw), nsym, total, &st);
        std::vector<uint8_t>().swap(sample);
        std::lock_guard<std::mutex> lk(g_mu);
        note_training(0, st);
    }
    tm.mark();
    // ---- encode (host encoder only; unlocked) ----
    std::vector<imc::EncodedLevels> enc(obs.size());
    const bool zipped = nd->dict.alphabet > nsym;
    if (zipped && !on_device)
        for (size_t k = 0; k < obs.size(); ++k) {
            const HostSymbols sym = symbols_in(raw[k], wide_raw);
            imc::encode_levels(nd->dict, sym.bytes, sym.wide, obs[k]->L, enc[k]);
            std::vector<uint8_t>().swap(raw[k]);
        }
    tm.mark();
    // ---- install: swap the streams in under the lock ----
    std::unique_lock<std::mutex> lk(g_mu);
    wait_all_idle(lk);
    HIP_TRY(hipSetDevice(g.device));
    HIP_TRY(hipDeviceSynchronize());                 // nothing of these chunks is in flight any more
    drop_plans_using(obs.data(), obs.size());        // plans hold raw pointers into the old streams
    if (!zipped) return IMC_OK;                      // (incompressible sample: keep what the chunks have)
    if (int rc = publish_dictionary(nsym, nd)) return rc;   // later chunks of this alphabet share it too
    if (on_device) {                                 // all chunks of the alphabet in one batched run of passes
        for (imc_obs *o : obs) release_tokens(o);
        if (int rc = device_encode(nd, obs.data(), obs.size())) return rc;
    } else
        for (size_t k = 0; k < obs.size(); ++k) {
            release_tokens(obs[k]);
            if (int rc = install_encoding(obs[k], nd, enc[k])) return rc;
        }
    tm.mark();
    if (PhaseTimer::enabled())
        std::fprintf(stderr, "[imc host] recompress %zu chunks, %zu columns: copy back %.1f ms, train %.1f ms, encode %.1f ms, install %.1f ms (%s encoder, %s trainer, %zu symbol bytes to the host)\n",
                     obs.size(), total, tm.ms(0), tm.ms(1), tm.ms(2), tm.ms(3), on_device ? "device" : "host", train_on_device ? "device" : "host", copied);
    return IMC_OK;
}

void publish_last(const Plan *p)     // what imc_last_plan() / imc_last_kernels() report: the plan just enqueued
{
    for (int k = 0; k < 8; ++k) g.last_plan[k] = p->lp[k];
    g.last_kernels = p->kernels;
}

// Device allocations of one upload with a sticky error: after the first failure the later calls do nothing, and the
// caller checks `e` once at the end.  (Host-side work between the calls - schedules, block lists - still runs after a
// failure; only the device calls become no-ops, and the error reported is the first one.)
struct DevUpload {
    hipError_t e = hipSuccess;
    template <class T> void alloc(DevBuf<T> &d, size_t bytes)             // uninitialised
    {
        if (e == hipSuccess) e = d.alloc(std::max<size_t>(bytes, 16));
    }
    template <class T> void zeroed(DevBuf<T> &d, size_t bytes)            // zero-filled (padded operator columns stay 0)
    {
        alloc(d, bytes);
        if (e == hipSuccess) e = hipMemset(d.get(), 0, std::max<size_t>(bytes, 16));
    }
    template <class T, class V> void put(DevBuf<T> &d, const std::vector<V> &h)   // a host vector's device copy
    {
        static_assert(sizeof(T) == sizeof(V), "the device buffer holds the host vector's elements");
        alloc(d, h.size() * sizeof(V));
        if (e == hipSuccess && !h.empty()) e = hipMemcpy(d.get(), h.data(), h.size() * sizeof(V), hipMemcpyHostToDevice);
    }
    template <class F> void then(F f)                                     // any other step that returns a hipError_t
    {
        if (e == hipSuccess) e = f();
    }
};

// What is left of building a plan once the host-only functions have run (build_plan: imc::decide_groups,
// imc::plan_geometry, imc::group_schedules): the plan with its groups filled, the geometry, and the segment cuts resolved
// against the chunks' device streams.  upload() computes nothing: it evicts, allocates, copies and registers the plan.
struct PlanBuilder {
    std::unique_ptr<Plan> p;
    imc::PlanGeometry geo;
    std::vector<SegDesc> segs;          // all segments, chunk order

    int upload(Plan **out)
    {
        while (g_plans.size() >= MAX_PLANS) {            // least recently used first; a plan somebody waits on stays
            auto victim = g_plans.end();
            for (auto it = g_plans.begin(); it != g_plans.end(); ++it)
                if (!(*it)->busy) victim = it;
            if (victim == g_plans.end()) break;
            g_plans.erase(victim);
        }

        Plan *q = p.get();
        const KernelChoice *kc = q->kc;
        const int N = q->N, B = q->B, n_chunks = q->n_chunks;
        const std::vector<imc::HostLevel> &hl = geo.levels;
        DevUpload u;
        u.put(q->d_segs, segs);
        u.put(q->d_vecs, geo.vecs);
        u.put(q->d_final_vec, geo.final_vec);
        q->levels.resize(hl.size());
        for (size_t l = 0; l < hl.size(); ++l) {
            Level &lv = q->levels[l];
            lv.n_segs = (uint32_t)hl[l].vec0.size();
            lv.n_vecs = hl[l].n_vecs;
            lv.n_chains = (uint32_t)hl[l].chains.size();
            const size_t nv = std::max<size_t>(lv.n_vecs, 1), ns = std::max<size_t>(lv.n_segs, 1);
            u.put(lv.d_vec0, hl[l].vec0);
            u.put(lv.d_first, hl[l].first);
            u.put(lv.d_chains, hl[l].chains);
            u.zeroed(lv.d_P, (size_t)B * nv * kc->NP * 8);
            u.zeroed(lv.d_EX, (size_t)B * nv * 4);
            u.zeroed(lv.d_EMAX, (size_t)B * ns * 4);
        }
        for (Group &gr : q->groups) {
            Group::Blocked &bl = gr.blk;
            Group::Chain &ch = gr.chain;
            const imc::GroupSchedules &sch = gr.sch;
            const int A = gr.dec.A;
            if (gr.is_blocked()) u.put(bl.d_blocks, gr.geo.blocks);
            if (!gr.geo.tails.empty()) {
                const size_t slots = (size_t)B * n_chunks * gr.geo.tail_stride;
                u.put(bl.d_tails, gr.geo.tails);
                u.alloc(bl.d_tailX, slots * kc->tok_doubles * 8);
                u.alloc(bl.d_tailE, slots * 128);
                u.zeroed(bl.d_tail_arrive, (size_t)B * n_chunks * 4);
            }
            if (gr.global_table()) {
                u.put(bl.d_hot, sch.hot);
                u.alloc(gr.d_Ctab, (size_t)B * (A + 1) * kc->tok_doubles * 8);
                u.alloc(gr.d_cex, (size_t)B * (A + 1) * 4 + 16);
            }
            if (gr.is_blocked() && gr.dec.tokens) {
                u.put(bl.d_tab_order, sch.tab.order);
                u.put(bl.d_tab_lvl, sch.tab.lvl);
                if (gr.global_table()) {
                    u.put(bl.d_tab_desc, sch.tab_desc);
                    if (!sch.tab2.desc.empty()) u.put(bl.d_tab_desc2, sch.tab2.desc);
                    if (!sch.tab3.desc.empty()) u.put(bl.d_tab_desc3, sch.tab3.desc);
                }
            }
            if (!gr.is_chain()) continue;
            const size_t np2 = (size_t)kc->NP * kc->NP;
            u.put(ch.d_big_blocks, sch.big_blocks);
            u.alloc(gr.d_Ctab, (size_t)B * A * np2 * 8);
            if ((gr.dec.kind == Group::Kind::MatVecChain || gr.dec.rank1) && N < kc->NP && q->key.opt.pack_table)   // the mat-vec chain reads a packed copy
                u.alloc(ch.d_Cpack, (size_t)B * A * N * (size_t)(N + (N & 1)) * 8);
            u.alloc(gr.d_cex, (size_t)B * A * 4 + 16);
            if (gr.dec.rank1) {
                const size_t nrec = (size_t)B * segs.size();
                u.put(ch.d_tail_blocks, sch.tail_blocks);
                u.zeroed(ch.d_r1flag, nrec * 4);
                u.zeroed(ch.d_r1at, nrec * 4);
                u.alloc(ch.d_r1u, nrec * kc->NP * 8);
                u.alloc(ch.d_r1alpha, nrec * kc->NP * 8);
            }
        }
        u.alloc(q->d_params, (size_t)B * q->pstride * 8);
        u.alloc(q->d_out, (size_t)B * std::max(n_chunks, 1) * 8);
        for (int k = 0; k < 2; ++k) {
            u.then([&] { return hipHostMalloc((void **)&q->h_params[k], (size_t)B * q->pstride * 8, hipHostMallocMapped); });
            u.then([&] { return hipHostGetDevicePointer((void **)&q->h_params_dev[k], q->h_params[k], 0); });
            u.then([&] { return hipEventCreateWithFlags(&q->ev_params[k], hipEventDisableTiming); });
        }
        u.then([&] { return hipHostMalloc((void **)&q->h_out, (size_t)B * std::max(n_chunks, 1) * 8, hipHostMallocMapped); });
        u.then([&] { return hipHostGetDevicePointer((void **)&q->h_out_dev, q->h_out, 0); });
        if (u.e != hipSuccess)                           // (the half-built plan is released with this builder)
            return fail(u.e == hipErrorOutOfMemory ? IMC_ERR_OOM : IMC_ERR_HIP,
                        std::string("plan allocation: ") + hipGetErrorString(u.e));
        g_plans.push_front(std::move(p));
        *out = q;
        return IMC_OK;
    }
};

// The planner's facts of a call's chunks; dictionaries are numbered in the order of their first appearance.
void gather_facts(const imc_obs *const *chunks, int n_chunks, std::vector<imc::ChunkFacts> &cf, std::vector<imc::DictFacts> &df,
                  std::vector<std::shared_ptr<DictDev>> &dict_of)
{
    cf.resize(n_chunks);
    for (int f = 0; f < n_chunks; ++f) {
        const imc_obs *o = chunks[f];
        imc::ChunkFacts &c = cf[f];
        c.L = o->L; c.nsym = o->nsym; c.wide_raw = o->wide_raw;
        if (o->dict) {
            c.dict = (int)(std::find(dict_of.begin(), dict_of.end(), o->dict) - dict_of.begin());
            if (c.dict == (int)dict_of.size()) { dict_of.push_back(o->dict); df.push_back(imc::DictFacts{&o->dict->depth}); }
        }
        for (int l = 0; l < imc::kNumLevels; ++l)
            c.level[l] = imc::ChunkFacts::Level{o->d_tok[l] != nullptr, o->wide[l], o->ntok[l], o->alphabet[l], &o->tok_count[l]};
    }
}

int build_plan(const imc_obs *const *chunks, int n_chunks, int N, int S, int B, bool op_mode, Plan **out)
{
    // The options of this call: the context's record as it stands, the device's size, and the planner's three variables -
    // read here, once per call, not at context creation: tests set IMC_FORCE_LEVEL between calls.
    PlanKey key;
    key.chunk_ids.reserve(n_chunks);
    for (int f = 0; f < n_chunks; ++f) key.chunk_ids.push_back(chunks[f]->id);
    key.N = N; key.S = S; key.B = B; key.op_mode = op_mode;
    static_cast<imc::Options &>(key.opt) = g.opt;
    key.opt.cus = g.cus;
    const char *force_level = std::getenv("IMC_FORCE_LEVEL");   // (experiments / tests)
    key.opt.force_level = force_level ? std::atoi(force_level) : -1;
    key.opt.debug = std::getenv("IMC_DEBUG") != nullptr;
    key.opt.debug_levels = std::getenv("IMC_DEBUG_LEVELS") != nullptr;
    const imc::PlanOptions &opt = key.opt;
    for (auto it = g_plans.begin(); it != g_plans.end(); ++it) {
        if ((*it)->key == key) {
            g_plans.splice(g_plans.begin(), g_plans, it);
            *out = g_plans.front().get();
            return IMC_OK;
        }
    }
    std::vector<imc::ChunkFacts> cf;
    std::vector<imc::DictFacts> df;
    std::vector<std::shared_ptr<DictDev>> dict_of;
    gather_facts(chunks, n_chunks, cf, df, dict_of);

    KernelChoice *kc = choose_kernel(N, imc::prefer_gemm(opt, cf, N, S));
    if (!kc) return fail(IMC_ERR_ARG, "N exceeds the largest built kernel (" + std::to_string(IMC_MAX_N) + ")");
    if (kc->R == 0 && (kc->G == 7 || kc->G == 9) && kc + 1 < kChoices + sizeof(kChoices) / sizeof(kChoices[0]) &&
        imc::next_shape_hands_off(opt, *kc, *(kc + 1), cf, S, B))
        kc = kc + 1;
    imc::PlanDecision dec = imc::decide_groups(opt, *kc, false, cf, df, N, S, B, op_mode);
    // 25-32 states, automatic mode: the blocked scan is one more candidate (imc::wide_plan_wins)
    bool wide = false;
    KernelChoice *kw = (N > 24 && N <= 32) ? choose_kernel(N, false) : nullptr;
    if (kw && kw->wide_blocked && opt.wide_blocked != 0 && opt.compression == 1 && opt.kernel_pref == 0 && n_chunks > 0) {
        imc::PlanDecision wdec = imc::decide_groups(opt, *kw, true, cf, df, N, S, B, op_mode);
        if (imc::wide_plan_wins(opt, dec, kc->R == 0, wdec, cf, N)) {
            dec = std::move(wdec);
            kc = kw;
            wide = true;
        }
    }
    // ---- geometry and schedules (host-only, plan_host.hpp), then the one step that needs the chunk handles ----
    PlanBuilder pb;
    pb.p = std::make_unique<Plan>(std::move(key));
    Plan *p = pb.p.get();
    p->kc = kc; p->wide = wide;
    const bool mfma = kc->use3(p->key.opt.blocked_variant) || wide;     // the blocked kernels of this plan are the fp64-MFMA ones
    imc::PlanGeometry &geo = pb.geo = imc::plan_geometry(dec, cf, *kc, N, S, op_mode, mfma);
    if (geo.too_many_vectors) return fail(IMC_ERR_ARG, "too many vectors in one call");
    p->n_segs = (uint32_t)geo.segs.size();
    p->n_vecs = (uint32_t)geo.vecs.size();
    p->pstride = geo.pstride;
    p->chain_steps = geo.chain_steps;
    p->finish_fused = geo.finish_fused;
    for (const imc::SegCut &cut : geo.segs) {
        const imc::GroupDecision &gd = dec.groups[dec.chunk_group[cut.chunk]];
        const uint8_t *base = gd.tokens ? chunks[cut.chunk]->d_tok[gd.level] : chunks[cut.chunk]->d_sym;
        pb.segs.push_back(SegDesc{base + cut.offset * ((cut.flags & SEG_WIDE) ? 2 : 1), cut.len, cut.flags});
    }
    for (size_t q = 0; q < dec.groups.size(); ++q) {
        Group gr;
        gr.dec = std::move(dec.groups[q]);
        gr.geo = std::move(geo.groups[q]);
        if (gr.dec.dict >= 0) gr.dict = dict_of[gr.dec.dict];
        gr.sch = imc::group_schedules(p->key.opt, *kc, wide, gr.dec, geo, gr.geo, cf, gr.dict.get(), S, B);
        p->groups.push_back(std::move(gr));
    }
    return pb.upload(out);
}

int check_args(const imc_obs *const *chunks, int n_chunks, int B, int N, int S, const double *pis,
               const double *Ts, const double *Es)
{
    if (n_chunks < 0 || (n_chunks > 0 && !chunks)) return fail(IMC_ERR_ARG, "chunks is null");
    if (B < 1) return fail(IMC_ERR_ARG, "B must be >= 1");
    if (N < 1) return fail(IMC_ERR_ARG, "N must be >= 1");
    if (S < 1 || S > imc::kMaxRawAlphabet) return fail(IMC_ERR_ARG, "S must be in [1," + std::to_string(imc::kMaxRawAlphabet) + "]");
    if (!pis || !Ts || !Es) return fail(IMC_ERR_ARG, "null parameter pointer");
    for (int f = 0; f < n_chunks; ++f) {
        if (!chunks[f]) return fail(IMC_ERR_ARG, "null chunk handle");
        if (chunks[f]->pid != getpid()) return fail(IMC_ERR_ARG, "chunk handle was created in another process");
        if (chunks[f]->device != g.device && g.ready) return fail(IMC_ERR_ARG, "chunk lives on another device");
        if (chunks[f]->nsym > S) return fail(IMC_ERR_SYMBOL, "chunk alphabet larger than S");
    }
    return IMC_OK;
}

// Enqueue everything for one batch on `stream`.  Results land in plan->d_out ([B][n_chunks]).
// Pad the caller's parameters into the plan's pinned staging buffer (host work only).
int stage_params(Plan *p, const double *pis, const double *Ts, const double *Es, bool fixed_slot = false)
{
    KernelChoice *kc = p->kc;
    const int N = p->N, S = p->S, NP = kc->NP, B = p->B;
    p->slot = fixed_slot ? 0 : p->slot ^ 1;          // (a captured graph always copies from slot 0)
    if (p->ev_used[p->slot]) HIP_TRY(hipEventSynchronize(p->ev_params[p->slot]));
    for (int b = 0; b < B; ++b) {
        double *pp = p->h_params[p->slot] + (size_t)b * p->pstride;
        std::memset(pp, 0, p->pstride * 8);
        const double *pi = pis + (size_t)b * N, *T = Ts + (size_t)b * N * N, *E = Es + (size_t)b * N * S;
        for (int i = 0; i < N; ++i) pp[i] = pi[i];
        double *Tp = pp + NP;
        for (int j = 0; j < N; ++j) std::memcpy(Tp + (size_t)j * NP, T + (size_t)j * N, (size_t)N * 8);
        double *Et = pp + NP + (size_t)NP * NP;
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < N; ++i) Et[(size_t)s * NP + i] = E[(size_t)i * S + s];
    }
    return IMC_OK;
}

// ---- enqueue: shared state, then one function per kernel family --------------------------------------------

// What the launches of one enqueue() share.
struct Launch {
    Plan *p;
    hipStream_t stream;
    double *out;
    bool allow_tail;
    KernelChoice *kc = p->kc;
    const imc::PlanOptions &opt = p->key.opt;   // the options the plan was built under
    int B = p->B;
    bool fuse_head = false;       // the first table launch fetches the parameters itself: no k_stage_params, no k_z4_raw
    bool direct_params = false;   // the few workgroups of a small k_zpropagate3 launch fetch them themselves
    // Profiling: ev.a .. ev.b brackets the propagate kernel(s).  For k_zpropagate4, whose operator table is built by
    // launches of its own, ev.a goes between the table launches and the scan: "kernel_ms" is then the duration of the
    // scan launch itself - the number rocprofv3's per-kernel average has to agree with.
    bool prof = false, a_recorded = false;
    Ev3 ev{nullptr, nullptr, nullptr};
    bool split_used = false;      // a table launch took the column-split form
    bool tail_used = false;       // the propagate launch finishes the chunks itself (zip3_tail): no stitch launches

    int mark_a()
    {
        if (prof && !a_recorded) { HIP_TRY(hipEventRecord(ev.a, stream)); a_recorded = true; }
        return IMC_OK;
    }
    void note(const std::string &k) const { p->kernels += (p->kernels.empty() ? "" : "+") + k; }
    // imc_last_plan's numbers: segment length, vector-steps (and stream length, alphabet) of the column / token groups
    void account(const Group &gr) const
    {
        uint64_t *lp = p->lp;
        if (gr.dec.tokens) { lp[4] = gr.dec.seglen; lp[5] += gr.geo.vsteps * (uint64_t)B; lp[6] += gr.geo.stream_len; lp[7] = std::max(lp[7], (uint64_t)gr.dec.A); }
        else { lp[2] = gr.dec.seglen; lp[3] += gr.geo.vsteps * (uint64_t)B; }
    }
    int fetch_params();
    BigArgs blocked_args(const Group &gr);
    int big_table(const Group &gr, const BigArgs &ba) const;
    int matvec_chain(const Group &gr);
    int gemm_chain(const Group &gr);
    int z4_table(const Group &gr, const BigArgs &ba);
    int zip4(const Group &gr);
    int zip32(const Group &gr);
    int zpropagate(const Group &gr);
    int propagate(const Group &gr);
    int stitch() const;
};

const char *stream_tag(const Group &gr) { return gr.dec.tokens ? "[tokens]" : "[columns]"; }

// Opt a kernel in to LDS_BUDGET bytes of dynamic LDS: one hipFuncSetAttribute per function and device (g.lds_opted).
template <class Fn>
int allow_lds_budget(Fn *fn)
{
    const void *f = (const void *)fn;
    if (std::find(g.lds_opted.begin(), g.lds_opted.end(), f) != g.lds_opted.end()) return IMC_OK;
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    g.lds_opted.push_back(f);
    return IMC_OK;
}

// Parameter upload.  Small sets (every BASELINE shape but the 64-proposal batch at N = 150) are fetched by a kernel
// from the mapped staging slot: a copy command costs its own ~3 us plus a ~10 us hand-over between the copy and the
// first kernel (rocprofv3 kernel trace), a kernel in the same queue costs one launch.
int Launch::fetch_params()
{
    const size_t pbytes = (size_t)B * p->pstride * 8;
    // One streamed / hybrid-table group and nothing else (BASELINE config[1], the config[3] slice): the first table launch
    // fetches the parameters itself (k_z4_level2<., true>) - no k_stage_params, no k_z4_raw.
    int active = 0;
    const Group *only = nullptr;
    for (const Group &gr : p->groups)
        if (gr.geo.n_vecs) { ++active; only = &gr; }
    const size_t head_lds = p->pstride * 8;
    fuse_head = opt.fuse_head && active == 1 && only->global_table() && opt.table_pairs && only->blk.d_tab_desc2 && !only->sch.tab2.launches.empty() &&
                kc->zip4_level2_first && pbytes <= STAGE_KERNEL_MAX_BYTES && head_lds <= 16 * 1024;
    // ... and a SMALL launch of the LDS-table MFMA kernel (the reference's own data sizes: one alignment of 1e5..1e6
    // columns): each of its few workgroups fetches the parameter set itself
    direct_params = opt.fuse_head && active == 1 && only->dec.kind == Group::Kind::BlockedLds && kc->use3(opt.blocked_variant) && pbytes <= STAGE_KERNEL_MAX_BYTES &&
                    only->geo.blocks.size() * (size_t)B <= 32 && p->pstride * 8 <= 8192 &&
                    ((kc->blocked_lds(only->dec.A, opt.blocked_variant) + 15) & ~(size_t)15) + p->pstride * 8 <= LDS_BUDGET;
    if (fuse_head || direct_params) {
        // (nothing to enqueue here)
    } else if (pbytes <= STAGE_KERNEL_MAX_BYTES) {
        const unsigned n2 = (unsigned)(pbytes / 16);
        hipLaunchKernelGGL(k_stage_params, dim3((n2 + 255) / 256), dim3(256), 0, stream,
                           reinterpret_cast<const double2 *>(p->h_params_dev[p->slot]), reinterpret_cast<double2 *>(p->d_params.get()), n2);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemcpyAsync(p->d_params.get(), p->h_params[p->slot], pbytes, hipMemcpyHostToDevice, stream));
    }
    return IMC_OK;
}

PropArgs prop_args(const Plan *p, const Group &gr)
{
    PropArgs a;
    a.segs = p->d_segs.get(); a.vecs = p->d_vecs.get() + gr.geo.vec_begin; a.n_vecs = gr.geo.n_vecs; a.vec_base = gr.geo.vec_begin;
    a.n_vecs_total = p->n_vecs; a.N = p->N; a.S = p->S;
    a.params = p->d_params.get(); a.pstride = p->pstride; a.P = p->levels[0].d_P.get(); a.EX = p->levels[0].d_EX.get();
    a.A = gr.dec.A; a.tok_left = gr.dec.tokens ? gr.dict->d_left : nullptr; a.tok_right = gr.dec.tokens ? gr.dict->d_right : nullptr;
    return a;
}

// The BigArgs every kernel of the GEMM-chain and blocked families starts from: whole segments (phase 0), no table, no
// block list, no fused tail, the two-dimensional grid.  The families set what differs.
BigArgs common_args(const Plan *p, const Group &gr)
{
    BigArgs ba{};
    ba.segs = p->d_segs.get();
    ba.n_vecs_total = p->n_vecs; ba.n_segs = p->n_segs; ba.n_chunks = p->n_chunks;
    ba.N = p->N; ba.S = p->S; ba.A = gr.dec.A; ba.params = p->d_params.get(); ba.pstride = p->pstride; ba.PP = p->kc->NP;
    ba.tok_left = gr.dec.tokens ? gr.dict->d_left : nullptr; ba.tok_right = gr.dec.tokens ? gr.dict->d_right : nullptr;
    ba.Ctab = gr.d_Ctab.get(); ba.cex = gr.d_cex.get();
    ba.P = p->levels[0].d_P.get(); ba.EX = p->levels[0].d_EX.get();
    ba.t_to = INT_MAX;
    return ba;
}

// ---- operator table in global memory: GEMM chain and mat-vec chain (kernels_big.hpp) ----

BigArgs big_args(const Plan *p, const Group &gr)
{
    BigArgs ba = common_args(p, gr);
    ba.n_group_segs = (uint32_t)gr.geo.seg_ids.size();
    ba.Cpack = gr.chain.d_Cpack.get(); ba.TS = p->N + (p->N & 1);
    ba.phase = gr.dec.rank1 ? 1 : 0; ba.t_to = gr.dec.rank1 ? gr.dec.checkpoints[0] : INT_MAX;
    ba.r1flag = gr.chain.d_r1flag.get(); ba.r1at = gr.chain.d_r1at.get(); ba.r1u = gr.chain.d_r1u.get(); ba.r1alpha = gr.chain.d_r1alpha.get();
    return ba;
}

// Raw symbols, then the merged tokens: one launch per run of one dictionary depth (tokens of a depth are independent)
int Launch::big_table(const Group &gr, const BigArgs &ba) const
{
    if (gr.dec.rank1) HIP_TRY(hipMemsetAsync(gr.chain.d_r1flag.get(), 0, (size_t)p->B * p->n_segs * 4, stream));   // nothing certified yet
    hipLaunchKernelGGL(kc->big_table_raw, dim3((unsigned)p->S, (unsigned)p->B), dim3(kc->G * 64), 0, stream, ba);
    HIP_TRY(hipGetLastError());
    for (const auto &run : gr.sch.table_runs) {
        hipLaunchKernelGGL(kc->big_table_level, dim3((unsigned)run.second, (unsigned)p->B), dim3(kc->G * 64), 0,
                           stream, ba, (const uint16_t *)gr.dict->d_order, run.first);
        HIP_TRY(hipGetLastError());
    }
    return IMC_OK;
}

// Every chunk is one segment: k_big_vector, no operators.
int Launch::matvec_chain(const Group &gr)
{
    const BigArgs ba = big_args(p, gr);
    if (int rc = big_table(gr, ba)) return rc;
    const unsigned grid = B >= 8 ? 8u * (unsigned)gr.sch.big_blocks.size() * (unsigned)((B + 7) / 8)
                                 : (unsigned)gr.sch.big_blocks.size() * (unsigned)B;
    hipLaunchKernelGGL(kc->big_vec, dim3(grid), dim3(kc->big_vec_waves * 64), 0, stream, ba,
                       (const BigBlock *)gr.chain.d_big_blocks.get(), (int)gr.sch.big_blocks.size(), B);
    note("k_big_vector<" + std::to_string(kc->G) + ">" + stream_tag(gr));
    account(gr);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

// One workgroup per (segment, column slab): k_big_propagate, and the rounds of the rank-one hand-off.
int Launch::gemm_chain(const Group &gr)
{
    BigArgs ba = big_args(p, gr);
    if (int rc = big_table(gr, ba)) return rc;
    if (int rc = allow_lds_budget(kc->big_prop)) return rc;
    const dim3 prop_grid((unsigned)gr.sch.big_blocks.size(), (unsigned)B), prop_block(kc->big_prop_waves * 64);
    hipLaunchKernelGGL(kc->big_prop, prop_grid, prop_block, kc->big_lds, stream, ba, (const BigBlock *)gr.chain.d_big_blocks.get());
    note(std::string(kc->big_prop_waves != kc->G ? "k_big_propagate_s<" : "k_big_propagate<") + std::to_string(kc->G) + ">" + stream_tag(gr));
    if (gr.dec.rank1 && !gr.sch.tail_blocks.empty()) {
        // The first round of heads is done.  Per checkpoint: certify which of the operators still on the GEMM
        // chain collapsed to rank one, then run the others up to the next checkpoint; after the last one the
        // certified segments finish on the mat-vec chain and the rest on the GEMM chain.  Every launch covers
        // all segments and a workgroup with nothing to do exits at once, so there is no host round trip.
        for (size_t r = 0; r < gr.dec.checkpoints.size(); ++r) {
            HIP_TRY(hipGetLastError());
            ba.t_to = gr.dec.checkpoints[r];
            hipLaunchKernelGGL(k_rank1_check, dim3((unsigned)gr.sch.tail_blocks.size(), (unsigned)B), dim3(1024), 0, stream, ba,
                               (const BigBlock *)gr.chain.d_tail_blocks.get(), kc->NP);
            HIP_TRY(hipGetLastError());
            ba.t_from = gr.dec.checkpoints[r];
            ba.t_to = r + 1 < gr.dec.checkpoints.size() ? gr.dec.checkpoints[r + 1] : INT_MAX;
            if (r + 1 == gr.dec.checkpoints.size()) {   // the mat-vec tails first: they are the long launch
                const unsigned grid = B >= 8 ? 8u * (unsigned)gr.sch.tail_blocks.size() * (unsigned)((B + 7) / 8)
                                             : (unsigned)gr.sch.tail_blocks.size() * (unsigned)B;
                hipLaunchKernelGGL(kc->big_vec_tail, dim3(grid), dim3(kc->big_vec_waves * 64), 0, stream, ba,
                                   (const BigBlock *)gr.chain.d_tail_blocks.get(), (int)gr.sch.tail_blocks.size(), B);
                HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(kc->big_prop, prop_grid, prop_block, kc->big_lds, stream, ba, (const BigBlock *)gr.chain.d_big_blocks.get());
        }
        note("rank1-handoff");
    }
    account(gr);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

// ---- register-blocked token kernels (kernels_zip2.hpp .. kernels_zip4.hpp) ----

BigArgs Launch::blocked_args(const Group &gr)
{
    BigArgs ba = common_args(p, gr);
    ba.blocks = gr.blk.d_blocks.get();
    ba.n_group_segs = (uint32_t)gr.geo.blocks.size();
    ba.tab_order = gr.blk.d_tab_order.get(); ba.tab_lvl = gr.blk.d_tab_lvl.get(); ba.tab_nlvl = gr.sch.tab.nlvl;
    ba.hot = gr.blk.d_hot.get(); ba.n_hot = gr.sch.n_hot; ba.tab_desc = gr.blk.d_tab_desc.get();
    if (gr.blk.d_tails && (opt.fuse_tail == 2 || (opt.fuse_tail == 1 && gr.geo.tail_stride <= 4)) && allow_tail && (kc->use3(opt.blocked_variant) || p->wide)) {
        ba.tail = gr.blk.d_tails.get(); ba.tailX = gr.blk.d_tailX.get(); ba.tailE = gr.blk.d_tailE.get(); ba.tail_arrive = gr.blk.d_tail_arrive.get();
        ba.tail_out = out; ba.tail_stride = gr.geo.tail_stride;
        tail_used = true;
    }
    return ba;
}

// The hybrid table's operators in global memory (they stay in L2): raw symbols, then the merged tokens three, two or
// one dictionary depth per launch.
int Launch::z4_table(const Group &gr, const BigArgs &ba)
{
    const double *const staged = p->h_params_dev[p->slot], *const none = nullptr;
    bool head = fuse_head;              // the first launch: parameters + raw operators too
    if (!fuse_head) {
        hipLaunchKernelGGL(kc->zip4_raw, dim3((unsigned)p->S + 1, (unsigned)B), dim3(256), 0, stream, ba);
        HIP_TRY(hipGetLastError());
    }
    if (opt.table_pairs && (opt.table_triples == 1 || (opt.table_triples < 0 && kc->NP <= 12)) && gr.blk.d_tab_desc3 && kc->zip4_level3) {
        if (int rc = allow_lds_budget(kc->zip4_level3)) return rc;
        if (int rc = allow_lds_budget(kc->zip4_level3_first)) return rc;
        for (const auto &lc : gr.sch.tab3.launches) {          // three dictionary depths per launch, one wavefront per token
            const dim3 grid((unsigned)(lc.second + Z4L3_WAVES - 1) / Z4L3_WAVES, (unsigned)B);
            if (head)
                hipLaunchKernelGGL(kc->zip4_level3_first, grid, dim3(Z4L3_WAVES * 64), kc->zip4_level3_lds(p->pstride), stream, ba,
                                   (const int4 *)gr.blk.d_tab_desc3.get(), lc.first, lc.second, staged);
            else
                hipLaunchKernelGGL(kc->zip4_level3, grid, dim3(Z4L3_WAVES * 64), kc->zip4_level3_lds(0), stream, ba,
                                   (const int4 *)gr.blk.d_tab_desc3.get(), lc.first, lc.second, none);
            head = false;
            HIP_TRY(hipGetLastError());
        }
    } else if (opt.table_pairs && gr.blk.d_tab_desc2 && kc->zip4_level2) {
        const size_t split_max = opt.table_split_max >= 0 ? (size_t)opt.table_split_max : (size_t)4 * opt.cus;
        for (const auto &lc : gr.sch.tab2.launches) {          // two dictionary depths per launch
            if (opt.table_split && (size_t)lc.second * B <= split_max) {     // a latency launch: one token per wavefront
                if (head)
                    hipLaunchKernelGGL(kc->zip4_level2_split_first, dim3((unsigned)(lc.second + Z4_SPLIT_WAVES_FIRST - 1) / Z4_SPLIT_WAVES_FIRST, (unsigned)B),
                                       dim3(Z4_SPLIT_WAVES_FIRST * 64), p->pstride * 8, stream, ba,
                                       (const int4 *)gr.blk.d_tab_desc2.get(), lc.first, lc.second, staged);
                else
                    hipLaunchKernelGGL(kc->zip4_level2_split, dim3((unsigned)(lc.second + Z4_SPLIT_WAVES - 1) / Z4_SPLIT_WAVES, (unsigned)B),
                                       dim3(Z4_SPLIT_WAVES * 64), 0, stream, ba,
                                       (const int4 *)gr.blk.d_tab_desc2.get(), lc.first, lc.second, none);
                split_used = true;
            } else if (head)
                hipLaunchKernelGGL(kc->zip4_level2_first, dim3((unsigned)(lc.second + 3) / 4, (unsigned)B), dim3(64),
                                   p->pstride * 8, stream, ba,
                                   (const int4 *)gr.blk.d_tab_desc2.get(), lc.first, lc.second, staged);
            else
                hipLaunchKernelGGL(kc->zip4_level2, dim3((unsigned)(lc.second + 3) / 4, (unsigned)B), dim3(64), 0, stream, ba,
                                   (const int4 *)gr.blk.d_tab_desc2.get(), lc.first, lc.second, none);
            head = false;
            HIP_TRY(hipGetLastError());
        }
    } else
        for (int d = 0; d < gr.sch.tab.nlvl; ++d) {   // one launch per dictionary depth: kernel boundaries order the depths
            const int first = gr.sch.tab.lvl[d], count = gr.sch.tab.lvl[d + 1] - first;
            hipLaunchKernelGGL(kc->zip4_level, dim3((unsigned)(count + 3) / 4, (unsigned)B), dim3(64), 0, stream, ba, first, count);
            HIP_TRY(hipGetLastError());
        }
    return IMC_OK;
}

// k_zpropagate4: the table launches, then the scan caches the hot operators in LDS and streams the rest a step ahead.
int Launch::zip4(const Group &gr)
{
    BigArgs ba = blocked_args(gr);
    if (int rc = z4_table(gr, ba)) return rc;
    void (*scan)(BigArgs) = gr.sch.stream_table ? (gr.dec.wide_tokens ? kc->zip4sw : kc->zip4s) : (gr.dec.wide_tokens ? kc->zip4w : kc->zip4);
    if (int rc = allow_lds_budget(scan)) return rc;
    if (int rc = mark_a()) return rc;
    // XCD-affine grid (BigArgs::n_phases): with the two-dimensional grid every XCD's L2 sees the tables of all
    // B parameter sets
    dim3 scan_grid(ba.n_group_segs, (unsigned)B);
    if (opt.xcd_affine && B > 1) {
        const imc::PhaseTable &t = gr.sch.phases;
        ba.n_phases = t.n_phases;
        for (int k = 0; k < t.n_phases; ++k) { ba.ph_begin[k] = t.ph_begin[k]; ba.ph_first[k] = t.ph_first[k]; ba.ph_sets[k] = t.ph_sets[k]; }
        scan_grid = dim3((unsigned)t.grid);
    }
    hipLaunchKernelGGL(scan, scan_grid, dim3(kc->z4_waves * 64), kc->zip4_lds(gr.dec.A, gr.sch.n_hot), stream, ba);
    note(std::string("k_zpropagate4<") + std::to_string(kc->NP / 4) + (gr.dec.wide_tokens ? ",16" : "") + (gr.sch.stream_table ? ",streamed>" : ">") + stream_tag(gr));
    account(gr);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

// k_zpropagate3 (fp64 MFMA) / k_zpropagate2 (DPP, VALU): the table is built in LDS by the scan's own workgroups.
int Launch::zip32(const Group &gr)
{
    BigArgs ba = blocked_args(gr);
    const bool v3 = kc->use3(opt.blocked_variant);
    void (*scan)(BigArgs) = v3 ? kc->zip3 : kc->zip2;
    if (int rc = allow_lds_budget(scan)) return rc;
    size_t lds3 = kc->blocked_lds(gr.dec.A, opt.blocked_variant);
    if (direct_params) { ba.params_src = p->h_params_dev[p->slot]; lds3 = ((lds3 + 15) & ~(size_t)15) + p->pstride * 8; }
    hipLaunchKernelGGL(scan, dim3(ba.n_group_segs, (unsigned)p->B), dim3(Z2WAVES * 64), lds3, stream, ba);
    note(std::string(v3 ? "k_zpropagate3<" : "k_zpropagate2<") + std::to_string(kc->NP / 4) + ">" + stream_tag(gr));
    account(gr);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

// ---- vector kernels (kernels_zip.hpp, kernels_plain.hpp) ----

int Launch::zpropagate(const Group &gr)
{
    const size_t lds = kc->zip_lds(gr.dec.A);
    if (int rc = allow_lds_budget(kc->zip)) return rc;
    const uint32_t vpb = (uint32_t)(ZWAVES * kc->VPW);
    dim3 grid((gr.geo.n_vecs + vpb - 1) / vpb, (unsigned)p->B);
    hipLaunchKernelGGL(kc->zip, grid, dim3(ZWAVES * 64), lds, stream, prop_args(p, gr));
    note("k_zpropagate<" + std::to_string(kc->R) + "," + std::to_string(kc->G) + ">" + stream_tag(gr));
    account(gr);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

int Launch::propagate(const Group &gr)
{
    const uint32_t vpb = (uint32_t)(WPB * kc->VPW);
    dim3 grid((gr.geo.n_vecs + vpb - 1) / vpb, (unsigned)p->B);
    const size_t lds = ((size_t)WPB * kc->VPW * kc->NP + (size_t)p->S * kc->NP) * 8;
    if (lds > LDS_BUDGET) return fail(IMC_ERR_ARG, "emission table (S x N) too large for LDS");
    if (lds > 48 * 1024)                  // large alphabets: opt in to > 64 KB of dynamic LDS
        if (int rc = allow_lds_budget(kc->plain)) return rc;
    hipLaunchKernelGGL(kc->plain, grid, dim3(WPB * 64), lds, stream, prop_args(p, gr));
    note("k_propagate<" + std::to_string(kc->R) + "," + std::to_string(kc->G) + ">" + stream_tag(gr));
    account(gr);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

// ---- stitch (kernels_stitch.hpp): k_emax / k_chain per level, k_finish ----

int Launch::stitch() const
{
    const int N = p->N, NP = kc->NP;
    for (size_t l = 0; l + 1 < p->levels.size(); ++l) {
        const Level &in = p->levels[l], &ot = p->levels[l + 1];
        if (!in.n_segs || !ot.n_chains) continue;
        if (!kc->chain_self_emax) {   // (the single-wavefront chain kernels find the units' largest exponents themselves)
            hipLaunchKernelGGL(k_emax, dim3((in.n_segs + 255) / 256, (unsigned)B), dim3(256), 0, stream,
                               in.d_vec0.get(), in.d_first.get(), in.n_segs, in.n_vecs, N, in.d_EX.get(), in.d_EMAX.get());
            HIP_TRY(hipGetLastError());
        }
        const int threads = (int)round_up((size_t)NP, 64);
        const bool last_level = l + 2 == p->levels.size();
        hipLaunchKernelGGL(opt.chain_lds ? kc->chain_lds : kc->chain, dim3(ot.n_chains, (unsigned)B), dim3(threads), 0, stream,
                           ot.d_chains.get(), N, in.n_segs, in.n_vecs, in.d_P.get(), in.d_EX.get(), in.d_EMAX.get(),
                           ot.n_vecs, ot.d_P.get(), ot.d_EX.get(), (last_level && p->finish_fused) ? out : (double *)nullptr, p->n_chunks);
        HIP_TRY(hipGetLastError());
    }
    if (p->n_chunks && !p->finish_fused) {
        const Level &last = p->levels.back();
        hipLaunchKernelGGL(k_finish, dim3((p->n_chunks + 63) / 64, (unsigned)B), dim3(64), 0, stream,
                           p->d_final_vec.get(), p->n_chunks, N, NP, last.n_vecs, last.d_P.get(), last.d_EX.get(), out);
        HIP_TRY(hipGetLastError());
    }
    return IMC_OK;
}

// Enqueue one batch evaluation on `stream`: parameter upload, propagate, stitch.  Per-chunk results are written
// to `out` ([B][n_chunks]; device memory or mapped pinned host memory).  Contains no synchronisation, so the
// same call sequence can be captured into a hipGraph.
int enqueue(Plan *p, hipStream_t stream, double *out, bool allow_tail = true)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap);
    if (cap == hipStreamCaptureStatusNone && p->have_last && p->last_stream != stream)
        HIP_TRY(hipStreamWaitEvent(stream, p->ev_params[p->last_slot], 0));     // the plan's previous call ran on another stream
    Launch L{p, stream, out, allow_tail};
    if (int rc = L.fetch_params()) return rc;

    uint64_t *lp = p->lp;
    lp[0] = p->n_segs; lp[1] = p->n_vecs; lp[2] = lp[3] = lp[4] = lp[5] = lp[6] = lp[7] = 0;
    L.prof = g.profile && p->n_vecs;
    if (L.prof) { HIP_TRY(hipEventCreate(&L.ev.a)); HIP_TRY(hipEventCreate(&L.ev.b)); HIP_TRY(hipEventCreate(&L.ev.c)); }
    p->kernels.clear();
    for (const Group &gr : p->groups) {
        if (!gr.geo.n_vecs) continue;
        if (!gr.global_table())
            if (int rc = L.mark_a()) return rc;
        int rc = IMC_OK;
        switch (gr.dec.kind) {
        case Group::Kind::ColumnVector: rc = L.propagate(gr); break;
        case Group::Kind::TokenVector: rc = L.zpropagate(gr); break;
        case Group::Kind::BlockedLds: rc = L.zip32(gr); break;
        case Group::Kind::BlockedGlobal: rc = L.zip4(gr); break;
        case Group::Kind::GemmChain: rc = L.gemm_chain(gr); break;
        case Group::Kind::MatVecChain: rc = L.matvec_chain(gr); break;
        }
        if (rc) return rc;
    }
    if (int rc = L.mark_a()) return rc;
    if (L.prof) HIP_TRY(hipEventRecord(L.ev.b, stream));
    if (L.split_used) L.note("table-split");
    if (L.tail_used) L.note("fused-tail");
    if (!L.tail_used)
        if (int rc = L.stitch()) return rc;
    if (L.prof) {
        HIP_TRY(hipEventRecord(L.ev.c, stream));
        g.events.push_back(L.ev);
    }
    if (cap == hipStreamCaptureStatusNone) {
        // one event per call, behind its last kernel (an event record holds the queue for ~5 us: not in front of the
        // first kernel): it marks the staging slot free again and orders the plan's next call if that comes on
        // another stream
        HIP_TRY(hipEventRecord(p->ev_params[p->slot], stream));
        p->ev_used[p->slot] = true;
        p->last_stream = stream;
        p->last_slot = p->slot;
        p->have_last = true;
    }
    return IMC_OK;
}

// After a call has been synchronised: how many operator segments the rank-one test saw and how many it certified
// (at any checkpoint).  Statistics only: nothing here feeds back into later calls.
void collect_rank1_stats(Plan *p)
{
    g.r1_checked = g.r1_collapsed = 0;
    for (Group &gr : p->groups) {
        if (!gr.dec.rank1 || gr.sch.r1_segs.empty() || gr.dec.checkpoints.empty()) continue;
        std::vector<int> flags((size_t)p->B * p->n_segs);
        if (hipMemcpy(flags.data(), gr.chain.d_r1flag.get(), flags.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) continue;
        for (int b = 0; b < p->B; ++b)
            for (const auto &sl : gr.sch.r1_segs) {
                if ((int)sl.second <= gr.dec.checkpoints[0]) continue;
                ++g.r1_checked;
                g.r1_collapsed += flags[(size_t)b * p->n_segs + sl.first] ? 1 : 0;
            }
        if (getenv("IMC_DEBUG_R1")) {          // where each head was certified (diagnostics only)
            std::vector<int> at((size_t)p->B * p->n_segs);
            if (hipMemcpy(at.data(), gr.chain.d_r1at.get(), at.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) continue;
            std::map<int, int> hist;
            for (const auto &sl : gr.sch.r1_segs) hist[flags[sl.first] ? at[sl.first] : -1]++;
            fprintf(stderr, "[imc] rank-one hand-off: segment length %zu tokens, checkpoints", (size_t)gr.dec.seglen);
            for (int c : gr.dec.checkpoints) fprintf(stderr, " %d", c);
            fprintf(stderr, "\n[imc]   certified at (tokens: segments)");
            for (auto &kv : hist) fprintf(stderr, " %d:%d", kv.first, kv.second);
            fprintf(stderr, "\n");
        }
    }
}

// The caller of a synchronous entry point is waiting for the value.  k_finish writes the per-chunk results straight
// into mapped host memory; the slots are set to a sentinel (a NaN payload no computation produces) before the launch
// and the host polls them for up to two milliseconds - an evaluation of BASELINE config[1] takes 0.3 ms, and a
// blocking hipStreamSynchronize returns some 15-20 us after the last kernel has finished - before it falls back to
// the blocking wait.  The stream itself is idle a few microseconds later; later calls are ordered behind it anyway.
constexpr uint64_t OUT_SENTINEL = 0x7ff8dead5e471e15ull;

hipError_t wait_results(hipStream_t st, const double *h_out, size_t n)
{
    const volatile uint64_t *v = reinterpret_cast<const volatile uint64_t *>(h_out);
    const auto t0 = std::chrono::steady_clock::now();
    size_t k = 0;
    for (unsigned spin = 0;; ++spin) {
        while (k < n && v[k] != OUT_SENTINEL) ++k;
        if (k == n) { std::atomic_thread_fence(std::memory_order_acquire); return hipSuccess; }
        if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return hipStreamSynchronize(st);
    }
}

int run_batch(const imc_obs *const *chunks, int n_chunks, int B, int N, int S, const double *pis, const double *Ts,
              const double *Es, double *out_sum, double *out_per_chunk)
{
    std::unique_lock<std::mutex> lk(g_mu);
    static const bool dbg_host = std::getenv("IMC_DEBUG_HOST") != nullptr;     // diagnostics: host time per phase
    auto now = [] { return std::chrono::steady_clock::now(); };
    const auto h0 = now();
    if (int rc = ensure_ctx()) return rc;
    if (int rc = check_args(chunks, n_chunks, B, N, S, pis, Ts, Es)) return rc;
    HIP_TRY(hipSetDevice(g.device));
    Plan *p = nullptr;
    for (;;) {                                   // (the plan is looked up again after every wait: it may have been released)
        if (int rc = build_plan(chunks, n_chunks, N, S, B, false, &p)) return rc;
        if (!p->busy) break;
        g_cv.wait(lk);                           // another thread is waiting for this plan's results
    }
    struct Busy {                                // destroyed with g_mu held (declared after lk)
        Plan *p;
        explicit Busy(Plan *q) : p(q) { p->busy = true; }
        ~Busy() { p->busy = false; g_cv.notify_all(); }
    } busy(p);
    const auto h1 = now();
    if (int rc = stage_params(p, pis, Ts, Es, p->key.opt.use_graphs)) return rc;
    const size_t n_out = (size_t)B * n_chunks;
    for (size_t k = 0; k < n_out; ++k) reinterpret_cast<volatile uint64_t *>(p->h_out)[k] = OUT_SENTINEL;
    std::atomic_thread_fence(std::memory_order_release);
    const auto h2 = now();
    // First call of a plan runs eagerly (kernel attributes get set); the second is captured into a hipGraph that
    // every later call replays: one graph launch instead of ~8 stream operations per evaluation.
    const bool use_graph = !g.profile && p->key.opt.use_graphs && p->calls >= 1;
    if (use_graph && !p->graph) {
        hipGraph_t gr = nullptr;
        HIP_TRY(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue(p, g.stream, p->h_out_dev);
        const hipError_t ec = hipStreamEndCapture(g.stream, &gr);
        if (rc) { if (gr) (void)hipGraphDestroy(gr); return rc; }
        if (ec != hipSuccess) return fail(IMC_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
        const hipError_t ei = hipGraphInstantiate(&p->graph, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
        if (ei != hipSuccess) { p->graph = nullptr; return fail(IMC_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); }
    }
    if (use_graph) HIP_TRY(hipGraphLaunch(p->graph, g.stream));
    else if (int rc = enqueue(p, g.stream, p->h_out_dev)) return rc;
    ++p->calls;
    publish_last(p);
    const auto h3 = now();
    const hipStream_t st = g.stream;
    lk.unlock();                                 // other threads may enqueue their evaluations while this one waits
    const hipError_t ew = n_out ? wait_results(st, p->h_out, n_out) : hipStreamSynchronize(st);
    lk.lock();
    HIP_TRY(ew);
    const auto h4 = now();
    collect_rank1_stats(p);
    if (dbg_host) {
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        static double acc[5] = {0, 0, 0, 0, 0};
        static int n_acc = 0;
        acc[0] += us(h0, h1); acc[1] += us(h1, h2); acc[2] += us(h2, h3); acc[3] += us(h3, h4); acc[4] += us(h4, now());
        if (++n_acc % 20 == 0) {
            fprintf(stderr, "[imc] host us per call: check+plan %.1f  stage %.1f  enqueue %.1f  sync wait %.1f  stats %.1f\n",
                    acc[0] / 20, acc[1] / 20, acc[2] / 20, acc[3] / 20, acc[4] / 20);
            for (double &a : acc) a = 0.0;
        }
    }
    for (int b = 0; b < B; ++b) {
        double tot = 0.0;   // Python sum(): left to right from 0 (likelihood.py:33)
        for (int f = 0; f < n_chunks; ++f) {
            const double v = p->h_out[(size_t)b * n_chunks + f];
            if (out_per_chunk) out_per_chunk[(size_t)b * n_chunks + f] = v;
            tot += v;
        }
        if (out_sum) out_sum[b] = tot;
    }
    return IMC_OK;
}

// State export (imc_forward_state): the plan runs as usual, then every chunk's final vector (from pi) or transfer
// operator is copied out with its power-of-two exponents instead of being reduced to a log-likelihood.
int run_state(const imc_obs *const *chunks, int n_chunks, bool op_mode, int B, int N, int S, const double *pis,
              const double *Ts, const double *Es, double *out_state, int *out_exp)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    if (int rc = check_args(chunks, n_chunks, B, N, S, pis, Ts, Es)) return rc;
    if (!out_state || !out_exp) return fail(IMC_ERR_ARG, "output buffer is null");
    for (int f = 0; f < n_chunks; ++f)
        if (chunks[f]->L == 0) return fail(IMC_ERR_ARG, "imc_forward_state: empty chunk");
    HIP_TRY(hipSetDevice(g.device));
    Plan *p = nullptr;
    if (int rc = build_plan(chunks, n_chunks, N, S, B, op_mode, &p)) return rc;
    if (int rc = stage_params(p, pis, Ts, Es, p->key.opt.use_graphs)) return rc;
    if (int rc = enqueue(p, g.stream, p->d_out.get(), false)) return rc;      // (the log-likelihoods are not read here; the state comes from the stitch levels)
    ++p->calls;
    publish_last(p);
    const size_t per = op_mode ? (size_t)N * N : (size_t)N, pere = op_mode ? (size_t)N : 1;
    const size_t n_state = (size_t)B * n_chunks * per, n_exp = (size_t)B * n_chunks * pere;
    DevBuf<double> d_state;
    DevBuf<int> d_exp;
    hipError_t e = d_state.alloc(std::max<size_t>(n_state * 8, 16));
    if (e == hipSuccess) e = d_exp.alloc(std::max<size_t>(n_exp * 4, 16));
    if (e == hipSuccess) {
        const Level &last = p->levels.back();
        hipLaunchKernelGGL(k_export, dim3((unsigned)n_chunks, (unsigned)B), dim3(256), 0, g.stream, p->d_final_vec.get(), n_chunks, N,
                           p->kc->NP, last.n_vecs, last.d_P.get(), last.d_EX.get(), op_mode ? 1 : 0, d_state.get(), d_exp.get());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_state, d_state.get(), n_state * 8, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_exp, d_exp.get(), n_exp * 4, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? IMC_ERR_OOM : IMC_ERR_HIP, std::string("state export: ") + hipGetErrorString(e));
    return IMC_OK;
}

}  // namespace

#include "engine_model.hpp"
#include "engine_sample.hpp"

// =====================================================================================================
// C ABI
// =====================================================================================================

extern "C" {

const char *imc_version(void) { return "imcoal_fwd 0.2 (gfx950)"; }
const char *imc_last_error(void) { return g_err.c_str(); }

int imc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int imc_set_device(int device)
{
    std::unique_lock<std::mutex> lk(g_mu);
    if (device < 0) return fail(IMC_ERR_ARG, "negative device index");
    wait_all_idle(lk);
    if (g.ready && g.pid == getpid() && g.device != device) {
        drop_plans();
        g.dicts.clear();
        model_release();
        (void)hipStreamDestroy(g.stream);
        g.ready = false;
        g.lds_opted.clear();         // the dynamic-LDS opt-in is per device
    }
    g.device = device;
    return ensure_ctx();
}

int imc_obs_create(const uint8_t *sym, size_t L, int nsym, imc_obs **out)
{
    if (!out) return fail(IMC_ERR_ARG, "out is null");
    if (nsym < 1 || nsym > 256) return fail(IMC_ERR_ARG, "nsym must be in [1,256] for byte symbols (larger alphabets: imc_obs_create_i32)");
    if (L && !sym) return fail(IMC_ERR_ARG, "sym is null");
    if (int rc = check_columns(L)) return rc;
    for (size_t t = 0; t < L; ++t)
        if (sym[t] >= nsym) return fail(IMC_ERR_SYMBOL, "symbol " + std::to_string(sym[t]) + " at column " + std::to_string(t) + " >= nsym");
    return obs_upload(sym, nullptr, L, nsym, out);
}

int imc_obs_create_i32(const int32_t *sym, size_t L, int nsym, imc_obs **out)
{
    if (!out) return fail(IMC_ERR_ARG, "out is null");
    if (nsym < 1 || nsym > imc::kMaxRawAlphabet) return fail(IMC_ERR_ARG, "nsym must be in [1," + std::to_string(imc::kMaxRawAlphabet) + "]");
    if (L && !sym) return fail(IMC_ERR_ARG, "sym is null");
    if (int rc = check_columns(L)) return rc;
    for (size_t t = 0; t < L; ++t)
        if (sym[t] < 0 || sym[t] >= nsym)
            return fail(IMC_ERR_SYMBOL, "symbol " + std::to_string(sym[t]) + " at column " + std::to_string(t) + " outside [0,nsym)");
    if (nsym > imc::kByteAlphabet) {                    // e.g. the 257-symbol quartet alphabet (prepare-alignments.py:186-190)
        std::vector<imc::tok_t> wide(sym, sym + L);
        return obs_upload(nullptr, wide.data(), L, nsym, out);
    }
    std::vector<uint8_t> tmp(sym, sym + L);
    return obs_upload(tmp.data(), nullptr, L, nsym, out);
}

int imc_obs_create_from_text(const char *path, int nsym, imc_obs **out)
{
    if (!out || !path) return fail(IMC_ERR_ARG, "null argument");
    if (nsym < 1 || nsym > imc::kMaxRawAlphabet) return fail(IMC_ERR_ARG, "nsym must be in [1," + std::to_string(imc::kMaxRawAlphabet) + "]");
    bool on_device;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        on_device = device_mode(&imc::Options::device_ingest) == 1;
    }
    if (on_device) {                                    // parsed / unpacked on the device, unless the device parser declines the file
        bool declined = false;
        const int rc = obs_from_file_device(path, nsym, out, &declined);
        if (!declined) return rc;
    }
    if (nsym > imc::kByteAlphabet) {
        std::vector<imc::tok_t> wide;
        const imc::IoResult rw = imc::read_observation_file(path, nsym, wide);
        if (rw.code) return fail(rw.code, rw.msg);
        if (int rc = check_columns(wide.size())) return rc;
        return obs_upload(nullptr, wide.data(), wide.size(), nsym, out);
    }
    std::vector<uint8_t> sym;
    const imc::IoResult r = imc::read_observation_file(path, nsym, sym);
    if (r.code) return fail(r.code, r.msg);
    if (int rc = check_columns(sym.size())) return rc;
    return obs_upload(sym.data(), nullptr, sym.size(), nsym, out);
}

int imc_obs_create_pairwise(const char *seq1, const char *seq2, size_t L, imc_obs **out)
{
    // every argument check before any HIP call
    if (!out) return fail(IMC_ERR_ARG, "out is null");
    if (L && (!seq1 || !seq2)) return fail(IMC_ERR_ARG, "null sequence");
    if (int rc = check_columns(L)) return rc;
    return obs_from_pairwise(seq1, seq2, L, out);
}

int imc_set_device_ingest(int mode)
{
    return set_device_mode(&imc::Options::device_ingest, mode, "device ingest mode must be 0 (host parser) or 1 (device parser)");
}

int imc_last_ingest(uint64_t *out4)
{
    if (!out4) return fail(IMC_ERR_ARG, "out4 is null");
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < 4; ++i) out4[i] = g.last_ingest[i];
    return IMC_OK;
}

int imc_set_device_training(int mode)
{
    return set_device_mode(&imc::Options::device_train, mode, "device training mode must be 0 (host trainer) or 1 (device trainer)");
}

int imc_last_training(uint64_t *out4)
{
    if (!out4) return fail(IMC_ERR_ARG, "out4 is null");
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < 4; ++i) out4[i] = g.last_training[i];
    return IMC_OK;
}

int imc_read_observations(const char *path, int nsym, uint8_t *sym_out, size_t capacity, size_t *length)
{
    if (!path || !length) return fail(IMC_ERR_ARG, "null argument");
    if (nsym < 1 || nsym > 256) return fail(IMC_ERR_ARG, "nsym must be in [1,256]");
    std::vector<uint8_t> sym;
    const imc::IoResult r = imc::read_observation_file(path, nsym, sym);
    if (r.code) return fail(r.code, r.msg);
    *length = sym.size();
    if (sym_out && capacity >= sym.size() && !sym.empty()) std::memcpy(sym_out, sym.data(), sym.size());
    return IMC_OK;
}

int imc_write_cache(const char *path, const uint8_t *sym, size_t L, int nsym)
{
    if (!path || (L && !sym)) return fail(IMC_ERR_ARG, "null argument");
    if (nsym < 1 || nsym > 256) return fail(IMC_ERR_ARG, "nsym must be in [1,256]");
    const imc::IoResult r = imc::write_cache(path, sym, L, nsym);
    return r.code ? fail(r.code, r.msg) : IMC_OK;
}

int imc_encode_pairwise(const char *seq1, const char *seq2, size_t L, uint8_t *sym_out)
{
    if (L && (!seq1 || !seq2 || !sym_out)) return fail(IMC_ERR_ARG, "null argument");
    imc::encode_pairwise(seq1, seq2, L, sym_out);
    return IMC_OK;
}

int imc_encode_triplet(const char *seq1, const char *seq2, const char *seq3, size_t L, uint8_t *sym_out)
{
    if (L && (!seq1 || !seq2 || !seq3 || !sym_out)) return fail(IMC_ERR_ARG, "null argument");
    imc::encode_triplet(seq1, seq2, seq3, L, sym_out);
    return IMC_OK;
}

// imc_read_fasta, imc_read_phylip: record `index` of what the host reader gave, into the caller's buffers.
static int read_records(AlnFormat format, const char *path, int index, char *name_out, size_t name_capacity, char *seq_out, size_t seq_capacity, size_t *length, int *count)
{
    if (!path || !count) return fail(IMC_ERR_ARG, "null argument");
    imc::FastaRecords r;
    const imc::IoResult io = aln_read_host(format, path, r);
    if (io.code) return fail(io.code, io.msg);
    *count = (int)r.names.size();
    if (index < 0 || (size_t)index >= r.names.size()) {
        if (length) *length = 0;
        return name_out || seq_out ? fail(IMC_ERR_ARG, "record index out of range") : IMC_OK;
    }
    const std::string &name = r.names[(size_t)index], &seq = r.seqs[(size_t)index];
    if (length) *length = seq.size();
    if (name_out && name_capacity > name.size()) std::memcpy(name_out, name.c_str(), name.size() + 1);
    if (seq_out && seq_capacity >= seq.size() && !seq.empty()) std::memcpy(seq_out, seq.data(), seq.size());
    return IMC_OK;
}

int imc_read_fasta(const char *path, int index, char *name_out, size_t name_capacity, char *seq_out, size_t seq_capacity, size_t *length, int *count)
{
    return read_records(kAlnFasta, path, index, name_out, name_capacity, seq_out, seq_capacity, length, count);
}

int imc_read_phylip(const char *path, int index, char *name_out, size_t name_capacity, char *seq_out, size_t seq_capacity, size_t *length, int *count)
{
    return read_records(kAlnPhylip, path, index, name_out, name_capacity, seq_out, seq_capacity, length, count);
}

int imc_aln_open_fasta(const char *path, imc_aln **out) { return aln_open(path, kAlnFasta, out); }

int imc_aln_open_phylip(const char *path, imc_aln **out) { return aln_open(path, kAlnPhylip, out); }

int imc_aln_count(const imc_aln *aln) { return aln ? (int)aln->names.size() : 0; }

const char *imc_aln_name(const imc_aln *aln, int index)
{
    return aln && index >= 0 && (size_t)index < aln->names.size() ? aln->names[(size_t)index].c_str() : nullptr;
}

size_t imc_aln_length(const imc_aln *aln, int index)
{
    return aln && index >= 0 && (size_t)index < aln->length.size() ? (size_t)aln->length[(size_t)index] : 0;
}

int imc_aln_sequence(const imc_aln *aln, int index, char *out, size_t capacity)
{
    if (!aln) return fail(IMC_ERR_ARG, "aln is null");
    if (index < 0 || (size_t)index >= aln->names.size()) return fail(IMC_ERR_ARG, "record index out of range");
    const size_t n = (size_t)aln->length[(size_t)index];
    if (n && !out) return fail(IMC_ERR_ARG, "out is null");
    if (capacity < n) return fail(IMC_ERR_ARG, "capacity smaller than the sequence");
    if (!n) return IMC_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    if (aln->pid != g.pid) return fail(IMC_ERR_HIP, "alignment was opened in another process");
    HIP_TRY(hipSetDevice(aln->device));
    HIP_TRY(hipStreamSynchronize(g.stream));
    HIP_TRY(hipMemcpy(out, aln->d_bases + aln->start[(size_t)index], n, hipMemcpyDeviceToHost));
    return IMC_OK;
}

int imc_aln_info(const imc_aln *aln, uint64_t *out4)
{
    if (!aln || !out4) return fail(IMC_ERR_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out4[i] = aln->info[i];
    return IMC_OK;
}

int imc_aln_free(imc_aln *aln)
{
    if (!aln) return IMC_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    aln_release(aln);
    delete aln;
    return IMC_OK;
}

int imc_obs_create_from_alignment(const imc_aln *aln, const int *members, int k, imc_obs **out)
{
    // every argument check before any HIP call
    if (!out) return fail(IMC_ERR_ARG, "out is null");
    if (k != 2 && k != 3) return fail(IMC_ERR_ARG, "k must be 2 (pairwise rule) or 3 (triplet rule)");
    if (!aln || !members) return fail(IMC_ERR_ARG, "null argument");
    uint64_t offsets[3] = {0, 0, 0};
    for (int j = 0; j < k; ++j) {
        if (members[j] < 0 || (size_t)members[j] >= aln->names.size())
            return fail(IMC_ERR_ARG, "member " + std::to_string(members[j]) + " is not a record of the alignment (" + std::to_string(aln->names.size()) + " records)");
        offsets[j] = aln->start[(size_t)members[j]];
    }
    const uint64_t L = aln->length[(size_t)members[0]];
    for (int j = 1; j < k; ++j)
        if (aln->length[(size_t)members[j]] != L)
            return fail(IMC_ERR_ARG, "sequences differ in length: " + aln->names[(size_t)members[0]] + " has " + std::to_string(L) + " bases, " +
                                         aln->names[(size_t)members[j]] + " has " + std::to_string(aln->length[(size_t)members[j]]));
    if (int rc = check_columns(L)) return rc;
    return obs_from_alignment(aln, offsets, k, (size_t)L, out);
}

size_t imc_obs_length(const imc_obs *obs) { return obs ? obs->L : 0; }
int imc_obs_nsym(const imc_obs *obs) { return obs ? obs->nsym : 0; }

size_t imc_obs_compressed_length(const imc_obs *obs, int alphabet_limit, int *alphabet_used)
{
    if (!obs) return 0;
    const int level = token_level(obs, alphabet_limit);
    if (alphabet_used) *alphabet_used = level >= 0 ? obs->alphabet[level] : obs->nsym;
    return level >= 0 ? obs->ntok[level] : obs->L;
}

int imc_obs_dictionary(const imc_obs *obs, int alphabet_limit, uint16_t *left, uint16_t *right, size_t capacity, int *alphabet_used)
{
    if (!obs || !alphabet_used) return fail(IMC_ERR_ARG, "null argument");
    const int level = token_level(obs, alphabet_limit), used = level >= 0 ? obs->alphabet[level] : obs->nsym;
    *alphabet_used = used;
    if ((left || right) && capacity < (size_t)(used - obs->nsym)) return fail(IMC_ERR_ARG, "capacity smaller than the number of merged tokens");
    for (int z = obs->nsym; z < used; ++z) {
        if (left) left[z - obs->nsym] = obs->dict->dict.left[z];
        if (right) right[z - obs->nsym] = obs->dict->dict.right[z];
    }
    return IMC_OK;
}

int imc_obs_tokens(const imc_obs *obs, int alphabet_limit, uint16_t *tokens, size_t capacity, size_t *length, int *alphabet_used)
{
    if (!obs || !length) return fail(IMC_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g_mu);
    if (obs->pid != getpid()) return fail(IMC_ERR_ARG, "chunk handle was created in another process");
    const int level = token_level(obs, alphabet_limit);
    const size_t n = level >= 0 ? obs->ntok[level] : obs->L;
    *length = n;
    if (alphabet_used) *alphabet_used = level >= 0 ? obs->alphabet[level] : obs->nsym;
    if (!tokens) return IMC_OK;
    if (capacity < n) return fail(IMC_ERR_ARG, "capacity smaller than the stream");
    if (int rc = ensure_ctx()) return rc;
    HIP_TRY(hipSetDevice(obs->device));
    const bool wide = level >= 0 ? obs->wide[level] : obs->wide_raw;
    const uint8_t *src = level >= 0 ? obs->d_tok[level] : obs->d_sym;
    if (wide) HIP_TRY(hipMemcpy(tokens, src, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    else {
        std::vector<uint8_t> tmp(n);
        if (n) HIP_TRY(hipMemcpy(tmp.data(), src, n, hipMemcpyDeviceToHost));
        for (size_t t = 0; t < n; ++t) tokens[t] = tmp[t];
    }
    return IMC_OK;
}

// Joint re-compression (see the header).  The first sufficiently long chunk of an alphabet trains the dictionary that
// every later chunk shares; when a data set arrives as many chunks, that sample is one chunk: recompress_alphabet()
// replaces it, alphabet by alphabet.
int imc_obs_recompress(imc_obs *const *chunks, int n_chunks)
{
    if (n_chunks < 0 || (n_chunks > 0 && !chunks)) return fail(IMC_ERR_ARG, "chunks is null");
    std::map<int, std::vector<imc_obs *>> by_alphabet;
    bool on_device = false;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ctx()) return rc;
        if (!g.opt.compression) return IMC_OK;
        on_device = g.opt.device_encode == 1;
        for (int f = 0; f < n_chunks; ++f) {
            imc_obs *o = chunks[f];
            if (!o) return fail(IMC_ERR_ARG, "chunk is null");
            if (o->pid != g.pid) return fail(IMC_ERR_HIP, "chunk was created in another process");
            if (imc::compressible(o->L, o->nsym)) by_alphabet[o->nsym].push_back(o);
        }
    }
    for (auto &kv : by_alphabet)
        if (int rc = recompress_alphabet(kv.first, kv.second, on_device)) return rc;
    return IMC_OK;
}

int imc_obs_create_device(const void *d_sym, size_t L, int nsym, int sym_bytes, void *hip_stream, imc_obs **out)
{
    // every argument check before any HIP call
    if (!out) return fail(IMC_ERR_ARG, "out is null");
    if (sym_bytes != 1 && sym_bytes != 2 && sym_bytes != 4) return fail(IMC_ERR_ARG, "sym_bytes must be 1, 2 or 4");
    if (nsym < 1 || nsym > imc::kMaxRawAlphabet) return fail(IMC_ERR_ARG, "nsym must be in [1," + std::to_string(imc::kMaxRawAlphabet) + "]");
    if (sym_bytes == 1 && nsym > imc::kByteAlphabet) return fail(IMC_ERR_ARG, "byte symbols cannot carry more than 256 symbols");
    if (L && !d_sym) return fail(IMC_ERR_ARG, "d_sym is null");
    if (int rc = check_columns(L)) return rc;
    return obs_from_device(d_sym, L, nsym, sym_bytes, (hipStream_t)hip_stream, out);
}

int imc_obs_token_counts(const imc_obs *obs, int alphabet_limit, uint32_t *counts, size_t capacity, int *alphabet_used)
{
    if (!obs || !alphabet_used) return fail(IMC_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g_mu);
    if (obs->pid != getpid()) return fail(IMC_ERR_ARG, "chunk handle was created in another process");
    const int level = token_level(obs, alphabet_limit), used = level >= 0 ? obs->alphabet[level] : obs->nsym;
    *alphabet_used = used;
    if (!counts) return IMC_OK;
    if (capacity < (size_t)used) return fail(IMC_ERR_ARG, "capacity smaller than the alphabet");
    for (int z = 0; z < used; ++z)
        counts[z] = level >= 0 && (size_t)z < obs->tok_count[level].size() ? obs->tok_count[level][z] : 0u;   // (zeros where the level keeps no counts)
    return IMC_OK;
}

int imc_set_device_encoding(int mode)
{
    return set_device_mode(&imc::Options::device_encode, mode, "device encoding mode must be 0 (host encoder) or 1 (device encoder)");
}

int imc_obs_free(imc_obs *obs)
{
    if (!obs) return IMC_OK;
    std::unique_lock<std::mutex> lk(g_mu);
    wait_all_idle(lk);
    if (obs->pid == getpid() && g.ready) {
        drop_plans_using(&obs, 1);
        (void)hipSetDevice(obs->device);
        obs_release(obs);
    }
    delete obs;
    return IMC_OK;
}

int imc_forward_state(const imc_obs *const *chunks, int n_chunks, int as_operator, int B, int N, int S, const double *pis,
                      const double *Ts, const double *Es, double *out_state, int *out_exp)
{
    return run_state(chunks, n_chunks, as_operator != 0, B, N, S, pis, Ts, Es, out_state, out_exp);
}

int imc_forward(const imc_obs *const *chunks, int n_chunks, int N, int S, const double *pi, const double *T,
                const double *E, double *out_loglik)
{
    if (!out_loglik) return fail(IMC_ERR_ARG, "out_loglik is null");
    return run_batch(chunks, n_chunks, 1, N, S, pi, T, E, out_loglik, nullptr);
}

int imc_forward_batch(const imc_obs *const *chunks, int n_chunks, int B, int N, int S, const double *pis,
                      const double *Ts, const double *Es, double *out_logliks)
{
    if (!out_logliks) return fail(IMC_ERR_ARG, "out_logliks is null");
    return run_batch(chunks, n_chunks, B, N, S, pis, Ts, Es, out_logliks, nullptr);
}

int imc_forward_batch_per_chunk(const imc_obs *const *chunks, int n_chunks, int B, int N, int S, const double *pis,
                                const double *Ts, const double *Es, double *out_per_chunk)
{
    if (!out_per_chunk) return fail(IMC_ERR_ARG, "out_per_chunk is null");
    return run_batch(chunks, n_chunks, B, N, S, pis, Ts, Es, nullptr, out_per_chunk);
}

int imc_forward_batch_device(const imc_obs *const *chunks, int n_chunks, int B, int N, int S, const double *pis,
                             const double *Ts, const double *Es, double *d_out_partial, void *hip_stream)
{
    if (!d_out_partial) return fail(IMC_ERR_ARG, "d_out_partial is null");
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    if (int rc = check_args(chunks, n_chunks, B, N, S, pis, Ts, Es)) return rc;
    HIP_TRY(hipSetDevice(g.device));
    // NULL is the default stream, as everywhere in HIP - NOT the library's own (non-blocking) stream: the caller goes on
    // to use d_out_partial on the stream it named (torch's default stream has the handle 0), and work queued on a
    // non-blocking stream would not be ordered before that use.
    hipStream_t st = (hipStream_t)hip_stream;
    Plan *p = nullptr;
    if (int rc = build_plan(chunks, n_chunks, N, S, B, false, &p)) return rc;
    // no stream synchronisation here: the parameters go through the two-slot pinned staging (stage_params waits only
    // for the upload issued two calls ago), and nothing is read back - the call returns once everything is enqueued
    if (int rc = stage_params(p, pis, Ts, Es, p->key.opt.use_graphs)) return rc;
    if (int rc = enqueue(p, st, p->d_out.get())) return rc;
    ++p->calls;
    publish_last(p);
    hipLaunchKernelGGL(k_sum_chunks, dim3((B + 63) / 64), dim3(64), 0, st, p->d_out.get(), n_chunks, B, d_out_partial);
    HIP_TRY(hipGetLastError());
    return IMC_OK;
}

int imc_set_segment_length(size_t columns)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g.opt.seg_override = columns;
    return IMC_OK;
}

int imc_set_compression(int mode)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (mode < 0 || mode > 5) return fail(IMC_ERR_ARG, "compression mode must be in [0,5]");
    g.opt.compression = (mode == 1 || mode == 2 || mode == 3) ? 1 : 0;
    g.opt.kernel_pref = (mode == 2 || mode == 4) ? 1 : (mode == 3 || mode == 5) ? 2 : 0;
    return IMC_OK;
}

int imc_dictionary_reset(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g.dicts.clear();   // chunks already created keep (and share) the dictionary they were encoded with
    return IMC_OK;
}

int imc_profile_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g.profile = on != 0;
    return IMC_OK;
}

int imc_profile_read(double *ms_propagate, double *ms_stitch, uint64_t *n_propagate, uint64_t *n_stitch)
{
    std::lock_guard<std::mutex> lk(g_mu);
    double mp = 0.0, ms = 0.0;
    for (auto &ev : g.events) {
        HIP_TRY(hipEventSynchronize(ev.c));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev.a, ev.b));
        mp += t;
        HIP_TRY(hipEventElapsedTime(&t, ev.b, ev.c));
        ms += t;
        (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); (void)hipEventDestroy(ev.c);
    }
    if (ms_propagate) *ms_propagate = mp;
    if (ms_stitch) *ms_stitch = ms;
    if (n_propagate) *n_propagate = g.events.size();
    if (n_stitch) *n_stitch = g.events.size();
    g.events.clear();
    return IMC_OK;
}

const char *imc_last_kernels(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    static thread_local std::string copy;
    copy = g.last_kernels;
    return copy.c_str();
}

int imc_set_rank1_handoff(int on)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g.opt.rank1_handoff = on != 0;          // (part of the plan key, as every option below: cached plans of the other setting stay valid)
    return IMC_OK;
}

#ifdef IMC_Z4_TIMING
int imc_debug_z4_timing(long long *out, int n)     // diagnostics build only (see kernels_zip4.hpp)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_z4_dbg), (size_t)std::min(n, 3 * 1024 * 8) * 8) != hipSuccess) return IMC_ERR_HIP;
    return IMC_OK;
}
#endif

int imc_set_blocked_kernel(int variant)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (variant < 2 || variant > 5) return fail(IMC_ERR_ARG, "blocked kernel variant must be 2 (VALU/DPP), 3 (fp64 MFMA, LDS table), 4 (+ hybrid table, default) or 5 (hybrid wherever possible)");
    g.opt.blocked_variant = variant;
    return IMC_OK;
}

int imc_set_table_streaming(int mode)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (mode < -1 || mode > 1) return fail(IMC_ERR_ARG, "table streaming mode must be -1 (automatic), 0 (hybrid LDS cache) or 1 (streamed)");
    g.opt.z4_stream = mode;
    return IMC_OK;
}

int imc_set_wide_blocked(int mode)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (mode < -1 || mode > 1) return fail(IMC_ERR_ARG, "wide blocked mode must be -1 (automatic), 0 (never) or 1 (wherever possible)");
    g.opt.wide_blocked = mode;
    return IMC_OK;
}

int imc_last_rank1(uint64_t *checked, uint64_t *collapsed)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (checked) *checked = g.r1_checked;
    if (collapsed) *collapsed = g.r1_collapsed;
    return IMC_OK;
}

int imc_last_plan(uint64_t *out8)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!out8) return fail(IMC_ERR_ARG, "out8 is null");
    for (int k = 0; k < 8; ++k) out8[k] = g.last_plan[k];
    return IMC_OK;
}

// ---- host-side model construction (include/imcoal_model.h; no device, no context) ----
int imc_model_transitions(int n_systems, int n_intervals, const int32_t *space_size, const int32_t *cls_off,
                          const int32_t *cls_idx, const int32_t *piece_q, const int32_t *piece_proj, int n_q,
                          const int32_t *q_size, int n_proj, const int32_t *proj_off, const double *proj, const double *Q,
                          const double *dt, const double *start, double *pi, double *T, int n_threads)
{
    // (the same checks and messages as before, now shared with imc_model_transitions_device: model_check_args above,
    //  which also refuses class offsets that decrease)
    std::vector<int32_t> q_off;
    int stride = 0;
    if (int rc = model_check_args("imc_model_transitions", n_systems, n_intervals, space_size, cls_off, cls_idx, piece_q, piece_proj, n_q,
                                  q_size, n_proj, proj_off, proj, Q, dt, start, pi, T, q_off, stride))
        return rc;
    imc_model::Structure st{n_intervals, space_size, cls_off, cls_idx, piece_q, piece_proj, n_q, q_size, q_off.data(), stride, proj_off, proj};
    const size_t n = (size_t)n_intervals, s0 = (size_t)space_size[0];
    const int threads = std::max(1, std::min(std::min(n_threads, n_systems), 64));
    std::vector<std::string> errs((size_t)threads);
    auto work = [&](int t) {
        for (int b = t; b < n_systems && errs[t].empty(); b += threads)
            errs[t] = imc_model::transitions_one(st, Q + (size_t)b * stride, dt ? dt + (size_t)b * (n - 1) : nullptr, start + (size_t)b * s0,
                                                 pi + (size_t)b * n, T + (size_t)b * n * n);
    };
    if (threads == 1) work(0);
    else {
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
        work(0);
        for (std::thread &th : pool) th.join();
    }
    for (const std::string &e : errs)
        if (!e.empty()) return fail(IMC_ERR_ARG, e);
    return IMC_OK;
}

int imc_model_expm(int n, const double *A, double *out)
{
    if (n < 1 || !A || !out) return fail(IMC_ERR_ARG, "imc_model_expm: bad arguments");
    std::vector<double> work;
    if (!imc_model::expm(A, out, n, work)) return fail(IMC_ERR_ARG, "imc_model_expm: singular Pade denominator");
    return IMC_OK;
}

// ---- the same two on the device (csrc/kernels_model.hpp): host pointers in and out, synchronous, on the library's stream ----
int imc_model_transitions_device(int n_systems, int n_intervals, const int32_t *space_size, const int32_t *cls_off,
                                 const int32_t *cls_idx, const int32_t *piece_q, const int32_t *piece_proj, int n_q,
                                 const int32_t *q_size, int n_proj, const int32_t *proj_off, const double *proj, const double *Q,
                                 const double *dt, const double *start, double *pi, double *T)
{
    std::vector<int32_t> q_off;
    int stride = 0;
    if (int rc = model_check_device_args(n_systems, n_intervals, space_size, cls_off, cls_idx, piece_q, piece_proj, n_q, q_size, n_proj,
                                         proj_off, proj, Q, dt, start, pi, T, q_off, stride))
        return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    if (n_systems == 0) return IMC_OK;
    const int rc = model_transitions_device(n_systems, n_intervals, space_size, cls_off, cls_idx, piece_q, piece_proj, q_size, q_off, stride,
                                            proj_off, proj, Q, dt, start, pi, T);
    if (rc != IMC_OK) (void)hipStreamSynchronize(g.stream);   // nothing of a failed call stays in flight on the kept buffers (g_err is kept)
    return rc;
}

int imc_model_expm_batch_device(int n, int count, const double *A, double *out)
{
    if (n < 1 || count < 0 || !A || !out) return fail(IMC_ERR_ARG, "imc_model_expm_batch_device: bad arguments");
    if (n > MODEL_MAX_ORDER) return fail(IMC_ERR_ARG, "imc_model_expm_batch_device: order " + std::to_string(n) + " exceeds " + std::to_string(MODEL_MAX_ORDER));
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    if (count == 0) return IMC_OK;
    const int rc = model_expm_batch_device(n, count, A, out);
    if (rc != IMC_OK) (void)hipStreamSynchronize(g.stream);
    return rc;
}

}  // extern "C"

extern "C" {

int imc_sample_host(int N, int S, int emit_symbols, const double *pi, const double *T, const double *E, uint64_t seed, uint32_t tag,
                    int n_replicates, size_t L, void *sym_out, int sym_bytes, uint8_t *states_out)
{
    imc::SampleTables tb;
    if (int rc = sample_check("imc_sample_host", N, S, emit_symbols, pi, T, E, n_replicates, L, sym_out, sym_bytes, &tb)) return rc;
    if (sym_bytes == 1) imc::sample_sequential(tb, seed, tag, n_replicates, (uint64_t)L, (uint8_t *)sym_out, states_out);
    else imc::sample_sequential(tb, seed, tag, n_replicates, (uint64_t)L, (uint16_t *)sym_out, states_out);
    std::lock_guard<std::mutex> lk(g_mu);
    g_last_sampling[0] = 0; g_last_sampling[1] = 0; g_last_sampling[2] = 0; g_last_sampling[3] = (uint64_t)n_replicates * L;
    return IMC_OK;
}

int imc_sample_device(int N, int S, int emit_symbols, const double *pi, const double *T, const double *E, uint64_t seed, uint32_t tag,
                      int n_replicates, size_t L, void *d_sym_out, int sym_bytes, uint8_t *d_states_out, void *hip_stream)
{
    // every argument check before any HIP call
    imc::SampleTables tb;
    if (int rc = sample_check("imc_sample_device", N, S, emit_symbols, pi, T, E, n_replicates, L, d_sym_out, sym_bytes, &tb)) return rc;
    const int tile = imc::tile_setting(std::getenv("IMC_SAMPLE_TILE"), SAMPLE_TILE_DEFAULT);
    if (!tile) return fail(IMC_ERR_ARG, "imc_sample_device: IMC_SAMPLE_TILE must be a number in [1," + std::to_string(imc::kSampleMaxTile) + "]");
    const uint64_t total = (uint64_t)n_replicates * L, ntiles = imc::sample_tile_count(total, (uint64_t)tile);
    if (ntiles >= (uint64_t)1 << 31) return fail(IMC_ERR_ARG, "imc_sample_device: the stream has 2^31 tiles or more (raise IMC_SAMPLE_TILE or draw fewer columns per call)");
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = ensure_ctx()) return rc;
    HIP_TRY(hipSetDevice(g.device));
    if (int rc = check_device_output(d_sym_out, (size_t)total * sym_bytes, "d_sym_out")) return rc;
    if (d_states_out)
        if (int rc = check_device_output(d_states_out, (size_t)total, "d_states_out")) return rc;
    // NULL is the default stream, as in imc_forward_batch_device: the caller goes on to use the outputs on the stream it named
    const int rc = sample_on_device(tb, seed, tag, (uint64_t)L, total, (uint32_t)tile, (uint32_t)ntiles, d_sym_out, sym_bytes, d_states_out, (hipStream_t)hip_stream);
    if (rc != IMC_OK) {
        const std::string msg = g_err;
        (void)hipStreamSynchronize((hipStream_t)hip_stream);   // nothing of a failed call stays in flight on the freed temporaries
        return fail(rc, msg);
    }
    g_last_sampling[0] = 1; g_last_sampling[1] = ntiles; g_last_sampling[2] = (uint64_t)tile; g_last_sampling[3] = total;
    return IMC_OK;
}

int imc_last_sampling(uint64_t *out4)
{
    if (!out4) return fail(IMC_ERR_ARG, "out4 is null");
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < 4; ++i) out4[i] = g_last_sampling[i];
    return IMC_OK;
}

}  // extern "C"
