// options_host.hpp - the engine's run-time options in one place: the record (imc::Options, every knob with its
// default), the table of environment variables (imc::kOptionVars: name, field, how the text becomes a value, when it is
// read) and the one comparison that says whether a cached plan may be replayed (imc::same_plan_options).  Host only, no
// HIP: planner_host.hpp derives PlanOptions from the record, engine_core.hpp keeps the live record in its context, a Plan
// keeps the one it was built under, and tests/options_host_check.cpp checks all of it on the CPU under ASan/UBSan.
// Needs no other header of the engine.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace imc {

// The knobs.  A setter of the C ABI (include/imcoal_fwd.h) or an environment variable of the table below changes one;
// nothing else does.
struct Options {
    // ---- what the planner reads (planner_host.hpp) ----
    size_t seg_override = 0;  // imc_set_segment_length: tests force stitching
    int compression = 1;      // 0 = raw symbol stream, 1 = pair-compressed token stream where possible
    int kernel_pref = 0;      // 0 = automatic, 1 = vector kernels (k_propagate / k_zpropagate), 2 = blocked (k_zpropagate2)
    bool rank1_handoff = true; // IMC_RANK1=0 switches the rank-one hand-off of the GEMM chain off (A/B measurements)
    int blocked_variant = 4;  // register-blocked kernel: 4 = fp64 MFMA 4x4x4 with the hybrid LDS/L2 table where it pays
                              // (k_zpropagate4) and the LDS table otherwise (k_zpropagate3); 3 = LDS table only;
                              // 5 = hybrid wherever it is possible (tests); 2 = k_zpropagate2 (DPP, VALU).
                              // IMC_BLOCKED=2|3|4|5 at start-up
    int wide_blocked = -1;    // 25-32 states on the blocked MFMA scan (k_zpropagate4<7 | 8>, four wavefronts per workgroup, streamed
                              // table) instead of the vector / GEMM-chain kernels: -1 = where the cost model prefers it, 0 = never,
                              // 1 = wherever every dictionary of the call has a token level the scan can run (IMC_WIDE_BLOCKED).
                              // Automatic mode only (imc_set_compression(1)): the pinned modes keep their kernels.
    int z4_stream = -1;       // k_zpropagate4's table: -1 = streamed (nothing cached in LDS) while the launch's tables are
                              // cache resident, 0 = always the hybrid LDS cache, 1 = always streamed (IMC_Z4_STREAM)
    bool table_pairs = true;  // IMC_TABLE_PAIRS=0: k_zpropagate4's table one dictionary depth per launch (A/B measurements)
    bool xcd_affine = true;   // k_zpropagate4: a parameter set's workgroups all on one XCD when B is 2, 4 or a multiple of 8 (IMC_XCD_AFFINE=0: off)
    // ---- what the plan's upload and its launches read beside those ----
    int table_triples = -1;   // three dictionary depths per table launch, one wavefront per token (k_z4_level3): -1 = up to 12 states
                              // (measured at 10 states: 106 vs 108 us and 113.5 vs 116 us per evaluation; at 20 states 54 vs 52.5 us for
                              // the table - 2197 wavefronts of 125 MFMAs in the depth 7-9 launch - so pairs stay; again with the column-split
                              // pairs: 253.3 / 256.4 vs 258.8 / 260.2 us per evaluation, profiles/table_split_sweep.txt), 0 = never, 1 = always
                              // (IMC_TABLE_TRIPLES)
    bool table_split = true;  // IMC_TABLE_SPLIT=0: every two-depth table launch in the four-tokens-per-wavefront form (A/B measurements).
                              // Otherwise a launch takes the column-split form (one token per wavefront, k_z4_level2<., ., W>) while it is
                              // latency: entries x parameter sets <= table_split_max, about one wavefront per SIMD.  Beyond that the build
                              // is throughput and the four-tokens form issues 1.6x fewer matrix instructions (at 20 states) in 4x fewer wavefronts.
    int table_split_max = -1; // -1: four per compute unit (IMC_TABLE_SPLIT_MAX)
    int fuse_tail = 1;        // the chunk's last workgroup finishes the chunk (zip3_tail) instead of k_chain launches: 1 = where a chunk is
                              // at most four workgroups (one in-wavefront fold; measured: 100 x 1e6 columns -1.5 us, and +6 us at 13
                              // workgroups of 20 states, where the chain's twenty parallel wavefronts win), 2 = wherever possible, 0 = never (IMC_FUSE_TAIL)
    bool chain_lds = false;   // IMC_CHAIN_LDS=1: k_chain's step hands its vector round through LDS, not lane to lane (A/B measurements)
    bool fuse_head = true;    // IMC_FUSE_HEAD=0: k_stage_params + k_z4_raw as launches of their own (A/B measurements)
    bool pack_table = true;   // IMC_PACK_TABLE=0: the mat-vec chain reads the padded table (A/B measurements)
    bool use_graphs = false;  // IMC_GRAPH=1: replay each plan's launch sequence as a hipGraph (measured: no gain, the
                              // per-evaluation latency is kernel time + kernel boundaries, not host launch cost)
    // ---- what no plan depends on ----
    int device_encode = -1;   // token streams of new / recompressed chunks: 0 = encoded on the host (imc::encode_levels), 1 = on the
                              // device from the symbols already there (kernels_encode.hpp; the same tokens).  -1: not set yet -
                              // IMC_DEVICE_ENCODE at start-up, else 0 (imc_set_device_encoding)
    int device_ingest = -1;   // imc_obs_create_from_text: 0 = the host parser (obs_io.hpp), 1 = the file's bytes go to the device
                              // in slabs and are parsed / unpacked there (kernels_ingest.hpp).  -1: not set yet - IMC_DEVICE_INGEST
                              // at first use, else 0 (imc_set_device_ingest)
    int device_train = -1;    // dictionary training: 0 = imc::train_dictionary on the host, 1 = on the device wherever the sample is
                              // there (kernels_train.hpp; the same dictionary).  -1: not set yet - IMC_DEVICE_TRAIN at first use,
                              // else 0 (imc_set_device_training)
    bool guard = false;       // IMC_GUARD=1: every device buffer ends flush against an unmapped guard range (dev_alloc)
};

// Whether a plan built under `a` may be replayed under `b`: every field that shapes a plan or its launches, and no other
// (the three device switches and guard mode decide how chunks and buffers are made, not what a plan holds).
inline bool same_plan_options(const Options &a, const Options &b)
{
    return a.seg_override == b.seg_override && a.compression == b.compression && a.kernel_pref == b.kernel_pref &&
           a.rank1_handoff == b.rank1_handoff && a.blocked_variant == b.blocked_variant && a.wide_blocked == b.wide_blocked &&
           a.z4_stream == b.z4_stream && a.table_pairs == b.table_pairs && a.xcd_affine == b.xcd_affine &&
           a.table_triples == b.table_triples && a.table_split == b.table_split && a.table_split_max == b.table_split_max &&
           a.fuse_tail == b.fuse_tail && a.chain_lds == b.chain_lds && a.fuse_head == b.fuse_head && a.pack_table == b.pack_table &&
           a.use_graphs == b.use_graphs;
}

// How a variable's text becomes a value (n = atoi of the text):
enum class Parse {
    Present,   // true if the variable is set at all, false if not
    NonZero,   // n != 0 (1 / 0 in an int field); unset: the field stays
    InRange,   // n if lo <= n <= hi, else ignored; unset: the field stays
    Clamp,     // n clamped to lo .. hi; unset: the field stays
    Switch,    // a device switch: consulted only while the field is -1 (the API has not set it): 1 if n == 1, else 0 - also when unset
    AtSite,    // read and parsed where it is used (named here so that this table and imcoal_fwd.h list the same set)
};
// ... and when it is read:
enum class ReadAt {
    Context,   // at every context creation, the one after imc_set_device() moved to another device included
    FirstUse,  // when the switch is first asked for (no device needed)
    Call,      // at every call that uses it: tests set these between calls of one process
    Once,      // at the first call that uses it, then kept for the process
};

struct OptionVar {
    const char *name;
    Parse parse;
    int lo, hi;                 // InRange, Clamp
    int Options::*i;            // the field it sets: an int ...
    bool Options::*b;           // ... or a bool (exactly one is set, none for AtSite)
    ReadAt when;
};

constexpr OptionVar kOptionVars[] = {
    {"IMC_GRAPH", Parse::Present, 0, 0, nullptr, &Options::use_graphs, ReadAt::Context},
    {"IMC_GUARD", Parse::NonZero, 0, 0, nullptr, &Options::guard, ReadAt::Context},
    {"IMC_BLOCKED", Parse::InRange, 2, 5, &Options::blocked_variant, nullptr, ReadAt::Context},
    {"IMC_RANK1", Parse::NonZero, 0, 0, nullptr, &Options::rank1_handoff, ReadAt::Context},
    {"IMC_PACK_TABLE", Parse::NonZero, 0, 0, nullptr, &Options::pack_table, ReadAt::Context},
    {"IMC_TABLE_PAIRS", Parse::NonZero, 0, 0, nullptr, &Options::table_pairs, ReadAt::Context},
    {"IMC_FUSE_HEAD", Parse::NonZero, 0, 0, nullptr, &Options::fuse_head, ReadAt::Context},
    {"IMC_TABLE_SPLIT", Parse::NonZero, 0, 0, nullptr, &Options::table_split, ReadAt::Context},
    {"IMC_TABLE_SPLIT_MAX", Parse::Clamp, 0, INT_MAX, &Options::table_split_max, nullptr, ReadAt::Context},
    {"IMC_TABLE_TRIPLES", Parse::NonZero, 0, 0, &Options::table_triples, nullptr, ReadAt::Context},   // (so -1 cannot be asked for)
    {"IMC_FUSE_TAIL", Parse::Clamp, 0, 2, &Options::fuse_tail, nullptr, ReadAt::Context},
    {"IMC_XCD_AFFINE", Parse::NonZero, 0, 0, nullptr, &Options::xcd_affine, ReadAt::Context},
    {"IMC_CHAIN_LDS", Parse::NonZero, 0, 0, nullptr, &Options::chain_lds, ReadAt::Context},
    {"IMC_WIDE_BLOCKED", Parse::InRange, -1, 1, &Options::wide_blocked, nullptr, ReadAt::Context},
    {"IMC_DEVICE_ENCODE", Parse::Switch, 0, 0, &Options::device_encode, nullptr, ReadAt::Context},
    {"IMC_Z4_STREAM", Parse::InRange, -1, 1, &Options::z4_stream, nullptr, ReadAt::Context},
    {"IMC_DEVICE_INGEST", Parse::Switch, 0, 0, &Options::device_ingest, nullptr, ReadAt::FirstUse},
    {"IMC_DEVICE_TRAIN", Parse::Switch, 0, 0, &Options::device_train, nullptr, ReadAt::FirstUse},
    // the planner's per-call variables (build_plan), training's (train_knobs), the slab size (ingest_slab_bytes), the
    // hand-off's diagnostics (collect_rank1_stats) and the sampler's (sample_on_device, imc_sample_device)
    {"IMC_FORCE_LEVEL", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_DEBUG", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_DEBUG_LEVELS", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_DEBUG_R1", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_DICT_MIN_COUNT", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_DICT_MAX_DEPTH", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_INGEST_SLAB_BYTES", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_SAMPLE_TILE", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_SAMPLE_LDS", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Call},
    {"IMC_DEBUG_HOST", Parse::AtSite, 0, 0, nullptr, nullptr, ReadAt::Once},
};

// Every row names its field the way its rule needs: none read at its site, a bool for Present, an int for a range, a clamp
// or a switch, exactly one of the two for NonZero.
constexpr bool option_vars_well_formed()
{
    for (const OptionVar &v : kOptionVars) {
        const bool has_int = v.i != nullptr, has_bool = v.b != nullptr;
        const bool ok = v.parse == Parse::AtSite    ? !has_int && !has_bool
                        : v.parse == Parse::Present ? !has_int && has_bool
                        : v.parse == Parse::NonZero ? has_int != has_bool
                                                    : has_int && !has_bool;
        if (!ok || (v.parse == Parse::AtSite) != (v.when == ReadAt::Call || v.when == ReadAt::Once)) return false;
    }
    return true;
}
static_assert(option_vars_well_formed(), "a row of kOptionVars names no field, both kinds of field, or the wrong kind for its rule");

// Where a variable's text comes from: the process environment in the library, a fixed list in the CPU check.
using EnvLookup = const char *(*)(const char *name);
inline const char *process_env(const char *name) { return std::getenv(name); }

// One row applied to the record (text: the variable's value, null when it is not set).
inline void apply_option(const OptionVar &v, const char *text, Options &o)
{
    if (v.parse == Parse::Switch) {
        if (o.*v.i < 0) o.*v.i = text && std::atoi(text) == 1 ? 1 : 0;
        return;
    }
    if (v.parse == Parse::Present) { o.*v.b = text != nullptr; return; }
    if (v.parse == Parse::AtSite || !text) return;
    const int n = std::atoi(text);
    if (v.parse == Parse::InRange && (n < v.lo || n > v.hi)) return;
    const int value = v.parse == Parse::NonZero ? (n != 0 ? 1 : 0) : v.parse == Parse::Clamp ? std::max(v.lo, std::min(v.hi, n)) : n;
    if (v.i) o.*v.i = value;
    else o.*v.b = value != 0;
}

// Every variable that is read at `when`, in the table's order.
inline void read_options(Options &o, ReadAt when, EnvLookup env)
{
    for (const OptionVar &v : kOptionVars)
        if (v.when == when) apply_option(v, env(v.name), o);
}

// A device switch (device_encode, device_ingest or device_train): its variable decides until the API has set it.
inline int device_switch(Options &o, int Options::*field, EnvLookup env)
{
    for (const OptionVar &v : kOptionVars)
        if (v.parse == Parse::Switch && v.i == field) apply_option(v, env(v.name), o);
    return o.*field;
}

}  // namespace imc
