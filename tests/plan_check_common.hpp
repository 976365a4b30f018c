// plan_check_common.hpp - what tests/planner_host_check.cpp and tests/plan_host_check.cpp share: a stand-in kernel table
// with the shapes of the real one (same R, G, NP, slabs, flags) behind small LDS size functions ("fits", "does not
// fit", affine), dictionaries trained on sticky random streams, and chunk facts made from them by encode_levels() exactly
// as the library installs them.
#pragma once
#include "../imcoalhmm_amd/csrc/planner_host.hpp"
#include <memory>
#include <random>

using namespace imc;

// ---- stand-ins for the kernel headers' LDS size functions ----
enum Mode { AFFINE, BLOCKED_NEVER, ZIP4_NEVER, ALL_FIT, ZIP_NEVER, N_MODES };
static int g_mode = AFFINE, g_np = 4;
static long gate_hits[5][2];   // per size function: calls that fitted / did not fit
static size_t gate(int which, size_t bytes) { gate_hits[which][bytes > LDS_BUDGET]++; return bytes; }
static size_t per_token() { return (size_t)g_np * g_np * 8; }
static size_t zip_lds(int A) { return gate(0, g_mode == ALL_FIT ? 0 : g_mode == ZIP_NEVER ? LDS_BUDGET + 1 : 2048 + A * per_token()); }
static size_t blocked_bytes(int A) { return g_mode == ALL_FIT ? 0 : g_mode == BLOCKED_NEVER ? LDS_BUDGET + 1 : 1024 + A * per_token() / 2; }
static size_t zip2_lds(int A) { return gate(1, blocked_bytes(A)); }
static size_t zip3_lds(int A) { return gate(2, blocked_bytes(A)); }
static size_t zip4_bytes(int A, int hot) { return g_mode == ALL_FIT ? 0 : g_mode == ZIP4_NEVER ? LDS_BUDGET + 1 : 8192 + (size_t)A * 40 + 16 * per_token() + hot * per_token(); }
static size_t zip4_lds(int A, int hot) { return gate(3, zip4_bytes(A, hot)); }
static int zip4_max_hot(int A, size_t budget)
{
    const size_t base = zip4_bytes(A, 0);
    const int hot = g_mode == ALL_FIT ? A : base >= budget ? 0 : (int)std::min<size_t>((size_t)A, (budget - base) / per_token());
    gate_hits[4][hot < 8]++;
    return hot;
}

// ---- the kernel table's shapes (imcoal_fwd.hip: make_kc, make_big, choose_kernel) ----
static KernelFacts vec_entry(int R, int G, int MW)
{
    KernelFacts k;
    k.R = R; k.G = G; k.NP = R * G; k.VPW = 64 / G; k.minw = MW; k.zwaves = 16; k.z4_waves = 8;
    k.zip_lds = zip_lds;
    if (k.NP % 4 == 0 && k.NP <= 24) {
        k.has_zip2 = k.has_zip3 = k.has_zip4 = k.has_zip4s = k.has_level2 = true;
        k.zip2_lds = zip2_lds; k.zip3_lds = zip3_lds; k.zip4_lds = zip4_lds; k.zip4_max_hot = zip4_max_hot;
        k.tok_doubles = k.NP * k.NP;
    }
    if (k.NP == 28 || k.NP == 32) {
        k.has_zip4s = true; k.zip4_lds = zip4_lds; k.tok_doubles = k.NP * k.NP; k.z4_waves = 4; k.wide_blocked = true;
    }
    return k;
}
static KernelFacts big_entry(int NT, int NSLAB)
{
    KernelFacts k;
    k.G = NT; k.NP = 16 * NT; k.big_nslab = NSLAB; k.z4_waves = 8;
    k.big_lds = (size_t)k.NP * k.NP * 8 / NSLAB + 4096;    // (NP = 160, two slabs: one workgroup per CU, 128 slots on 256 CUs)
    return k;
}
static const std::vector<KernelFacts> kTable = {
    vec_entry(4, 1, 2), vec_entry(4, 2, 2), vec_entry(4, 3, 2), vec_entry(4, 4, 2), vec_entry(4, 5, 2), vec_entry(3, 8, 2),
    vec_entry(2, 14, 2), vec_entry(2, 16, 2), vec_entry(2, 20, 1), vec_entry(1, 48, 1), vec_entry(1, 56, 1), vec_entry(1, 64, 1),
    big_entry(6, 1), big_entry(7, 1), big_entry(8, 2), big_entry(9, 3), big_entry(10, 2), big_entry(12, 3), big_entry(14, 7), big_entry(16, 8)};
static const std::vector<KernelFacts> kMid = {big_entry(2, 1), big_entry(3, 1), big_entry(4, 1)};
static const KernelFacts *choose(int N, bool gemm)
{
    if (gemm && N > 24 && N <= 64)
        for (const KernelFacts &k : kMid) if (k.NP >= N) return &k;
    for (const KernelFacts &k : kTable) if (k.NP >= N) return &k;
    return nullptr;
}

// ---- chunk facts as obs_upload / install_encoding leave them ----
struct HostChunk {
    ChunkFacts facts;
    std::vector<uint32_t> counts[kNumLevels];
};
struct HostDict : TrainedDict {};
constexpr size_t ZIP_MIN_COLUMNS = 4096;

static std::vector<uint8_t> sticky(std::mt19937 &rng, size_t L, int S)
{
    std::vector<uint8_t> obs(L);
    uint8_t cur = 0;
    for (auto &x : obs) { if (rng() % 100 >= 96) cur = (uint8_t)(rng() % S); x = cur; }
    return obs;
}

static std::unique_ptr<HostDict> train(std::mt19937 &rng, int S)
{
    auto hd = std::make_unique<HostDict>();
    const std::vector<uint8_t> obs = sticky(rng, 2000000, S);
    train_dict(hd->dict, S, std::vector<uint8_t>(obs.begin() + 1, obs.end()), 4);
    if (hd->dict.alphabet >= kByteAlphabet) {
        const std::vector<uint8_t> b = encode_bytes(hd->dict, obs.data(), obs.size(), nullptr);
        train_dict_wide(hd->dict, std::vector<tok_t>(b.begin() + 1, b.end()), 3);
    }
    hd->depth = dict_depths(hd->dict);
    hd->order = dict_order(hd->dict, hd->depth);
    return hd;
}

static std::unique_ptr<HostChunk> make_chunk(std::mt19937 &rng, size_t L, int S, const HostDict *hd, int dict_index)
{
    auto hc = std::make_unique<HostChunk>();
    ChunkFacts &c = hc->facts;
    c.L = L; c.nsym = S;
    for (int l = 0; l < kNumLevels; ++l) c.level[l].alphabet = S;
    if (!hd || L < ZIP_MIN_COLUMNS) return hc;
    const std::vector<uint8_t> obs = sticky(rng, L, S);
    EncodedLevels enc;
    encode_levels(hd->dict, obs.data(), nullptr, L, enc);
    c.dict = dict_index;
    for (int l = 0; l < kNumLevels; ++l) {
        ChunkFacts::Level &lv = c.level[l];
        lv.alphabet = enc.alphabet[l]; lv.ntok = enc.length[l]; lv.wide = enc.is_wide[l];
        if (l > 0 && enc.alphabet[l] == enc.alphabet[l - 1]) { lv.stream = c.level[l - 1].stream; lv.wide = c.level[l - 1].wide; hc->counts[l] = hc->counts[l - 1]; continue; }
        if (enc.alphabet[l] <= S) continue;                                     // the raw stream
        lv.stream = true;
        if (!enc.is_wide[l] || enc.alphabet[l] <= HYBRID_MAX_ALPHABET) {
            hc->counts[l].assign((size_t)enc.alphabet[l], 0u);
            for (size_t t = 1; t < enc.length[l]; ++t) hc->counts[l][enc.is_wide[l] ? enc.wide[l][t] : enc.bytes[l][t]]++;
        }
    }
    for (int l = 0; l < kNumLevels; ++l) c.level[l].tok_count = &hc->counts[l];   // (the chunk is on the heap: stable)
    return hc;
}
