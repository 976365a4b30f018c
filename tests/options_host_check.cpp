// options_host_check.cpp - CPU check of csrc/options_host.hpp (built with g++ -fsanitize=address,undefined by
// tests/test_plan_host_cpu.py): the record's defaults, what every environment variable's text does to its field and when,
// that a device switch the API has set is left alone, and which fields the plan-key comparison covers.  The environment
// is an injected lookup over one (name, text) pair; every expectation below is written out, none is computed by the code
// under test, and each row names its field by its place in flatten(), not through the table's member pointer.
#include <cstdio>
#include <cstring>

#include "../imcoalhmm_amd/csrc/options_host.hpp"

using imc::Options;

static int g_failures = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                     \
            std::fprintf(stderr, __VA_ARGS__);                                            \
            std::fprintf(stderr, "\n");                                                   \
            ++g_failures;                                                                 \
        }                                                                                 \
    } while (0)

// ---- the injected environment: one variable, set or not ----
static const char *g_name = nullptr, *g_text = nullptr;
static const char *one_variable(const char *name) { return g_name && std::strcmp(name, g_name) == 0 ? g_text : nullptr; }

static const char *const kTexts[8] = {nullptr, "", "0", "1", "2", "-1", "7", "abc"};
static const char *shown(const char *t) { return t ? t : "(unset)"; }

// Every field of the record as one line of numbers: "nothing else moved" is a comparison of two of these.
static void flatten(const Options &o, long long out[21])
{
    const long long v[21] = {(long long)o.seg_override, o.compression, o.kernel_pref, o.rank1_handoff, o.blocked_variant, o.wide_blocked, o.z4_stream,
                             o.table_pairs, o.xcd_affine, o.table_triples, o.table_split, o.table_split_max, o.fuse_tail, o.chain_lds, o.fuse_head,
                             o.pack_table, o.use_graphs, o.device_encode, o.device_ingest, o.device_train, o.guard};
    std::memcpy(out, v, sizeof v);
}

struct Expect {
    const char *name;
    int slot;                     // index of the variable's field in flatten(), -1: the variable is read where it is used
    imc::ReadAt when;
    long long value[8];           // the field after the texts of kTexts, from a default record
};

// (transcribed from the engine before the table existed: IMC_GRAPH is "set at all"; the A/B switches atoi != 0; IMC_BLOCKED
// taken within 2..5 and IMC_WIDE_BLOCKED / IMC_Z4_STREAM within -1..1, else ignored; IMC_FUSE_TAIL clamped to 0..2;
// IMC_TABLE_SPLIT_MAX max(0, atoi); IMC_TABLE_TRIPLES atoi != 0 ? 1 : 0; the device switches 1 only for atoi == 1, else 0)
static const Expect kExpect[] = {
    //                                                          unset  ""  "0"  "1"  "2" "-1"  "7" "abc"
    {"IMC_GRAPH", 16, imc::ReadAt::Context,                    {0,     1,   1,   1,   1,   1,   1,   1}},
    {"IMC_GUARD", 20, imc::ReadAt::Context,                    {0,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_BLOCKED", 4, imc::ReadAt::Context,                   {4,     4,   4,   4,   2,   4,   4,   4}},
    {"IMC_RANK1", 3, imc::ReadAt::Context,                     {1,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_PACK_TABLE", 15, imc::ReadAt::Context,               {1,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_TABLE_PAIRS", 7, imc::ReadAt::Context,               {1,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_FUSE_HEAD", 14, imc::ReadAt::Context,                {1,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_TABLE_SPLIT", 10, imc::ReadAt::Context,              {1,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_TABLE_SPLIT_MAX", 11, imc::ReadAt::Context,          {-1,    0,   0,   1,   2,   0,   7,   0}},
    {"IMC_TABLE_TRIPLES", 9, imc::ReadAt::Context,             {-1,    0,   0,   1,   1,   1,   1,   0}},
    {"IMC_FUSE_TAIL", 12, imc::ReadAt::Context,                {1,     0,   0,   1,   2,   0,   2,   0}},
    {"IMC_XCD_AFFINE", 8, imc::ReadAt::Context,                {1,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_CHAIN_LDS", 13, imc::ReadAt::Context,                {0,     0,   0,   1,   1,   1,   1,   0}},
    {"IMC_WIDE_BLOCKED", 5, imc::ReadAt::Context,              {-1,    0,   0,   1,  -1,  -1,  -1,   0}},
    {"IMC_DEVICE_ENCODE", 17, imc::ReadAt::Context,            {0,     0,   0,   1,   0,   0,   0,   0}},
    {"IMC_Z4_STREAM", 6, imc::ReadAt::Context,                 {-1,    0,   0,   1,  -1,  -1,  -1,   0}},
    {"IMC_DEVICE_INGEST", 18, imc::ReadAt::FirstUse,           {0,     0,   0,   1,   0,   0,   0,   0}},
    {"IMC_DEVICE_TRAIN", 19, imc::ReadAt::FirstUse,            {0,     0,   0,   1,   0,   0,   0,   0}},
    {"IMC_FORCE_LEVEL", -1, imc::ReadAt::Call, {}},
    {"IMC_DEBUG", -1, imc::ReadAt::Call, {}},
    {"IMC_DEBUG_LEVELS", -1, imc::ReadAt::Call, {}},
    {"IMC_DEBUG_R1", -1, imc::ReadAt::Call, {}},
    {"IMC_DICT_MIN_COUNT", -1, imc::ReadAt::Call, {}},
    {"IMC_DICT_MAX_DEPTH", -1, imc::ReadAt::Call, {}},
    {"IMC_INGEST_SLAB_BYTES", -1, imc::ReadAt::Call, {}},
    {"IMC_SAMPLE_TILE", -1, imc::ReadAt::Call, {}},
    {"IMC_SAMPLE_LDS", -1, imc::ReadAt::Call, {}},
    {"IMC_DEBUG_HOST", -1, imc::ReadAt::Once, {}},
};
constexpr int kRows = sizeof(kExpect) / sizeof(kExpect[0]);

static void check_defaults()
{
    const Options o;
    CHECK(o.seg_override == 0 && o.compression == 1 && o.kernel_pref == 0 && o.rank1_handoff == true && o.blocked_variant == 4 && o.wide_blocked == -1 &&
              o.z4_stream == -1 && o.table_pairs == true && o.table_triples == -1 && o.table_split == true && o.table_split_max == -1 &&
              o.xcd_affine == true && o.fuse_tail == 1 && o.chain_lds == false && o.fuse_head == true && o.pack_table == true &&
              o.device_encode == -1 && o.device_ingest == -1 && o.device_train == -1 && o.guard == false && o.use_graphs == false,
          "a default differs from the engine's");
}

// How the engine asks: every Context variable at context creation, a FirstUse switch through device_switch.
static void read_as_the_engine(Options &o, const Expect &e)
{
    imc::read_options(o, imc::ReadAt::Context, one_variable);
    if (e.slot == 18) (void)imc::device_switch(o, &Options::device_ingest, one_variable);
    if (e.slot == 19) (void)imc::device_switch(o, &Options::device_train, one_variable);
}

static void check_table()
{
    const int n_vars = (int)(sizeof(imc::kOptionVars) / sizeof(imc::kOptionVars[0]));
    CHECK(n_vars == kRows, "the table has %d rows, the check expects %d", n_vars, kRows);
    for (int r = 0; r < kRows && r < n_vars; ++r) {
        const Expect &e = kExpect[r];
        CHECK(std::strcmp(imc::kOptionVars[r].name, e.name) == 0, "row %d is %s, expected %s", r, imc::kOptionVars[r].name, e.name);
        CHECK(imc::kOptionVars[r].when == e.when, "%s is read at another moment", e.name);
        CHECK((imc::kOptionVars[r].parse == imc::Parse::AtSite) == (e.slot < 0), "%s: read at its site or not", e.name);
        for (int t = 0; t < 8; ++t) {
            g_name = e.name;
            g_text = kTexts[t];
            Options o;
            read_as_the_engine(o, e);
            // a default record read with nothing set: the baseline every other field must keep (device_encode becomes 0)
            g_name = nullptr;
            Options base;
            read_as_the_engine(base, e);
            long long got[21], want[21];
            flatten(o, got);
            flatten(base, want);
            if (e.slot >= 0) want[e.slot] = e.value[t];
            for (int k = 0; k < 21; ++k)
                CHECK(got[k] == want[k], "%s=%s: field %d is %lld, expected %lld", e.name, shown(kTexts[t]), k, got[k], want[k]);
        }
    }
    // the variables of the first-use switches are not read at context creation
    g_name = "IMC_DEVICE_INGEST"; g_text = "1";
    Options o;
    imc::read_options(o, imc::ReadAt::Context, one_variable);
    CHECK(o.device_ingest == -1, "IMC_DEVICE_INGEST was read at context creation");
    g_name = "IMC_DEVICE_TRAIN";
    imc::read_options(o, imc::ReadAt::Context, one_variable);
    CHECK(o.device_train == -1, "IMC_DEVICE_TRAIN was read at context creation");
    CHECK(o.device_encode == 0, "IMC_DEVICE_ENCODE unset must leave the host encoder");
}

static void check_switches_set_by_the_api()
{
    int Options::*const fields[3] = {&Options::device_encode, &Options::device_ingest, &Options::device_train};
    const char *const names[3] = {"IMC_DEVICE_ENCODE", "IMC_DEVICE_INGEST", "IMC_DEVICE_TRAIN"};
    for (int k = 0; k < 3; ++k)
        for (int api = 0; api <= 1; ++api) {
            g_name = names[k];
            g_text = api ? "0" : "1";                    // the variable asks for the other setting
            Options o;
            o.*fields[k] = api;
            imc::read_options(o, imc::ReadAt::Context, one_variable);
            CHECK(o.*fields[k] == api, "%s overrode the API at context creation", names[k]);
            CHECK(imc::device_switch(o, fields[k], one_variable) == api && o.*fields[k] == api, "%s overrode the API at first use", names[k]);
            imc::read_options(o, imc::ReadAt::Context, one_variable);     // (a second context creation, after imc_set_device)
            CHECK(o.*fields[k] == api, "%s overrode the API at the second context creation", names[k]);
        }
    // ... and once the variable has decided, a later change of the variable does not either
    g_name = "IMC_DEVICE_TRAIN"; g_text = "1";
    Options o;
    CHECK(imc::device_switch(o, &Options::device_train, one_variable) == 1, "IMC_DEVICE_TRAIN=1 at first use");
    g_text = "0";
    CHECK(imc::device_switch(o, &Options::device_train, one_variable) == 1, "the switch was read a second time");
}

static void check_comparison()
{
    struct Change { const char *field; void (*apply)(Options &); bool covered; };
    const Change changes[] = {
        {"seg_override", [](Options &o) { o.seg_override = 48; }, true},
        {"compression", [](Options &o) { o.compression = 0; }, true},
        {"kernel_pref", [](Options &o) { o.kernel_pref = 2; }, true},
        {"rank1_handoff", [](Options &o) { o.rank1_handoff = false; }, true},
        {"blocked_variant", [](Options &o) { o.blocked_variant = 3; }, true},
        {"wide_blocked", [](Options &o) { o.wide_blocked = 1; }, true},
        {"z4_stream", [](Options &o) { o.z4_stream = 0; }, true},
        {"table_pairs", [](Options &o) { o.table_pairs = false; }, true},
        {"xcd_affine", [](Options &o) { o.xcd_affine = false; }, true},
        {"table_triples", [](Options &o) { o.table_triples = 1; }, true},
        {"table_split", [](Options &o) { o.table_split = false; }, true},
        {"table_split_max", [](Options &o) { o.table_split_max = 0; }, true},
        {"fuse_tail", [](Options &o) { o.fuse_tail = 2; }, true},
        {"chain_lds", [](Options &o) { o.chain_lds = true; }, true},
        {"fuse_head", [](Options &o) { o.fuse_head = false; }, true},
        {"pack_table", [](Options &o) { o.pack_table = false; }, true},
        {"use_graphs", [](Options &o) { o.use_graphs = true; }, true},
        {"device_encode", [](Options &o) { o.device_encode = 1; }, false},
        {"device_ingest", [](Options &o) { o.device_ingest = 1; }, false},
        {"device_train", [](Options &o) { o.device_train = 1; }, false},
        {"guard", [](Options &o) { o.guard = true; }, false},
    };
    const Options a;
    CHECK(imc::same_plan_options(a, a), "a record differs from itself");
    for (const Change &c : changes) {
        Options b;
        long long before[21], after[21];
        flatten(b, before);
        c.apply(b);
        flatten(b, after);
        int moved = 0;
        for (int k = 0; k < 21; ++k) moved += before[k] != after[k];
        CHECK(moved == 1, "%s: the change moved %d fields", c.field, moved);
        CHECK(imc::same_plan_options(a, b) == !c.covered && imc::same_plan_options(b, a) == !c.covered, "%s: %s by the comparison", c.field,
              c.covered ? "not seen" : "seen");
    }
    CHECK(sizeof(changes) / sizeof(changes[0]) == 21, "a field of the record has no change here");
}

int main()
{
    check_defaults();
    check_table();
    check_switches_set_by_the_api();
    check_comparison();
    if (g_failures) {
        std::fprintf(stderr, "%d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("options_host ok\n");
    return 0;
}
