// ingest_tiles_check.cpp - the parallel form of observation ingestion (csrc/ingest_tiles.hpp) against the host loops of
// csrc/obs_io.hpp, on the CPU.  The functions the ingestion kernels call are driven here sequentially, the way the device
// path runs them: the file goes through the product's own loop (imc::slab_stream of csrc/slab_stream.hpp: two buffers of
// the slab size, slab_cut, what lies behind the cut is carried into the next slab), and per slab the three launches - a
// summary per tile (folded from ingest_position) with the token-start flags, one scan over the tile summaries for output
// offsets and the slab's summary, then every tile (in reverse order here: they are independent) writes its tokens' values
// from its own offset alone.  The first slab whose verdict is not "ok" ends the file, as on the device.
//   (a) every string up to length 7 over {'0','1','7',' ','\n','x'} at nsym 3 and 20
//   (b) random longer strings: 1-3-digit tokens, leading zeros, whitespace runs of all six whitespace bytes, bad bytes,
//       tokens of 16 digits (accepted) and of 17 and more (declined)
//   at tile sizes 1, 2, 3, 4, 7, 64 x slab sizes 4, 5, 9, 64: symbols, error kind, value, column and which error comes
//   first must be TextParser's; a file may be declined only for a slab without whitespace or a digit run beyond 16.
//   (c) pairwise_symbol against encode_pairwise for all 256 x 256 byte pairs, unpack2 against the cache reader's
//       expression, the slab size setting.
// Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../imcoalhmm_amd/csrc/ingest_tiles.hpp"
#include "../imcoalhmm_amd/csrc/obs_io.hpp"
#include "../imcoalhmm_amd/csrc/slab_stream.hpp"

static long g_compared = 0, g_declined = 0;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 1) {}
    uint32_t next()
    {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        return (uint32_t)(s >> 16);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

struct Parsed {
    int code = 0;                    // 0, -2, -5 (IoResult), or 1: declined
    std::string msg;
    std::vector<uint16_t> sym;
};

static const char *kPath = "f";

static void host_parse(const std::vector<uint8_t> &data, int nsym, Parsed &out)
{
    out.sym.clear();
    imc::TextParser<uint16_t> p;
    imc::IoResult r = p.feed(reinterpret_cast<const char *>(data.data()), data.size(), nsym, kPath, out.sym);
    if (!r.code) r = p.finish(nsym, out.sym);
    out.code = r.code;
    out.msg = r.msg;
}

// scratch of tiled_parse, kept between calls
static std::vector<uint8_t> t_buf[2], t_flag;
static std::vector<imc::IngestSummary> t_sums;
static std::vector<uint32_t> t_off;

// The product's loop (imc::slab_stream) over two buffers of the slab size, with the three launches as its "queue" and the
// product's rules (imc::TextSession: cut, accept) as its cut and its "judge".
static void tiled_parse(const std::vector<uint8_t> &data, size_t slab, size_t tile, uint32_t nsym, Parsed &out)
{
    out.code = 0;
    out.msg.clear();
    out.sym.clear();
    for (auto &b : t_buf) b.assign(slab, 0);
    uint8_t *const host[2] = {t_buf[0].data(), t_buf[1].data()};
    size_t pos = 0;
    imc::TextSession ses(data.size());                         // the product's rules, with the arguments the engine passes
    const uint64_t &cols = ses.cols;
    imc::IngestSummary all = imc::ingest_identity();
    out.code = imc::slab_stream(
        host, slab,
        [&](uint8_t *dst, size_t want, bool &eof) {
            const size_t take = std::min(want, data.size() - pos);
            if (take) std::memcpy(dst, data.data() + pos, take);
            pos += take;
            if (pos == data.size()) eof = true;
            return take;
        },
        [&](const uint8_t *buf, size_t fill, bool last) { return ses.cut(buf, fill, last); },           // 0 before the end: a slab without whitespace
        [&](int cur, size_t cut) -> int {
            const uint32_t n = (uint32_t)cut;
            const uint8_t *b = host[cur];
            const size_t ntiles = (n + tile - 1) / tile;
            // launch 1: flags and tile summaries
            t_flag.assign(n, 0);
            t_sums.assign(ntiles, imc::ingest_identity());
            for (size_t k = 0; k < ntiles; ++k) {
                imc::IngestSummary s = imc::ingest_identity();
                for (uint32_t i = (uint32_t)(k * tile); i < std::min<size_t>(n, (k + 1) * tile); ++i) {
                    const uint8_t prev = i ? b[i - 1] : (uint8_t)' ';
                    t_flag[i] = imc::token_start(prev, b[i]);
                    s = imc::ingest_combine(s, imc::ingest_position(b + i, prev, i, n, nsym));
                }
                t_sums[k] = s;
            }
            // launch 2: offsets and the slab's summary
            t_off.assign(ntiles, 0);
            all = imc::ingest_identity();
            for (size_t k = 0; k < ntiles; ++k) {
                t_off[k] = all.count;
                all = imc::ingest_combine(all, t_sums[k]);
            }
            CHECK(cols + all.count <= imc::max_tokens_in(data.size()));
            // launch 3: every tile writes its tokens from its own offset (whatever the verdict will be, as on the device)
            out.sym.resize(cols + all.count, 0xffff);
            for (size_t k = ntiles; k-- > 0;) {
                uint32_t w = t_off[k];
                for (uint32_t i = (uint32_t)(k * tile); i < std::min<size_t>(n, (k + 1) * tile); ++i)
                    if (t_flag[i]) out.sym[cols + w++] = (uint16_t)imc::token_read(b + i, n - i).value;
                CHECK(w == t_off[k] + t_sums[k].count);
            }
            return 0;
        },
        [&](int, size_t cut) -> int {
            const imc::IoResult r = ses.accept(all, cut, kPath);
            out.msg = r.msg;
            return r.code;
        });
}

static size_t longest_digit_run(const std::vector<uint8_t> &d)
{
    size_t best = 0, run = 0;
    for (uint8_t c : d) {
        run = imc::byte_class(c) == imc::kByteDigit ? run + 1 : 0;
        best = std::max(best, run);
    }
    return best;
}

static size_t longest_run_without_space(const std::vector<uint8_t> &d)
{
    size_t best = 0, run = 0;
    for (uint8_t c : d) {
        run = imc::byte_class(c) != imc::kByteSpace ? run + 1 : 0;
        best = std::max(best, run);
    }
    return best;
}

static const size_t kTiles[] = {1, 2, 3, 4, 7, 64};
static const size_t kSlabs[] = {4, 5, 9, 64};

static void compare_all(const std::vector<uint8_t> &data, int nsym)
{
    static Parsed want, got;
    host_parse(data, nsym, want);
    const size_t digits = longest_digit_run(data), solid = longest_run_without_space(data);
    for (size_t slab : kSlabs)
        for (size_t tile : kTiles) {
            tiled_parse(data, slab, tile, (uint32_t)nsym, got);
            ++g_compared;
            if (got.code == 1) {
                CHECK(digits > imc::kMaxTokenDigits || solid >= slab);
                ++g_declined;
                continue;
            }
            CHECK(digits <= imc::kMaxTokenDigits || want.code != 0);      // an accepted file holds no longer run before its first error
            CHECK(got.code == want.code);
            CHECK(got.msg == want.msg);
            if (want.code == 0) CHECK(got.sym == want.sym);
        }
}

static void exhaustive()
{
    const char alphabet[6] = {'0', '1', '7', ' ', '\n', 'x'};
    std::vector<uint8_t> s;
    for (int len = 0; len <= 7; ++len) {
        long total = 1;
        for (int i = 0; i < len; ++i) total *= 6;
        s.resize(len);
        for (long code = 0; code < total; ++code) {
            long c = code;
            for (int i = 0; i < len; ++i) { s[i] = (uint8_t)alphabet[c % 6]; c /= 6; }
            compare_all(s, 3);
            compare_all(s, 20);
        }
    }
}

static void random_strings()
{
    const char ws[6] = {' ', '\n', '\t', '\r', '\f', '\v'};
    const int nsyms[] = {3, 20, 257, 1000};
    Rng rng(7);
    for (int round = 0; round < 4000; ++round) {
        const int nsym = nsyms[rng.below(4)];
        const uint32_t tokens = 1 + rng.below(60);
        const uint32_t p_bad = rng.below(3) == 0 ? 40 : 0, p_big = rng.below(3) == 0 ? 30 : 0, p_long = rng.below(4) == 0 ? 25 : 0;
        std::vector<uint8_t> s;
        if (rng.below(2)) for (uint32_t k = rng.below(4); k > 0; --k) s.push_back((uint8_t)ws[rng.below(6)]);   // leading whitespace
        for (uint32_t t = 0; t < tokens; ++t) {
            if (p_long && rng.below(p_long) == 0) {                       // 15 to 20 digits, leading zeros or not
                const uint32_t len = 15 + rng.below(6);
                const bool zeros = rng.below(2);
                for (uint32_t j = 0; j < len; ++j) s.push_back((uint8_t)('0' + (zeros && j + 1 < len ? 0 : rng.below(10))));
            } else {
                uint32_t v = rng.below((uint32_t)std::min(nsym, 1000));
                if (p_big && rng.below(p_big) == 0) v = (uint32_t)nsym + rng.below(3);
                char text[16];
                if (rng.below(5) == 0) std::snprintf(text, sizeof text, "%03u", v);   // leading zeros
                else std::snprintf(text, sizeof text, "%u", v);
                for (const char *q = text; *q; ++q) s.push_back((uint8_t)*q);
            }
            if (p_bad && rng.below(p_bad) == 0) s.push_back((uint8_t)"x-+.A\x80"[rng.below(6)]);
            if (t + 1 < tokens || rng.below(2))
                for (uint32_t k = 1 + (rng.below(4) == 0 ? rng.below(12) : 0); k > 0; --k) s.push_back((uint8_t)ws[rng.below(6)]);
        }
        compare_all(s, nsym);
    }
    // the cap: every value beyond 1000000 reads as 1000000, at the end of the file and before whitespace
    for (const char *text : {"1000001", "99999999 ", "0 1234567890123456", "0 1234567890123456 1", "007", "0000000000000002", "00000000000000002"}) {
        std::vector<uint8_t> s(text, text + std::strlen(text));
        compare_all(s, 3);
        compare_all(s, 1000);
    }
}

static void other_rules()
{
    std::vector<char> a(65536), b(65536);
    std::vector<uint8_t> want(65536);
    for (int x = 0; x < 256; ++x)
        for (int y = 0; y < 256; ++y) { a[x * 256 + y] = (char)x; b[x * 256 + y] = (char)y; }
    imc::encode_pairwise(a.data(), b.data(), 65536, want.data());
    for (int i = 0; i < 65536; ++i) CHECK(imc::pairwise_symbol((uint8_t)a[i], (uint8_t)b[i]) == want[i]);
    Rng rng(11);
    std::vector<uint8_t> pk(64);
    for (auto &v : pk) v = (uint8_t)rng.below(256);
    for (uint32_t t = 0; t < 256; ++t) CHECK(imc::unpack2(pk.data(), t) == ((pk[t >> 2] >> (2 * (t & 3))) & 3u));
    CHECK(imc::slab_bytes_setting(nullptr, 1 << 20) == (1u << 20));
    CHECK(imc::slab_bytes_setting("", 1 << 20) == (1u << 20));
    CHECK(imc::slab_bytes_setting("junk", 1 << 20) == (1u << 20));
    CHECK(imc::slab_bytes_setting("1", 1 << 20) == imc::kMinSlabBytes);
    CHECK(imc::slab_bytes_setting("4097", 1 << 20) == 4097);
    CHECK(imc::slab_bytes_setting("99999999999999", 1 << 20) == imc::kMaxSlabBytes);
    CHECK(imc::max_tokens_in(0) == 0 && imc::max_tokens_in(1) == 1 && imc::max_tokens_in(2) == 1 && imc::max_tokens_in(3) == 2);
    // the room rule: "1 1 1" and "0 0 0 0" (both among the exhaustive strings, taken at every slab and tile size) hold exactly
    // max_tokens_in(file bytes) tokens; no file holds more, so the error behind the bound is asked for directly
    for (uint32_t tokens : {3u, 4u}) {
        imc::TextSession ses(2 * tokens - 1);
        imc::IngestSummary s = imc::ingest_identity();
        s.count = tokens - 1;
        CHECK(ses.room == tokens && ses.accept(s, 2 * tokens - 2, kPath).code == 0 && ses.cols == tokens - 1);
        s.count = 1;
        CHECK(ses.accept(s, 1, kPath).code == 0 && ses.cols == ses.room);                   // exactly the room: taken
        const imc::IoResult over = ses.accept(s, 1, kPath);                                 // one more: the engine's error
        CHECK(over.code == imc::kRuleHip && over.msg == "ingest: more tokens than the file can hold");
    }
}

int main()
{
    exhaustive();
    random_strings();
    other_rules();
    CHECK(g_declined > 0 && g_declined < g_compared / 2);
    std::printf("ingest_tiles ok: %ld comparisons, %ld declined\n", g_compared, g_declined);
    return 0;
}
