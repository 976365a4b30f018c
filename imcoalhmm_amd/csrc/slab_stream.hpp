// slab_stream.hpp - the two pieces of host-side scaffolding the tiled device pipelines share, host-only (no HIP include):
// the loop that pumps a file through two slab buffers and carries what lies behind the cut into the next slab, and the
// split of n scan elements among the threads of a one-workgroup scan (tile_scan.hpp).  The product (imcoal_fwd.hip:
// slab_pass, the one driver of ingest_text, aln_parse_device and phy_parse_device) and the CPU checks
// (tests/ingest_tiles_check.cpp, tests/align_tiles_check.cpp, tests/phylip_tiles_check.cpp) call the same functions, so
// the checks' comparisons cover the product's loop; the rules inside its callbacks are the session records of
// ingest_tiles.hpp, align_tiles.hpp and phylip_tiles.hpp, which both call as well.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#if defined(__HIPCC__)
#define IMC_SLAB_HD __host__ __device__
#else
#define IMC_SLAB_HD
#endif

namespace imc {

// ---- the shares of a one-workgroup scan ------------------------------------------------------------------------
// Thread t of `threads` owns the elements [lo, hi) of n: ceil(n / threads) consecutive ones, in thread order; the last
// non-empty share may be short and the threads behind it own nothing.
struct ScanShare {
    uint32_t lo, hi;
};

IMC_SLAB_HD inline ScanShare scan_share(uint32_t n, uint32_t threads, uint32_t t)
{
    const uint32_t per = (n + threads - 1) / threads;
    const uint32_t lo = t * per < n ? t * per : n;
    return ScanShare{lo, lo + per < n ? lo + per : n};
}

// ---- the carried-slab loop -------------------------------------------------------------------------------------
constexpr int kSlabDone = 0;         // the whole input went through
constexpr int kSlabDeclined = 1;     // a slab cannot be cut, or a callback declines: the caller's other parser takes the input
                                     // (every other value a callback returns is its own error code and ends the loop)

// The reader of a regular file of known size, from fp's position: a short read ends the file.
struct FileSlabReader {
    FILE *fp;
    uint64_t left;
    size_t operator()(uint8_t *dst, size_t want, bool &eof)
    {
        if (want > left) want = (size_t)left;
        const size_t got = want ? std::fread(dst, 1, want, fp) : 0;
        left -= got;
        if (got < want || left == 0) eof = true;
        return got;
    }
};

// The input goes through host[0] and host[1] (`slab` bytes each; host[1] is not touched when the first read ends the
// input) alternately:
//   read(dst, want, eof)      up to `want` bytes into dst; returns how many, sets eof when the input ends with them
//   cut_of(buf, fill, last)   how many of the fill buffered bytes form the next slab (slab_cut, aln_slab_cut in the state
//                             the previous slab left); 0 declines unless the input has ended
//   queue(cur, cut)           start the work on host[cur][0 .. cut)
//   judge(cur, cut)           wait for that work and look at its verdict
// queue and judge return kSlabDone to go on, kSlabDeclined, or an error code.  The order is fixed: what lies behind the
// cut is copied into the other buffer and more input is read behind it WHILE slab k is at work (between queue and judge),
// and slab k is judged before slab k + 1 is cut and queued.  The loop itself takes no lock and makes no device call; a
// caller that holds a lock for its device calls takes it in queue and in judge.
template <class Read, class Cut, class Queue, class Judge>
int slab_stream(uint8_t *const host[2], size_t slab, Read &&read, Cut &&cut_of, Queue &&queue, Judge &&judge)
{
    bool eof = false;
    size_t fill = read(host[0], slab, eof);
    for (int cur = 0;; cur ^= 1) {
        const bool last = eof;
        const size_t cut = cut_of(host[cur], fill, last);
        if (cut == 0) return last ? kSlabDone : kSlabDeclined;
        if (const int rc = queue(cur, cut)) return rc;
        const size_t carry = fill - cut;
        if (carry) std::memcpy(host[cur ^ 1], host[cur] + cut, carry);
        fill = carry;
        if (!last) fill += read(host[cur ^ 1] + carry, slab - carry, eof);
        if (const int rc = judge(cur, cut)) return rc;
        if (last) return kSlabDone;
    }
}

}  // namespace imc
