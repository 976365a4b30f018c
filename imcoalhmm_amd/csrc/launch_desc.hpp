// launch_desc.hpp - the plain 32-bit descriptor records that the launch plan uploads and the kernels index device memory
// through.  No HIP here: the kernel headers read them on the device, plan_host.hpp fills them on the host and
// tests/plan_host_check.cpp checks what it filled on the CPU.  (SegDesc carries a device pointer and stays in
// kernels_plain.hpp; its flag bits are here because the host cuts carry them too.)
#pragma once
#include <cstdint>

static constexpr uint32_t SEG_FIRST = 1u, SEG_WIDE = 2u;

struct VecDesc {          // one propagated vector
    uint32_t seg;         // segment id
    uint32_t c;           // basis index (0 for a first segment)
};

struct ChainDesc {
    uint32_t seg_begin, seg_end;   // input segments [begin, end) of the previous level
    uint32_t c;                    // basis index when the run does not start its chunk
    uint32_t out_vec;              // output vector index in the next level
    uint32_t first;                // 1: the run starts with its chunk's first segment (a vector)
    uint32_t chunk1;               // last level only: 1 + the chunk whose final vector this chain produces (0: none)
    uint32_t vec_first;            // first == 1: that vector's index in the previous level
    uint32_t vbase;                // first vector of the run's first operator (operator t starts at vbase + t*N); 0: no operator
};

struct Z2Block {                  // one workgroup of k_zpropagate2: up to Z2SLOTS consecutive segments of one chunk
    uint32_t seg0, n;             // first segment id, number of segments
    uint32_t out_vec0;            // where the block's combined result goes (level-0 vector index)
    uint32_t first;               // 1: seg0 is its chunk's first segment -> the result is a vector; 2 (MFMA forms): a PACKED block -
                                  // every one of the n segments is a whole chunk, slot s writes its vector to out_vec0 + s, no fold
};

struct Z2Tail { uint32_t chunk, unit, n_units, pad; };

// One workgroup of the GEMM chain (k_big_propagate: one per (segment, column slab)) or of the mat-vec chain.
struct BigBlock {
    uint32_t seg;        // segment id
    uint32_t slab;       // column slab index
    uint32_t out_vec0;   // level-0 vector index of the segment's result
    uint32_t pad;
};
