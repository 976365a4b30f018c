"""The parallel form of the HMM sampler (csrc/sample_tiles.hpp: a column as a map on the state space, tile summaries, their
associative combine, the walk from an entering state) under AddressSanitizer + UBSan on the CPU: tests/sample_tiles_check.cpp
drives the functions the sampling kernels call, tile by tile at tile lengths 1, 2, 3, 7, 64 and 4096, against the sequential
specification - six state-space sizes, replicate starts inside tiles, seven kinds of transition matrix - and checks the
Philox known answers and the threshold rules."""
from test_encode_tiles_cpu import run_check_under_asan_ubsan


def test_sample_tiles_under_asan_ubsan(tmp_path):
    run_check_under_asan_ubsan(tmp_path, "sample_tiles_check", "sample_tiles ok")
