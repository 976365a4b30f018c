"""The parallel form of an encoder pass (csrc/encode_tiles.hpp: tile summary, its associative combine, the emit rule, the
pass schedule) under AddressSanitizer + UBSan on the CPU: tests/encode_tiles_check.cpp drives the functions the device
encoder's kernels call, tile by tile at tile sizes 1, 2, 3, 4, 7 and 64, against the greedy loops of csrc/pair_dict.hpp -
single passes on every short string, concatenated marked chunks, and all 23 levels of trained dictionaries against
encode_levels().  tests/chunk_policy_check.cpp does the same for the rules behind chunk creation: how a chunk stores each
level (encode_tiles.hpp: level_rules) and the dictionary training policy (pair_dict.hpp), with scaled-down limits."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def run_check_under_asan_ubsan(tmp_path, name, says):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = tmp_path / name
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            "-o", str(exe), os.path.join(HERE, name + ".cpp")], capture_output=True, text=True, cwd=HERE)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert run.returncode == 0 and says in run.stdout, (run.stdout + run.stderr)[-2000:]


def test_encode_tiles_under_asan_ubsan(tmp_path):
    run_check_under_asan_ubsan(tmp_path, "encode_tiles_check", "encode_tiles ok")


def test_chunk_policy_under_asan_ubsan(tmp_path):
    run_check_under_asan_ubsan(tmp_path, "chunk_policy_check", "chunk_policy ok")
