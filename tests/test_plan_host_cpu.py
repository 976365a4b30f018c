"""Host-only launch geometry (csrc/plan_host.hpp) under AddressSanitizer + UBSan on the CPU: tests/plan_host_check.cpp
trains dictionaries on sticky random streams and checks the depth order, the two- and three-depths-per-launch table
schedules, the depth runs of the GEMM chain's table, the hot-set order, the workgroup dealing of the GEMM chain and the
XCD-affine phase table against what the kernels that run from them need.  The same program checks the geometry of a
plan, imc::plan_geometry: over states of every table family (28 and 32 with the wide scan too), 1 / 3 / 9 parameter
sets, both operator modes, the compression modes, forced segment lengths and chunk sets with an empty chunk, chunks
shorter than a segment, many one-segment chunks and one long chunk beside many short ones, it asserts what the kernels
need of the segments, stitch units, vectors, block lists, fused-tail records, stitch hierarchy and finish_fused, and
fails if its sweep never met a packed block, a fused tail, one withdrawn for packed blocks, either finish_fused, an
empty chunk, the operator mode, a hierarchy of three levels or one of the group kinds.

The planner's decisions (csrc/planner_host.hpp) the same way: tests/planner_host_check.cpp gathers chunk facts from such
dictionaries, puts small stand-ins behind the kernel table's LDS size functions and sweeps states, parameter sets, chunk
sets, compression modes, a forced segment length and the operator mode through decide_groups(), checking the grouping,
the kernel family against the gates, segment lengths, the chain's slot target, the rank-one checkpoints, forced
dictionary levels and determinism.

The options record (csrc/options_host.hpp) the same way: tests/options_host_check.cpp checks the defaults, what every
environment variable's text does to its field and when (through an injected lookup, not setenv), that a device switch
the API has set is not overridden, and which fields the plan-key comparison covers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _check_under_asan_ubsan(tmp_path, name, ok):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = tmp_path / name
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            "-o", str(exe), os.path.join(HERE, name + ".cpp")], capture_output=True, text=True, cwd=HERE)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert run.returncode == 0 and ok in run.stdout, (run.stdout + run.stderr)[-2000:]


def test_plan_host_under_asan_ubsan(tmp_path):
    _check_under_asan_ubsan(tmp_path, "plan_host_check", "plan_host ok")


def test_planner_host_under_asan_ubsan(tmp_path):
    _check_under_asan_ubsan(tmp_path, "planner_host_check", "planner_host ok")


def test_options_host_under_asan_ubsan(tmp_path):
    _check_under_asan_ubsan(tmp_path, "options_host_check", "options_host ok")
