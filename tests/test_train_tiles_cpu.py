"""Dictionary training in its parallel form (csrc/train_tiles.hpp: pair bins, the winner's associative combine, the
counting table, the sample's pieces, and train_with - the sequence of decisions the device trainer follows) under
AddressSanitizer + UBSan on the CPU: tests/train_tiles_check.cpp emulates the kernels of csrc/kernels_train.hpp tile by
tile in scrambled order at tile sizes 1, 2, 3, 4, 7 and 64 and compares every dictionary, entry for entry, with the host
trainer of csrc/pair_dict.hpp under scaled-down limits.  The program counts the branches it reached (the retry loop with
thresholds 8 and 2, the depth cap excluding the top pair, a short last round, 16384 tokens, a pair merged that exists only
across the joints of a recompression sample) and fails if one of them stayed at zero."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_train_tiles_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = tmp_path / "train_tiles_check"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            "-o", str(exe), os.path.join(HERE, "train_tiles_check.cpp")], capture_output=True, text=True, cwd=HERE)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert run.returncode == 0 and "train_tiles ok" in run.stdout, (run.stdout + run.stderr)[-2000:]
    branches = [l for l in run.stdout.splitlines() if l.startswith("branches:")]
    assert len(branches) == 1, run.stdout[-2000:]
    counts = [int(x) for x in re.findall(r" (\d+)(?:,|$)", branches[0])]
    assert len(counts) == 11 and all(c > 0 for c in counts), branches[0]
