"""Compile-time check of the 25-32 state blocked kernels (no GPU needed: hipcc cross-compiles): the library holds the
streamed scan and the two table kernels for seven and eight tiles, none of them uses scratch memory, and each fits the
512 registers (VGPRs + AGPRs) a lane has with one wavefront per SIMD."""
import os
import re
import subprocess
import tempfile

from imcoalhmm_amd import build

# mangled names: <length><identifier>I...Li<NT>E
WANTED = {
    "k_zpropagate4 (bytes)": "13k_zpropagate4ILi%dELb0ELb0EE",
    "k_zpropagate4 (16-bit)": "13k_zpropagate4ILi%dELb1ELb0EE",
    "k_z4_raw": "8k_z4_rawILi%dEE",
    "k_z4_level": "10k_z4_levelILi%dEE",
}


def test_wide_blocked_kernels_fit_the_register_file():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "k.o"), build.SRC]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split()[0]] = int(m.group(2))
    for nt in (7, 8):
        for what, pattern in WANTED.items():
            hits = [k for k in usage if pattern % nt in k]
            assert len(hits) == 1, (what, nt, hits)
            u = usage[hits[0]]
            print(hits[0], u)
            assert u["ScratchSize"] == 0, (hits[0], u)
            assert u["VGPRs"] + u["AGPRs"] <= 512, (hits[0], u)
    # of the blocked family only these exist from seven tiles on: no hybrid scan, no LDS-table kernel, no multi-depth table build
    extra = [k for k in usage if re.search(r"Li[78]E", k) and any(
        h in k for h in ("13k_zpropagate4", "13k_zpropagate3", "13k_zpropagate2", "11k_z4_level2", "11k_z4_level3", "10k_z4_level", "8k_z4_raw"))
        and not any(p % nt in k for p in WANTED.values() for nt in (7, 8))]
    assert not extra, extra
