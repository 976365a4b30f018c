"""What the "kernels use no scratch" tests of the CPU modules share: compile a small translation unit that includes one
kernel header for gfx950, device code only, with the compiler's kernel-resource remarks on, and read the scratch bytes per
lane of every kernel whose mangled name starts with a prefix.  The kernel lists and the assertions stay with the tests."""
import os
import re
import subprocess
import tempfile

from imcoalhmm_amd import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "imcoalhmm_amd", "csrc")


def scratch_bytes(src, prefix):
    """{mangled kernel name: ScratchSize [bytes/lane]} of the kernels of `src` (the text of a .hip file) named `prefix`..."""
    with tempfile.TemporaryDirectory() as tmp:
        tu = os.path.join(tmp, "kernels.hip")
        with open(tu, "w") as fh:
            fh.write(src)
        cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-o", os.path.join(tmp, "k.o"), tu]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and re.match(r"_Z\d+%s" % prefix, name):
            seen[name] = int(m.group(1))
    return seen
