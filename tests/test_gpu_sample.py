"""The HMM sampler on the device (csrc/kernels_sample.hpp behind imc_sample_device, imcoalhmm_amd/simulate.py) against the
sequential specification imc_sample_host, exactly: every state-space size at which the kernels change shape (1 .. 256: packed
wavefronts, one wavefront per tile, several; LDS and global tables), lengths around the tile and the staging row, one and
three replicates, byte and 16-bit symbols, states on and off, the matrix kinds of the CPU check.  The cases are
tests/sample_gpu_cases.py; they run in child processes that import torch before the library (one HIP runtime per
process), the bulk of them in one process with IMC_SAMPLE_TILE=64 so that tens of tiles exist at small lengths."""
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = textwrap.dedent('''
    import sys
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import torch                                   # torch first: its bundled HIP runtime must be the one that initialises
    import sample_gpu_cases
    for name in sys.argv[1:]:
        getattr(sample_gpu_cases, name)(torch)
        print(name + " ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def run_cases(tmp_path, names, **env):
    script = tmp_path / "sample_cases_run.py"
    script.write_text(SCRIPT)
    environ = {k: v for k, v in os.environ.items() if k not in ("IMC_SAMPLE_TILE", "IMC_SAMPLE_LDS")}
    environ.update(env)
    return subprocess.run([sys.executable, str(script)] + list(names), capture_output=True, text=True, timeout=600, env=environ)


MAIN = ("equality", "determinism", "stream_ordering", "forwarders", "model_simulate")


@pytest.fixture(scope="module")
def main_run(tmp_path_factory):
    return run_cases(tmp_path_factory.mktemp("sample"), MAIN, IMC_SAMPLE_TILE="64")


@pytest.mark.parametrize("name", MAIN)
def test_device_sampler(main_run, name):
    """equality: imc_sample_device == imc_sample_host, symbols and states; determinism: repeated calls, tags, seeds and
    replicates; stream_ordering: output written on a side stream, host pointers refused; forwarders: simulate.forwarders
    chunks equal array-built ones at every level, log-likelihoods bit for bit; model_simulate: Model.simulate with the
    missing-data overlay at exactly the host mask chain's positions."""
    assert name + " ok" in main_run.stdout, (main_run.returncode, main_run.stdout[-1500:], main_run.stderr[-3000:])


def test_result_does_not_depend_on_the_tile_length(tmp_path):
    out = run_cases(tmp_path, ("tile_lengths",))
    assert out.returncode == 0 and "tile_lengths ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


def test_global_table_kernels(tmp_path):
    """IMC_SAMPLE_LDS=0: every table read from global memory, at every size - the variants large state spaces take."""
    out = run_cases(tmp_path, ("equality",), IMC_SAMPLE_TILE="64", IMC_SAMPLE_LDS="0")
    assert out.returncode == 0 and "equality ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


def test_sampler_under_guard_pages(tmp_path):
    """Tables, tile summaries and entering states flush against unmapped pages (IMC_GUARD=1): 20, 150 and 256 states,
    one-column replicates and L = 3 * 64 + 5."""
    out = run_cases(tmp_path, ("guard",), IMC_SAMPLE_TILE="64", IMC_GUARD="1")
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "guard ok" in out.stdout, tail
