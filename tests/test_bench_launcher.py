"""bench.py must never label a one-GPU measurement as N GPUs: run without a torchrun environment, `--gpus N` starts
its own N rank processes (before anything touches the GPU); under a launcher, WORLD_SIZE must equal --gpus.  The
no-GPU rehearsal mode exercises launcher, static sharding and the gloo reduction on CPU (world 2)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
ORACLE_TOL = 1e-11


def _clean_env():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_self_launch_world2_gloo():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-cpu", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=_clean_env())
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1                                   # rank 0 only
    rec = json.loads(line[0])
    assert rec["n_gpus"] == 2 and rec["ranks"] == 2 and rec["backend"] == "gloo"
    assert rec["config"]["loglik"] == rec["config"]["loglik_expected"]


def test_world_size_mismatch_is_refused():
    env = _clean_env()
    env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--rehearse-cpu"], capture_output=True, text=True,
                         timeout=120, env=env)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)


def test_single_rank_reports_one_rank():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--rehearse-cpu"], capture_output=True, text=True,
                         timeout=120, env=_clean_env())
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert rec["n_gpus"] == 1 and rec["ranks"] == 1 and rec["backend"] is None


def test_dump_outputs_writes_what_the_timed_path_returned(tmp_path):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-cpu", "--steps", "2", "--warmup", "0",
                          "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=300,
                         env=_clean_env())
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    got = np.load(str(tmp_path / "out" / "loglik.npy"))
    assert got.dtype == np.float64 and got.tolist() == [rec["config"]["loglik"]]


def test_steps_below_one_is_refused():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--rehearse-cpu", "--steps", "0"], capture_output=True,
                         text=True, timeout=120, env=_clean_env())
    assert out.returncode != 0 and "--steps" in (out.stderr + out.stdout)


def test_multi_rank_line_carries_its_own_single_gpu_base():
    """An N > 1 line must be judgeable by itself: the ranks' shards timed alone (no collective), the efficiency against
    that base, and every rank's step time; --strong deals a FIXED number of chunks over the ranks."""
    for extra, total, scaling in (([], 8, "weak"), (["--strong", "--chunks", "6"], 6, "strong")):
        out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-cpu", "--steps", "3", "--warmup", "0"] + extra,
                             capture_output=True, text=True, timeout=300, env=_clean_env())
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
        assert rec["scaling"] == scaling and rec["config"]["chunks"] == total
        assert rec["config"]["chunks_this_rank"] == total // 2
        assert rec["config"]["loglik"] == rec["config"]["loglik_expected"]
        base = rec["single_gpu_same_workload"]
        assert base["value"] > 0 and base["ms_per_step"] > 0 and len(base["per_rank_ms_per_step"]) == 2
        assert 0 < rec["scaling_efficiency"] < 10
        per = rec["rank_ms_per_step"]
        assert len(per["per_rank"]) == 2 and per["min"] <= per["max"] and per["max"] == max(per["per_rank"])
        # rank 0's partial alone is only its own shard: chunks 0, 2, 4, ...
        assert rec["config"]["alone_partial"] == -float(sum(1000 + i for i in range(0, total, 2)))


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_its_outputs_repeat(tmp_path):
    """A plain run times the headline and nothing else (the other legs are --full's); two runs with the same arguments
    see the same inputs, so their dumped outputs are bit-identical and equal the line's loglik."""
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, env=_clean_env())
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["dtype"] == "f64"
        assert "cpu_baseline" not in rec and "extra_configs" not in rec
        dumps.append(np.load(str(d / "loglik.npy")))
        assert dumps[-1].dtype == np.float64 and dumps[-1].tolist() == [rec["config"]["loglik"]]
    assert dumps[0].tobytes() == dumps[1].tobytes()
    want = _bench_oracle()["headline"]["zip"]["total"][0]               # tests/golden/make_bench_oracle.py
    assert abs(dumps[0][0] - want) < ORACLE_TOL * abs(want), (dumps[0][0], want)


def _bench_oracle():
    with open(os.path.join(REPO, "tests", "golden", "bench_oracle.json")) as fh:
        return json.load(fh)["workloads"]


@pytest.mark.gpu
def test_variant_runs_dump_the_oracle_values(tmp_path):
    """What bench.py returns under its workload flags equals the CPU oracle on the same inputs: config[2], the
    config[3] slice, the headline with 64 proposals and the per-GPU slice of config[4] (all 64 proposal totals).
    The runs go in sequence and stop at the first failing one: nothing follows a run that went wrong on the GPU."""
    import bench_workloads as bw
    oracle = _bench_oracle()
    for name in ("config2", "config3_slice", "headline_b64", "pop150_slice"):
        w = bw.WORKLOADS[name]
        d = tmp_path / name
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--condition-ms", "0",
                              "--dump-outputs", str(d)] + list(w.flags),
                             capture_output=True, text=True, timeout=600, env=_clean_env())
        assert out.returncode == 0, (name, out.returncode, out.stderr[-2000:])
        got = np.load(str(d / "loglik.npy"))
        want = np.array(oracle[name]["zip"]["total"])
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = np.abs(got - want) / np.abs(want)
        if not err.max() < ORACLE_TOL and [bw.digest(c) for c in bw.generate(w)] != oracle[name]["sha256"]:
            pytest.fail("inputs changed: rerun make_bench_oracle.py (%s)" % name)
        assert err.max() < ORACLE_TOL, (name, int(err.argmax()), got[err.argmax()], want[err.argmax()])
        print("\n[bench oracle] bench.py %s: worst rel err %.2e over %d values" % (" ".join(w.flags), err.max(), err.size))
