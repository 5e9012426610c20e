"""bench.py's plain line and --dump-outputs: a plain run prints the headline alone, --full adds the rest, and both write the state
the last timed step computed (m_x, m_v) so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_dump_outputs_float64_and_capped_by_a_fixed_sample(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1000, 3)).astype(np.float32)
    v = rng.standard_normal((1000, 3))
    assert bench.dump_outputs(str(tmp_path / "all"), {"m_x": x, "m_v": v}) is None
    xa, va = np.load(tmp_path / "all" / "m_x.npy"), np.load(tmp_path / "all" / "m_v.npy")
    assert xa.dtype == np.float64 and va.dtype == np.float64
    assert np.array_equal(xa, x.astype(np.float64)) and np.array_equal(va, v)
    limit = 20000                                  # 48 000 bytes of rows: a sample has to be taken
    keep = bench.dump_outputs(str(tmp_path / "s1"), {"m_x": x, "m_v": v}, limit_bytes=limit)
    again = bench.dump_outputs(str(tmp_path / "s2"), {"m_x": x, "m_v": v}, limit_bytes=limit)
    assert keep is not None and np.array_equal(keep, again) and np.all(np.diff(keep) > 0)
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= limit
    assert np.array_equal(np.load(tmp_path / "s1" / "m_x.npy"), x[keep].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "s1" / "m_v.npy"), v[keep])


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stdout + r.stderr


def _bench(extra, out_dir):
    env = dict(os.environ, ADMM_BENCH_N="30")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_both_runs_dump_the_timed_state(tmp_path):
    plain = _bench([], tmp_path / "plain")
    full = _bench(["--full", "--no-cpu-baseline"], tmp_path / "full")
    for d in (plain, full):
        assert all(k in d for k in HEADLINE), d
        assert d["metric"] == "ADMM iterations/sec" and d["unit"] == "ADMM it/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] - 1e3 * d["config"]["admm_iters_per_step"] / d["ms_per_step"]) <= 1e-9 * d["value"]
    # what a plain run leaves out: statistics frames, checks, roofline, baselines
    for k in ("split_ms_per_admm_iter", "unconverged_solves_in_timed_region", "finite", "roofline", "pcie_inclusive_admm_it_per_s"):
        assert k not in plain and k in full, k
    assert full["unconverged_solves_in_timed_region"] == 0 and full["finite"]
    nv = plain["config"]["verts"]
    got = {}
    for run in ("plain", "full"):
        for name in ("m_x", "m_v"):
            a = np.load(tmp_path / run / (name + ".npy"))
            assert a.dtype == np.float64 and a.shape == (nv, 3) and np.isfinite(a).all(), (run, name, a.dtype, a.shape)
            got[run, name] = a
    assert np.abs(got["plain", "m_v"]).max() > 0          # the body moved: the dump is the stepped state, not the initial one
    # same inputs, same number of steps: the same state (the statistics frames of --full run after the dump)
    assert scenes.rel_err(got["plain", "m_x"], got["full", "m_x"]) < 1e-7
    # ... and it is the state after the LAST timed frame: the same scene and settings stepped here, 1 warm-up + 3 timed frames
    import bench
    sc, _, _ = bench.build_scene(bench.WORKLOADS["blob1m_mix"], 30)
    tol, soft = bench.workload_settings("blob1m_mix")
    s = sc.make_solver(pcg_tol=tol, pcg_max_iters=600, soft_modes=soft)
    s.upload()
    s.step_device(stats=True)
    states = []
    for _ in range(3):
        s.step_device(stats=False)
        s.download()
        states.append((s.m_x.reshape(-1, 3).copy(), s.m_v.reshape(-1, 3).copy()))
    s.close()
    assert scenes.rel_err(got["plain", "m_x"], states[2][0]) < 1e-7
    assert np.abs(got["plain", "m_v"] - states[2][1]).max() <= 1e-7 * np.abs(states[2][1]).max()
    for x_early, _ in states[:2]:                         # one or two timed frames earlier: measurably elsewhere
        assert scenes.rel_err(got["plain", "m_x"], x_early) > 1e-6
