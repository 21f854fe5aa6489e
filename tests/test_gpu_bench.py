"""GPU: `bench.py` on one GPU, plain and with --full.  Both compute the same headline outputs; the plain line leaves the legs beyond the
headline out, --full runs them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(dump_dir, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--L", "16", "--steps", "20", "--warmup", "2", "--cg-iters", "20",
           "--dump-outputs", str(dump_dir)] + list(extra)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_runs_compute_the_same_headline(tmp_path):
    plain = _bench(tmp_path / "plain")
    full = _bench(tmp_path / "full", ["--full", "--no-cpu"])
    for rec in (plain, full):
        assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["cg"]["iters_per_s"] > 0 and rec["dtype"] == "f64"
        assert sorted(rec["dump_outputs"]["arrays"]) == ["cg_solution", "hopping_f1", "hopping_f2"]
    assert plain["config"]["full"] is False and full["config"]["full"] is True
    assert plain["hermiticity_rel_dev"] is None and plain["cg"]["solve_to_1e-10"] is None and "cpu_baseline" not in plain
    assert all(plain[k] is None for k in ("gauge_recon12", "next_rows", "nocom", "cg_16"))
    assert abs(full["hermiticity_rel_dev"]) < 1e-12 and full["cg"]["solve_to_1e-10"]["cg_her"]["true_rel_res_sq"] < 1e-19
    assert full["gauge_recon12"]["value"] > 0 and full["next_rows"]["md_step_ms"] > 0 and full["roofline"]["measured_stream"]["triad_GBps"] > 0
    for name in ("hopping_f1", "hopping_f2", "cg_solution"):
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), name
