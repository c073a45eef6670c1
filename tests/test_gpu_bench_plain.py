"""bench.py without --full: the line carries the headline figures and nothing that takes runs of its own, and
--dump-outputs DIR writes the last timed step's result, checked here per group against numpy on the same generator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    from sqlrs_amd import datagen
    n_fact, n_dim = 2_000_000, 100_000
    out_dir = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "SQLRS_BENCH_SINGLE_DEVICE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
           "--rows", str(n_fact), "--dim-rows", str(n_dim), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["unit"] == "Mrows/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(n_fact / line["ms_per_step"] / 1e3, rel=0.01)
    assert line["roofline"] is None and line["cpu_baseline"] is None and not line["full"]
    for k in ("operators", "c5_variants", "ms_per_step_processes", "ms_per_step_each"):
        assert k not in line
    assert "check (per group" not in r.stderr and "profiled steps" not in r.stderr

    names = ("groups_key", "groups_count", "groups_sum", "summary")
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in names)
    a = {n: np.load(out_dir / (n + ".npy")) for n in names}
    assert all(v.dtype == np.float64 for v in a.values())

    idx = np.arange(n_fact, dtype=np.int64)
    fk, fv = datagen.key_np(0xF1, idx, n_dim), datagen.val_np(0xF2, idx)
    assert np.array_equal(np.sort(datagen.dim_key_np(np.arange(n_dim, dtype=np.int64), n_dim)), np.arange(n_dim))
    m = fv > 0.5
    cnt = np.bincount(fk[m], minlength=n_dim)
    sm = np.bincount(fk[m], weights=fv[m], minlength=n_dim)
    keys = a["groups_key"].astype(np.int64)
    assert keys.size == int((cnt > 0).sum()) == line["config"]["groups"] and np.unique(keys).size == keys.size
    assert np.array_equal(a["groups_count"], cnt[keys].astype(np.float64))
    assert np.allclose(a["groups_sum"], sm[keys], rtol=1e-9, atol=0)
    assert a["summary"][0] == keys.size and a["summary"][1] == int(m.sum()) and a["summary"][3] == keys.size
    assert a["summary"][2] == pytest.approx(float(fv[m].sum()), rel=1e-9)
