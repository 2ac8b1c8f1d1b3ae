"""GPU: a plain `bench.py` run -- the headline alone -- and what it writes with --dump-outputs: the lnprobs of the last timed
step, equal to the reference goldens (the check a --full run makes inside bench.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path, golden):
    out = tmp_path / "outputs"
    # 1 warm-up + 2 timed steps: the last one evaluates the first proposal set, i.e. the walkers in their own order
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["metric"] == "GP lnprob evals/sec (SB2, N=6000)" and rec["unit"] == "evals/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f64" and rec["full"] is False
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["value"] > 0
    assert abs(rec["value"] * rec["ms_per_step"] * 1e-3 - 32) <= 1e-9 * 32          # 32 evaluations per timed step
    for key in ("stream_beside", "roofline", "cfg4_strong", "cpu_baseline"):
        assert key not in rec
    lnp = np.load(out / "lnprob.npy")
    table = np.load(out / "chunk_lnprob.npy")
    assert lnp.dtype == np.float64 and lnp.shape == (32,) and table.shape == (1, 32)
    assert np.array_equal(table.sum(axis=0), lnp) and lnp[0] == rec["lnprob_walker0"]
    want0 = float(golden["lnlike_vals"][list(golden["lnlike_names"]).index("cfg3_sb2_n6000")])
    want = np.asarray(golden["walkers_cfg3"], dtype=np.float64)
    assert abs(lnp[0] - want0) <= 1e-10 * max(1.0, abs(want0))
    assert np.all(np.abs(lnp[:len(want)] - want) <= 1e-10 * np.maximum(1.0, np.abs(want)))
