"""bench.py as a command: a plain run times its steps and prints the headline line without the sections of --full, and
--dump-outputs writes what the last timed step handed its caller, every value finite through all 32 layers (the f16 residual
stream of the synthetic model stays in range).  The headline workload itself at three steps: a few seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    steps, warmup, layers, bs, ctx = 3, 1, 32, 32, 1024
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(bs * 1e3 / line["ms_per_step"], rel=1e-9)
    assert line["step_hbm"]["frac_of_peak"] > 0
    # the sections of --full stay out of a plain run
    for key in ("roofline", "roofline_all", "value_ops_path", "prefill_kernels", "prefill_e2e", "cpu_baseline", "legs", "fp8"):
        assert key not in line, key

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["hidden_states", "k_last", "next_token_ids", "positions", "seq_lens", "v_last"]
    assert all(a.dtype == np.float32 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
    assert got["next_token_ids"].shape == (bs, ) and got["hidden_states"].shape == (bs, 4096)
    assert got["k_last"].shape == got["v_last"].shape == (layers, bs, 8 * 128)
    tok = got["next_token_ids"]
    assert np.array_equal(tok, np.round(tok)) and tok.min() >= 0 and tok.max() < 128256
    # every sequence advanced by one position per step run, the timed ones included, and the lengths with them
    assert np.all(got["positions"] == got["positions"][0]) and got["positions"][0] >= ctx - 1 + warmup + steps
    assert np.array_equal(got["seq_lens"], got["positions"] + 1)
    for name in ("hidden_states", "k_last", "v_last"):
        assert np.isfinite(got[name]).all() and np.abs(got[name]).max() > 0, name
