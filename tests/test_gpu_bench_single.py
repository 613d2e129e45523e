"""The single-GPU bench line end to end: a plain `bench.py --gpus 1` run times its steps and prints the headline
record only; --dump-outputs writes the iterate the timed cycles ended on; --full adds the other measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "north_star_kernel", "fine_level_kernels", "residual_contraction_per_cycle",
             "time_to_solution", "cpu_baseline", "vcycle_algorithmic_bytes"}


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", "128", *extra], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_what_the_timed_cycles_computed(tmp_path):
    """70 steps: two graph blocks (32 + 32) and a remainder, so the warm-up runs the shortened calls (32 + 6 cycles).
    The dump must be bitwise the solver's iterate after warm-up + timed cycles from zero on the bench's seeded
    right-hand side (joined cycles are bitwise separate ones, whatever the call sizes), in the run's precision: the
    inputs are the same in every run."""
    from feanet_amd.solver import MultigridSolver
    d1 = str(tmp_path / "out")
    rec = _bench("--steps", "70", "--warmup", "3", "--dump-outputs", d1)
    assert HEADLINE <= set(rec) and not (FULL_ONLY & set(rec)), sorted(rec)
    assert rec["steps"] == 70 and rec["ms_per_step"] > 0 and rec["dtype"] == "f64" and rec["higher_is_better"] is True
    assert rec["value"] == pytest.approx(129 * 129 / (rec["ms_per_step"] * 1e-3), rel=1e-12)
    assert 3 <= rec["warmup_executed_steps"] < 6 * 70
    got = np.load(os.path.join(d1, "solution.npy"))
    assert got.dtype == np.float64 and got.shape == (1, 1, 129, 129)
    assert rec["outputs"]["solution"]["sample"] is None and rec["outputs"]["solution"]["written"] == 129 * 129
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    s = MultigridSolver(128, dtype=torch.float64)
    s.set_rhs(f=torch.randn(1, 1, 129, 129, device="cuda", dtype=torch.float64, generator=g))
    s.load()
    s.vcycle(rec["warmup_executed_steps"] + 70)
    np.testing.assert_array_equal(got, s.solution().cpu().numpy())


def test_full_run_adds_the_other_measurements(tmp_path):
    rec = _bench("--steps", "5", "--warmup", "1", "--dtype", "f32", "--full", "--kernel-reps", "2",
                 "--dump-outputs", str(tmp_path))
    assert HEADLINE <= set(rec) and FULL_ONLY <= set(rec), sorted(rec)
    assert 0 < rec["residual_contraction_per_cycle"] < 1 and rec["roofline"]["kernel"].startswith("fea_mg_")
    assert rec["cpu_baseline"]["value"] > 0
    assert np.load(os.path.join(str(tmp_path), "solution.npy")).dtype == np.float32
