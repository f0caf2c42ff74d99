"""`bench.py` as the driver runs it: a plain run prints the headline line only, `--steps` is the number of timed steps, and
`--dump-outputs` writes what the last timed step returned - the same arrays, bit for bit, whatever the number of steps."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


# bench.py as __main__, with every pass of the engine counted: "screen calls N" after the line
_COUNTING = """
import runpy, sys
sys.path.insert(0, sys.argv[1])
from pharmaconet_amd import engine
calls = [0]
screen = engine.screen
def counted(*a, **k):
    calls[0] += 1
    return screen(*a, **k)
engine.screen = counted
sys.argv = sys.argv[2:]
runpy.run_path(sys.argv[0], run_name="__main__")
print("screen calls", calls[0])
"""


def _bench(*argv):
    """(the JSON line, passes of the engine the run made)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, "-c", _COUNTING, str(REPO), str(REPO / "bench.py"), *argv]
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    calls = [int(ln.split()[-1]) for ln in run.stdout.splitlines() if ln.startswith("screen calls")]
    assert len(calls) == 1, run.stdout[-2000:]
    return json.loads(lines[0]), calls[0]


def test_plain_run_dumps_the_last_step_identically(tmp_path):
    args = ["--gpus", "1", "--ligands", "20000", "--warmup", "1", "--topk", "100"]
    a, calls_a = _bench(*args, "--steps", "3", "--dump-outputs", str(tmp_path / "a"))
    b, calls_b = _bench(*args, "--steps", "5", "--dump-outputs", str(tmp_path / "b"))
    # a plain run makes the warm-up passes and the timed ones, nothing else: --steps is the number of timed passes
    assert (calls_a, calls_b) == (1 + 3, 1 + 5)
    for line, steps in ((a, 3), (b, 5)):
        assert line["steps"] == steps and line["warmup"] == 1 and line["full"] is False
        assert line["unit"] == "ligand-conformers/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        n = line["config"]["ligands_per_gpu"]
        assert abs(line["value"] - n * 8 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
        # the side measurements are --full's
        assert not {"roofline", "issue", "work", "parity_sample", "cpu_baseline", "end_to_end", "survey_library"} & set(line)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["scores.npy", "status.npy", "topk_indices.npy", "topk_scores.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    out = {}
    for name in names:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
        out[name[:-4]] = x
    assert out["scores"].shape == out["status"].shape == (n,) and out["topk_scores"].shape == out["topk_indices"].shape == (100,)
    assert np.all(out["status"] == 0) and np.isfinite(out["scores"]).all()
    # the ranking the path returned is the host's ranking of the scores it returned (descending, ties by ascending index)
    order = np.lexsort((np.arange(n), -out["scores"].astype(np.float64)))[:100]
    assert out["topk_indices"].tolist() == order.tolist()
    np.testing.assert_array_equal(out["topk_scores"], out["scores"][order])
