"""GPU: a plain `bench.py` run (no --full) is the headline alone -- W warm-up and K timed steps of convert, one line --
and with --dump-outputs writes the same files as a --full run, holding what the --full run computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--frames", "50000", "--steps", "3", "--warmup", "1"]
DUMPED = ["convert_broad_y.npy", "convert_fixture_y.npy", "convert_y.npy", "dtw_paths.npy", "estep_fixture_stats.npy",
          "estep_stats.npy", "traj_y.npy"]


def _bench(args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    plain = _bench(SMALL)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["roofline"]["kernel_ms"] > 0
    for k in ("summary", "cpu_baseline", "parity_max_rel_err_vs_oracle", "steady", "host_inclusive", "detail"):
        assert k not in plain, k


def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _bench(SMALL + ["--dump-outputs", str(tmp_path / "plain")])
    for k in ("cpu_baseline", "parity_max_rel_err_vs_oracle", "steady", "host_inclusive", "detail"):
        assert k not in plain, k
    full = _bench(SMALL + ["--full", "--cpu-seconds", "0.5", "--cpu-seconds-sub", "0.5", "--pmc", "off",
                           "--dump-outputs", str(tmp_path / "full")])
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert full[k] == plain[k], k
    assert full["parity_max_rel_err_vs_oracle"] < 1e-9 and full["cpu_baseline"]["value"] > 0 and full["steady"] and full["detail"]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "full")) == DUMPED
    for f in DUMPED:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-12, atol=0.0), f
