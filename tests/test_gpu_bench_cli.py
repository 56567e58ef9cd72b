"""bench.py's command line on the GPU: a plain run (`--gpus 1 --steps K
--warmup W`) times its steps and prints the result line with the side legs
left out; `--dump-outputs DIR` writes the last timed step's records; `--full`
brings the side legs back.  One plain and one `--full` run of the same small
corpus (64 MiB, 4 blocks) in fresh processes: the `--full` run's parity leg
checks its records against the oracle order-exactly, and the plain run's dump
must equal the `--full` run's file for file (same arguments, same inputs, same
outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 5
NAMES = ("match_end", "match_order", "match_id", "step_counts", "sample_index")


def _bench(out_dir, *extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
              "VSA_BENCH_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
           "--warmup", "2", "--gib", "0.0625", "--blocks", "4", "--no-settle",
           "--dump-outputs", str(out_dir), *extra]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_gpu_bench_plain_and_full(tmp_path):
    plain = _bench(tmp_path / "plain")
    full = _bench(tmp_path / "full", "--full", "--no-cpu", "--no-e2e", "--no-cfg5")

    # the plain line: the headline fields, none of the side legs
    assert plain["full"] is False and full["full"] is True
    assert plain["steps"] == STEPS and plain["matches"] > 0
    assert plain["unit"] == "GB/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "u8"
    assert plain["ms_per_step"] > 0
    # value is the corpus over one step's time, in GB/s
    assert plain["value"] == pytest.approx((64 << 20) / (plain["ms_per_step"] * 1e-3) / 1e9,
                                           rel=1e-3)
    assert plain["parity"] is None and plain["parity_bytes"] == 0
    assert plain["cpu_baseline"] is None
    assert plain["end_to_end"] is None and plain["end_to_end_cfg5proxy"] is None
    assert plain["roofline"]["peak_measured"] is None
    assert plain["roofline"]["kernel_ms"] > 0

    # the --full line: parity over the whole corpus and the read ceiling
    assert full["parity"] is True and full["parity_bytes"] == 64 << 20
    assert full["roofline"]["peak_measured"] > 0
    assert full["matches"] == plain["matches"]

    # the dumps: float64, consistent with the line, equal between the runs
    total = 0
    for name in NAMES:
        a = np.load(tmp_path / "plain" / (name + ".npy"))
        b = np.load(tmp_path / "full" / (name + ".npy"))
        assert a.dtype == np.float64 and a.ndim == 1
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64_000_000
    d = {n: np.load(tmp_path / "plain" / (n + ".npy")) for n in NAMES}
    nm = plain["matches"]
    assert d["step_counts"].tolist() == [nm] * STEPS
    assert len(d["match_end"]) == len(d["match_id"]) == len(d["match_order"]) == nm
    assert np.array_equal(d["sample_index"], np.arange(nm))
    # records come in end order, inside the corpus, ids of the 5,000 literals
    assert np.all(np.diff(d["match_end"]) >= 0)
    assert d["match_end"][0] >= 0 and d["match_end"][-1] <= 64 << 20
    assert d["match_id"].min() >= 0 and d["match_id"].max() < 5000
