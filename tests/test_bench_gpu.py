"""bench.py on the GPU box: the 1-rank --full line is well-formed, --dump-outputs writes the edge set the line's
checksum describes, a plain run does nothing but its timed steps (no phase pass, no CPU baseline), and a 2-rank run (both ranks on the one card, gloo for the exchange — the box has a single
GPU, RCCL needs one device per rank) gathers exactly the edge set of the 1-rank run: tile-range sharding +
gather on real engine output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, env):
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_bench_line_and_two_rank_equivalence(tmp_path):
    common = ["--steps", "2", "--warmup", "1", "--n-sources", "1500", "--cpu-sample", "0"]
    dump = str(tmp_path / "outputs")
    one = _run([sys.executable, "bench.py", "--gpus", "1", "--full"] + common + ["--dump-outputs", dump],
               {"KSP_BENCH_CHECKSUM": "1"})
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in one
    assert one["n_gpus"] == 1 and one["config"]["n_sources"] == 1500 and one["value"] > 0
    assert one["roofline"]["bound"] == "hbm" and one["roofline"]["peak"] == 8000.0
    # a roofline FRACTION: recomputable from the line itself, never above 1
    r = one["roofline"]
    assert 0 < r["frac"] <= 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert abs(r["achieved"] - r["bytes_per_step"] / (one["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["groups"] and {"partition", "join"} <= {g["group"] for g in r["groups"]}
    assert all(g["ms"] > 0 for g in r["groups"])
    assert one["naive_pairwise"]["bytes_per_step"] > r["bytes_per_step"]
    assert one["config"]["buffers_regrown_in_timed_region"] == 0
    assert one["steps"] == 2 and one["ms_per_step"] > 0
    # --dump-outputs: the whole edge set of the last timed step (small enough not to be sampled), rows ordered
    assert one["dump_outputs"]["rows"] == one["config"]["nonzero_pairs"] and not one["dump_outputs"]["sampled"]
    cols = {k: np.load(os.path.join(dump, k + ".npy")) for k in ("source_1", "source_2", "shared")}
    assert all(c.dtype == np.float64 and len(c) == one["config"]["nonzero_pairs"] for c in cols.values())
    assert (np.diff(cols["source_1"]) >= 0).all() and (cols["source_1"] < cols["source_2"]).all()
    u = {k: c.astype(np.uint64) for k, c in cols.items()}
    x = (u["source_1"] << np.uint64(40)) + (u["source_2"] << np.uint64(20)) + u["shared"]
    assert int(x.sum(dtype=np.uint64)) == one["config"]["checksum"]
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", "29713", "bench.py", "--gpus", "2"] + common,
               {"KSP_BENCH_CHECKSUM": "1", "KSP_BENCH_SHARE_GPU": "1", "KSP_BENCH_BACKEND": "gloo"})
    assert two["n_gpus"] == 2
    assert two["config"]["nonzero_pairs"] == one["config"]["nonzero_pairs"] > 1000
    assert two["config"]["checksum"] == one["config"]["checksum"] != 0


def test_bench_plain_line(tmp_path):
    """Without --full: the headline fields and --dump-outputs as in a --full run, but no phase pass, no CPU baseline
    (its sample size left at the default) and no other configs."""
    dump = str(tmp_path / "outputs")
    line = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--n-sources", "1500",
                 "--dump-outputs", dump], {})
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype", "config", "roofline"):
        assert k in line
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2
    assert line["roofline"]["groups"] == [] and 0 < line["roofline"]["frac"] <= 1
    assert not {"cpu_baseline", "dropin_s", "other_configs"} & set(line)
    assert line["config"]["verified_against_cpu_baseline"] is None
    assert line["dump_outputs"]["rows"] == line["config"]["nonzero_pairs"] > 1000
    u = {k: np.load(os.path.join(dump, k + ".npy")).astype(np.uint64) for k in ("source_1", "source_2", "shared")}
    x = (u["source_1"] << np.uint64(40)) + (u["source_2"] << np.uint64(20)) + u["shared"]
    assert int(x.sum(dtype=np.uint64)) == line["config"]["checksum"] != 0
