#!/usr/bin/env python3
"""HIP-event times of compare beside the unweighted probe of the same process:
    python tools/compare_times.py [--samples 300] [--hashes 100000,1000000] [--spread 20] [--reps 7]
A synthetic set of --samples counted sketches of H hashes each, drawn from spread x H values (so a hash has about samples / spread
holders), abundances heavy-tailed.  The first sample is the database, the others the queries, mode KSP_QUERY_CROSS_AND_SELF, so
that ksp_query_device takes the same keys (it needs a database source).  For every H: the size query, two warm-up calls, then
--reps calls of ksp_compare_device and of ksp_query_device with everything resident in HBM; one JSON line with the medians of the
timers — totals, holders, table and probe of compare reported separately, table and probe of query mode — and the ratio of the
two probes.  The yardstick is the unweighted probe, not the new code against itself."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine  # noqa: E402


def samples(n, hashes, spread, seed):
    """(keys, abund, offsets): n strictly ascending runs of about `hashes` values out of spread x hashes"""
    rng = np.random.default_rng(seed)
    stride = np.uint64((2**63) // (spread * hashes))
    runs = [np.unique(rng.integers(0, spread * hashes, size=hashes, dtype=np.uint64)) * stride for _ in range(n)]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in runs])
    keys = np.concatenate(runs)
    abund = np.minimum(np.floor(rng.pareto(0.9, size=keys.size)) + 1, 60000).astype(np.uint32)
    return keys, abund, offsets


def median(values):
    return round(float(np.median(values)), 3)


def run(n, hashes, spread, reps):
    keys, abund, offsets = samples(n, hashes, spread, 23)
    cut = int(offsets[1])
    db_off, q_off = offsets[:2], offsets[1:] - offsets[1]
    d = [engine.DeviceBuffer.from_numpy(a) for a in (keys[:cut], abund[:cut], keys[cut:], abund[cut:])]
    mode = engine.QUERY_CROSS_AND_SELF
    _, needed, _, _, _ = engine.compare_device(d[0].ptr, d[1].ptr, db_off, d[2].ptr, d[3].ptr, q_off, None, 0, mode=mode)
    d_rows = engine.DeviceBuffer(40 * max(needed, 1))
    weighted = {k: [] for k in ("ms_totals", "ms_holders", "ms_table", "ms_probe")}
    plain = {k: [] for k in ("ms_table", "ms_probe")}
    st = None
    for r in range(reps + 2):
        rc, got, _, _, st = engine.compare_device(d[0].ptr, d[1].ptr, db_off, d[2].ptr, d[3].ptr, q_off, d_rows.ptr, needed, mode=mode)
        assert rc == engine.KSP_OK and got == needed
        if r >= 2:
            for k in weighted:
                weighted[k].append(st[k])
    for r in range(reps + 2):                                                   # 16-byte edges fit the 40-byte rows' buffer
        rc, got, qst = engine.query_device(d[0].ptr, db_off, d[2].ptr, q_off, d_rows.ptr, needed, mode=mode)
        assert rc == engine.KSP_OK and got == needed
        if r >= 2:
            for k in plain:
                plain[k].append(qst[k])
    line = {"samples": n, "hashes": int(keys.size), "rows": needed, "holders": st["table_holders"], "table_keys": st["table_keys"], "passes": st["passes"],
            "passes_query": qst["passes"], "list_overflows": st["list_overflows"], "calls_timed": reps}
    line.update({"compare_" + k: median(v) for k, v in weighted.items()})
    line.update({"query_" + k: median(v) for k, v in plain.items()})
    line["probe_ratio"] = round(line["compare_ms_probe"] / max(line["query_ms_probe"], 1e-6), 2)
    print(json.dumps(line), flush=True)
    for b in d + [d_rows]:
        b.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=300)
    ap.add_argument("--hashes", default="100000,1000000")
    ap.add_argument("--spread", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("compare_times: no GPU visible (there is nothing to time without one)")
    for h in [int(h) for h in a.hashes.split(",") if h]:
        run(a.samples, h, a.spread, a.reps)
