#!/usr/bin/env python3
"""HIP-event times and rounds of the average-linkage tree:
    python tools/upgma_times.py [--reps 3] [--paths 256,1024,4096,16384,65536] [--host-max 16384] [--bench] [--dense 0] [--tails 0,4096]
--paths   a path of P + 1 nodes with strictly decreasing values (the bad case of the rounds: about 0.6 * P of them), P live pairs
          after the first fold.  Per P one JSON line: the whole call with KSP_UPGMA_TAIL_PAIRS=0 (the device to the end), its rounds
          and the time per round; and, up to --host-max pairs, the whole call with the threshold above P (the host finishes at once):
          the host finish is O(pairs) per merge.  KSP_UPGMA_TAIL_PAIRS belongs where the two cross.
--bench   the bench workload's edge list (the join of synth.generate("C2"), 10 000 sketches) at the shipped threshold and at every
          threshold of --tails.
--dense N all N * (N - 1) / 2 pairs of N sources (10 000: 5 * 10^7 records) with seeded shared counts, at the same thresholds.
Every time covers everything the call does, its allocations, its copies and the host finish included; one warm-up run first."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine, synth  # noqa: E402


def timed(e, cnt, n_nodes, reps, tail):
    if tail is None:
        os.environ.pop("KSP_UPGMA_TAIL_PAIRS", None)
    else:
        os.environ["KSP_UPGMA_TAIL_PAIRS"] = str(tail)
    L = engine.lib()
    ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
    rows = np.zeros(max(n_nodes, 1), dtype=engine.UPGMA_ROW_DTYPE)
    n_rows, counts = np.zeros(1, dtype=np.uint32), np.zeros(6, dtype=np.uint64)
    ms = (ctypes.c_float * (reps + 1))()
    rc = L.ksp_debug_upgma_times(0, n_nodes, ed.ptr, len(e), cd.ptr, 5, reps + 1, ms, rows.ctypes.data, n_rows.ctypes.data, counts.ctypes.data)
    ed.free()
    cd.free()
    if rc:
        raise engine.KspError(rc, L.ksp_last_error().decode())
    t = np.array(list(ms))[1:]                                             # (the first run warms up)
    return {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3), "rows": int(n_rows[0]),
            "first_pairs": int(counts[0]), "rounds": int(counts[1]), "device_merges": int(counts[2]), "handed_over": int(counts[3]), "host_merges": int(counts[4])}


def path_records(P):
    e = np.zeros(P, dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"] = np.arange(P), np.arange(P) + 1
    e["shared"] = (1 << 20) - np.arange(P)                                 # over 2^20 k-mers: strictly decreasing, exact floats
    return e, np.full(P + 1, 1 << 20, dtype=np.uint32)


def main(a):
    for P in a.paths:
        e, cnt = path_records(P)
        out = {"input": "path", "pairs": P, "device": timed(e, cnt, P + 1, a.reps, 0)}
        out["device_ms_per_round"] = round(out["device"]["ms_median"] / max(1, out["device"]["rounds"]), 4)
        if P <= a.host_max:
            out["host"] = timed(e, cnt, P + 1, a.reps, P + 1)
        print(json.dumps(out), flush=True)
    if a.bench:
        sk = synth.generate("C2")
        e, _ = engine.pairwise_host(sk.keys, sk.offsets)
        e, cnt = np.ascontiguousarray(e), sk.sizes.astype(np.uint32)
        out = {"input": "bench", "records": len(e), "nodes": sk.n_sources, "shipped": timed(e, cnt, sk.n_sources, a.reps, None)}
        out.update({f"tail_{t}": timed(e, cnt, sk.n_sources, a.reps, t) for t in a.tails})
        print(json.dumps(out), flush=True)
    if a.dense:
        N = a.dense
        rng = np.random.default_rng(7)
        s1, s2 = np.triu_indices(N, 1)
        e = np.zeros(len(s1), dtype=engine.EDGE_DTYPE)
        e["source_1"], e["source_2"], e["shared"] = s1, s2, rng.integers(1, 1 << 20, len(s1))
        del s1, s2
        cnt = np.full(N, 1 << 20, dtype=np.uint32)
        out = {"input": "dense", "records": len(e), "nodes": N, "shipped": timed(e, cnt, N, a.reps, None)}
        out.update({f"tail_{t}": timed(e, cnt, N, a.reps, t) for t in a.tails})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--paths", default="256,1024,4096,16384,65536")
    ap.add_argument("--host-max", type=int, default=16384)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--dense", type=int, default=0)
    ap.add_argument("--tails", default="")
    a = ap.parse_args()
    a.paths = [int(p) for p in a.paths.split(",") if p]
    a.tails = [int(t) for t in a.tails.split(",") if t]
    if engine.device_count() < 1:
        raise SystemExit("upgma_times: no GPU visible (there is nothing to time without one)")
    main(a)
