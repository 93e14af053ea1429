#!/usr/bin/env python3
"""HIP-event times of the cut-off ladder on synthetic edge lists:
    python tools/sweep_times.py [--sizes 450000,45000000] [--ks 1,5,20] [--reps 10] [--nodes 20000]
For every size and K evenly spaced cut-offs in (0, 1) on column 5 it times, alternating between the two in the same run,
ksp_components_edges_sweep ("sweep") and K calls of ksp_components_edges ("separate") over the same records, and prints one
JSON line each: median, minimum and maximum in ms over the rounds, and the bytes the form moves over the edges, computed from
counts: the sweep reads every 16-byte record twice (level, scatter), writes and reads one level byte per record, writes 8
bytes per edge of level >= 1 and reads them once per hooking round of their band; the separate calls read every 16-byte
record once per hooking round of every call.  The number of rounds is whatever the graph needs, so the tool reports the
fixed bytes and the bytes per hooking round.  Both times cover everything the calls do on the device, allocations and the
copy of the labels included; the labels of the two forms are compared first."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine  # noqa: E402

NAMES = ("sweep", "separate")


def records(n, n_nodes, seed=1):
    """n records over n_nodes sources of about 5 000 k-mers in groups of 50: `shared` uniform below the smaller count, so that
    column 5 is uniform in [0, 1) and every cut-off of a ladder keeps its share."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(4500, 5501, size=n_nodes).astype(np.uint32)
    e = np.zeros(n, dtype=engine.EDGE_DTYPE)
    a = rng.integers(0, n_nodes, size=n, dtype=np.uint32)
    b = (a // 50) * 50 + rng.integers(0, 50, size=n, dtype=np.uint32)       # a neighbour inside a's group of 50
    b = np.minimum(b, n_nodes - 1).astype(np.uint32)
    e["source_1"], e["source_2"] = np.minimum(a, b), np.maximum(a, b)
    small = np.minimum(cnt[e["source_1"]], cnt[e["source_2"]])
    e["shared"] = (rng.random(n) * small).astype(np.uint64)
    return e, cnt


def times(L, which, reps, n_nodes, ed, n, cd, cutoffs, labels):
    ms = (ctypes.c_float * reps)()
    rc = L.ksp_debug_sweep_times(0, n_nodes, ed.ptr, n, cd.ptr, 5, cutoffs.ctypes.data, len(cutoffs), which, reps, ms, labels.ctypes.data)
    if rc:
        raise engine.KspError(rc, L.ksp_last_error().decode())
    return list(ms)


def main(sizes, ks, reps, n_nodes):
    L = engine.lib()
    L.ksp_debug_sweep_times.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p]
    for n in sizes:
        e, cnt = records(n, n_nodes)
        ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
        for K in ks:
            cutoffs = np.ascontiguousarray(np.arange(1, K + 1) / (K + 1), dtype=np.float64)
            out = [np.zeros((K, n_nodes), dtype=np.uint32) for _ in NAMES]
            for w in range(2):                  # warm-up, and the two forms agree
                times(L, w, 1, n_nodes, ed, n, cd, cutoffs, out[w])
            assert (out[0] == out[1]).all(), "the sweep and the separate calls disagree"
            _, kept = engine.components_edges_sweep(n_nodes, ed.ptr.value, n, cd.ptr.value, 5, cutoffs)
            ms = {w: [] for w in range(2)}
            for _ in range(reps):               # alternating: one run of each per round
                for w in range(2):
                    ms[w] += times(L, w, 1, n_nodes, ed, n, cd, cutoffs, out[w])
            banded = int(kept.max())            # the edges of level >= 1
            fixed = (16 * 2 * n + 2 * n + 8 * banded, 0)
            per_round = (8 * banded, 16 * n * K)   # the sweep: every band once per round of ITS rank; separate: every record per round of every call
            for w in range(2):
                t = np.array(ms[w])
                print(json.dumps({"records": n, "nodes": n_nodes, "K": K, "how": NAMES[w], "rounds": reps, "ms_median": round(float(np.median(t)), 3),
                                  "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3), "edge_bytes_fixed": fixed[w],
                                  "edge_bytes_per_hook_round": per_round[w], "kept_least_strict": banded}), flush=True)
        ed.free()
        cd.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="450000,45000000")
    ap.add_argument("--ks", default="1,5,20")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=20000)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("sweep_times: no GPU visible (there is nothing to time without one)")
    main([int(s) for s in a.sizes.split(",") if s], [int(k) for k in a.ks.split(",") if k], a.reps, a.nodes)
