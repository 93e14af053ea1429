#!/usr/bin/env python3
"""HIP-event times of the single-linkage tree on synthetic edge lists:
    python tools/tree_times.py [--sizes 450000,45000000] [--reps 10] [--nodes 20000] [--k 20]
For every size, over the records of tools/sweep_times.py (the generator of the table in 7e) on column 5, it times in the same
run, alternating from round to round:
    tree            ksp_edges_forest's device part as shipped (a load and compare before every atomic)
    tree_no_load    the same with the atomic alone
    one_cut         one ksp_components_edges call at the cut-off 0.5 (unchanged)
    sweep_K         ksp_components_edges_sweep at K evenly spaced cut-offs (unchanged)
and prints one JSON line each: median, minimum and maximum in ms over the rounds.  Every time covers everything the call does
on the device, its allocations and the copy of its result to the host included.  The tree lines also carry the number of
rounds the graph needed and the bytes moved over the edges, from counts: the preparation reads every 16-byte record and writes
12 bytes per record; every round reads those 12 bytes per record once (and gathers two labels per record from the 4-byte-per-
node label array, which the counts leave out).  The forests of the two tree forms are compared first."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kspider_amd import engine  # noqa: E402
from sweep_times import records  # noqa: E402


def tree_times(L, which, reps, n_nodes, ed, n, cd, index):
    ms = (ctypes.c_float * reps)()
    n_forest, rounds = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = L.ksp_debug_tree_times(0, n_nodes, ed.ptr, n, cd.ptr, 5, which, reps, ms, index.ctypes.data, ctypes.byref(n_forest), ctypes.byref(rounds))
    if rc:
        raise engine.KspError(rc, L.ksp_last_error().decode())
    return list(ms), n_forest.value, rounds.value


def sweep_times(L, which, reps, n_nodes, ed, n, cd, cutoffs, labels):
    ms = (ctypes.c_float * reps)()
    rc = L.ksp_debug_sweep_times(0, n_nodes, ed.ptr, n, cd.ptr, 5, cutoffs.ctypes.data, len(cutoffs), which, reps, ms, labels.ctypes.data)
    if rc:
        raise engine.KspError(rc, L.ksp_last_error().decode())
    return list(ms)


def main(sizes, reps, n_nodes, K):
    L = engine.lib()
    L.ksp_debug_tree_times.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.ksp_debug_sweep_times.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p]
    one = np.array([0.5])
    ladder = np.ascontiguousarray(np.arange(1, K + 1) / (K + 1), dtype=np.float64)
    for n in sizes:
        e, cnt = records(n, n_nodes)
        ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
        index = [np.zeros(n_nodes, dtype=np.uint32) for _ in range(2)]
        lab1, labK = np.zeros((1, n_nodes), dtype=np.uint32), np.zeros((K, n_nodes), dtype=np.uint32)
        forests = []
        for w in range(2):                      # warm-up, and the two forms agree
            _, nf, rounds = tree_times(L, w, 1, n_nodes, ed, n, cd, index[w])
            forests.append(index[w][:nf].copy())
        assert (forests[0] == forests[1]).all(), "the two forms of the offer disagree"
        sweep_times(L, 1, 1, n_nodes, ed, n, cd, one, lab1)
        sweep_times(L, 0, 1, n_nodes, ed, n, cd, ladder, labK)
        ms = {name: [] for name in ("tree", "tree_no_load", "one_cut", f"sweep_{K}")}
        for _ in range(reps):                   # alternating: one run of each per round
            ms["tree"] += tree_times(L, 0, 1, n_nodes, ed, n, cd, index[0])[0]
            ms["tree_no_load"] += tree_times(L, 1, 1, n_nodes, ed, n, cd, index[1])[0]
            ms["one_cut"] += sweep_times(L, 1, 1, n_nodes, ed, n, cd, one, lab1)
            ms[f"sweep_{K}"] += sweep_times(L, 0, 1, n_nodes, ed, n, cd, ladder, labK)
        for name, t in ms.items():
            t = np.array(t)
            line = {"records": n, "nodes": n_nodes, "how": name, "rounds_timed": reps, "ms_median": round(float(np.median(t)), 3),
                    "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3)}
            if name.startswith("tree"):
                line.update({"boruvka_rounds": rounds, "forest_edges": int(len(forests[0])), "edge_bytes_prep": 28 * n, "edge_bytes_per_round": 12 * n})
            print(json.dumps(line), flush=True)
        ed.free()
        cd.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="450000,45000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--k", type=int, default=20)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("tree_times: no GPU visible (there is nothing to time without one)")
    main([int(s) for s in a.sizes.split(",") if s], a.reps, a.nodes, a.k)
