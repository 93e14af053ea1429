#!/usr/bin/env python3
"""HIP-event times of the top-k neighbours, hand-written select kernels against rocPRIM's segmented sort:
    python tools/topk_times.py [--workloads bench,skewed] [--ks 1,10,100] [--reps 20] [--hub 100005]
    bench     the edge list of the bench workload: the join of synth.generate("C2") (10 000 sketches, as bench.py builds
              it), its records uploaded to HBM in the join's order, column 5
    skewed    tests/topk_inputs.hubs scaled up: one hub of --hub entries (streamed), one of 3 000 (a workgroup), the small
              nodes and the leaves (waves), every record at a random position
For every workload and k it runs both modes once (warm-up; the two results are compared), then alternates them from round
to round and prints one JSON line per mode: median, minimum and maximum in ms over the rounds, and what
ksp_debug_topk_classes reports.  Every time covers everything the call does on the device, its allocations and the copy of
the result to the host included."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kspider_amd import engine, synth  # noqa: E402

MODES = ("kernels", "library")


def workload(name, hub):
    if name == "bench":
        sk = synth.generate("C2")
        e, _ = engine.pairwise_host(sk.keys, sk.offsets)
        return np.ascontiguousarray(e), sk.sizes.astype(np.uint32), sk.n_sources
    import topk_inputs as ti
    e, cnt, n_nodes, _ = ti.hubs([hub, 3000])
    return np.ascontiguousarray(e), cnt, n_nodes


def times(L, which, reps, n_nodes, ed, n, cd, k, index, count):
    ms = (ctypes.c_float * reps)()
    rc = L.ksp_debug_topk_times(0, n_nodes, ed.ptr, n, cd.ptr, 5, k, which, reps, ms, index.ctypes.data, count.ctypes.data)
    if rc:
        raise engine.KspError(rc, L.ksp_last_error().decode())
    return list(ms)


def main(workloads, ks, reps, hub):
    L = engine.lib()
    L.ksp_debug_topk_times.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                                       ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    for name in workloads:
        e, cnt, n_nodes = workload(name, hub)
        n = len(e)
        ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
        for k in ks:
            out = [(np.zeros(n_nodes * k, dtype=np.uint32), np.zeros(n_nodes, dtype=np.uint32)) for _ in MODES]
            classes = None
            for w in range(2):                      # warm-up, and the two modes agree
                times(L, w, 1, n_nodes, ed, n, cd, k, *out[w])
                if w == 0:
                    classes = engine.topk_classes()
            assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all(), "the two modes disagree"
            ms = {m: [] for m in MODES}
            for _ in range(reps):                   # alternating: one run of each per round
                for w, m in enumerate(MODES):
                    ms[m] += times(L, w, 1, n_nodes, ed, n, cd, k, *out[w])
            for m in MODES:
                t = np.array(ms[m])
                print(json.dumps({"workload": name, "records": n, "nodes": n_nodes, "k": k, "select": m, "rounds_timed": reps,
                                  "ms_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                                  "hits": int(out[0][1].sum()), "classes": classes}), flush=True)
        ed.free()
        cd.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="bench,skewed")
    ap.add_argument("--ks", default="1,10,100")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hub", type=int, default=100005)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("topk_times: no GPU visible (there is nothing to time without one)")
    main([w for w in a.workloads.split(",") if w], [int(k) for k in a.ks.split(",") if k], a.reps, a.hub)
