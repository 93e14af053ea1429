#!/usr/bin/env python3
"""HIP-event times of the cluster report beside ksp_components_edges on the same records in the same run:
    python tools/report_times.py [--cutoffs 0.0,0.1] [--reps 10] [--col 5]
The edge list is the bench workload's: the join of synth.generate("C2") (10 000 sketches, as bench.py builds it), its records
uploaded to HBM in the join's order.  One warm-up round, then per cut-off one JSON line: median, minimum and maximum in ms over the
rounds of the report's whole device part (allocations and the copies to the host included), of its accumulate, medoid and links
passes alone, and of ksp_components_edges (the labels are what both pay: the difference is the price of the report), and what
ksp_debug_report_counts reports."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine, synth  # noqa: E402

PARTS = ("report", "accumulate", "medoid", "links", "components_edges")


def main(cutoffs, reps, col):
    L = engine.lib()
    sk = synth.generate("C2")
    e, _ = engine.pairwise_host(sk.keys, sk.offsets)
    e, cnt, n_nodes = np.ascontiguousarray(e), sk.sizes.astype(np.uint32), sk.n_sources
    n = len(e)
    ed, cd = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt)
    cluster = np.zeros(n_nodes, dtype=engine.CLUSTER_ROW_DTYPE)
    member = np.zeros(n_nodes, dtype=engine.MEMBER_ROW_DTYPE)
    n_clusters = np.zeros(1, dtype=np.uint32)
    for cutoff in cutoffs:
        ms = (ctypes.c_float * (5 * (reps + 1)))()
        rc = L.ksp_debug_report_times(0, n_nodes, ed.ptr, n, cd.ptr, col, cutoff, reps + 1, ms, cluster.ctypes.data, n_clusters.ctypes.data, member.ctypes.data)
        if rc:
            raise engine.KspError(rc, L.ksp_last_error().decode())
        t = np.array(list(ms)).reshape(reps + 1, 5)[1:]            # (the first round warms up)
        out = {"records": n, "nodes": n_nodes, "col": col, "cutoff": cutoff, "rounds_timed": reps, "clusters": int(n_clusters[0]),
               "largest": int(cluster["size"][:int(n_clusters[0])].max()), "counts": engine.report_counts()}
        for i, part in enumerate(PARTS):
            out[part] = {"ms_median": round(float(np.median(t[:, i])), 3), "ms_min": round(float(t[:, i].min()), 3), "ms_max": round(float(t[:, i].max()), 3)}
        print(json.dumps(out), flush=True)
    ed.free()
    cd.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cutoffs", default="0.0,0.1")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--col", type=int, default=5)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("report_times: no GPU visible (there is nothing to time without one)")
    main([float(c) for c in a.cutoffs.split(",") if c], a.reps, a.col)
