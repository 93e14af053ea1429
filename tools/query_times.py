#!/usr/bin/env python3
"""HIP-event times of query mode against the full pairwise pass and against the copy-rate floor:
    python tools/query_times.py [--workloads bench,skewed,short] [--qs 1,100,1000,10000] [--reps 11] [--short-sources 1000000]
    bench     the database has the bench workload's shape (synth.generate("C2"): 10 000 sources, 5 x 10^7 hashes); the queries
              come from the same generator (one set of 10 000 + max(Q) sources, shuffled with a fixed seed; the first 10 000
              are the database, the next Q the queries)
    skewed    C4's law (lognormal run lengths up to 2 x 10^6), --skewed-sources of them, 100 queries of the same law
    short     C5's law (16 .. 256 hashes), --short-sources of them, 100 queries of the same law
For every workload and Q, in cross mode with the database resident in HBM: the size query, two warm-up calls, then --reps calls
of ksp_query_device; one JSON line with the medians of ms_table and ms_probe (HIP events, summed over the query tiles), the
floor (8 bytes per database hash and pass at the copy rate measured in this run: device-to-device hipMemcpy of 1 GiB, read +
write counted), and — with --baseline — what the full pass needs for the same answer: ksp_engine_build_blocks +
ksp_engine_join over the concatenation (ms_build + ms_join, medians) and the edges it produces."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine, synth  # noqa: E402


def copy_rate(reps):
    """bytes per ms moved by a device-to-device copy (read + write)"""
    L = engine.lib()
    L.ksp_debug_copy_times.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    n = 1 << 30
    ms = (ctypes.c_float * (reps + 2))()
    engine._check(L.ksp_debug_copy_times(0, n, reps + 2, ms))
    return 2 * n / float(np.median(list(ms)[2:]))


def shuffled(config, n, seed):
    sk = synth.generate(config, n_sources=n)
    order = np.random.default_rng(seed).permutation(sk.n_sources)
    sizes = sk.sizes[order]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(sizes)
    keys = np.empty(sk.keys.size, dtype=np.uint64)
    for new, old in enumerate(order):
        keys[int(offsets[new]):int(offsets[new + 1])] = sk.run(int(old))
    return keys, offsets


def baseline(keys, offsets, n_sources, reps):
    """ms_build + ms_join of the full pass over the first n_sources runs, and its edges"""
    end = int(offsets[n_sources])
    d_keys = engine.DeviceBuffer.from_numpy(keys[:end])
    eng = engine.Engine(0)
    ms, edges = [], 0
    d_edges = None
    for r in range(reps + 1):
        eng.build_blocks(d_keys.ptr, offsets[:n_sources + 1])
        if d_edges is None:
            cap = eng.edge_bound(0, eng.num_tiles) + 1
            d_edges = engine.DeviceBuffer(16 * cap)
        edges = eng.join(0, eng.num_tiles, d_edges.ptr, cap)
        st = eng.stats()
        if r:
            ms.append(st["ms_build"] + st["ms_join"])
    eng.close()
    d_keys.free()
    d_edges.free()
    return float(np.median(ms)), int(edges)


def run(name, keys, offsets, n_db, qs, reps, rate, with_baseline):
    db_end = int(offsets[n_db])
    d_db = engine.DeviceBuffer.from_numpy(keys[:db_end])
    db_off = offsets[:n_db + 1]
    for q in qs:
        q_off = offsets[n_db:n_db + q + 1] - offsets[n_db]
        d_q = engine.DeviceBuffer.from_numpy(keys[db_end:db_end + int(q_off[-1])])
        _, needed, _ = engine.query_device(d_db.ptr, db_off, d_q.ptr, q_off, None, 0)
        d_edges = engine.DeviceBuffer(16 * max(needed, 1))
        table, probe, st = [], [], None
        for r in range(reps + 2):
            rc, n, st = engine.query_device(d_db.ptr, db_off, d_q.ptr, q_off, d_edges.ptr, needed)
            assert rc == engine.KSP_OK and n == needed
            if r >= 2:
                table.append(st["ms_table"])
                probe.append(st["ms_probe"])
        line = {"workload": name, "db_sources": n_db, "db_hashes": db_end, "queries": q, "query_hashes": int(q_off[-1]), "edges": needed,
                "passes": st["passes"], "short_sources": st["short_sources"], "long_sources": st["long_sources"], "list_overflows": st["list_overflows"],
                "table_keys": st["table_keys"], "ms_table": round(float(np.median(table)), 3), "ms_probe": round(float(np.median(probe)), 3),
                "ms_probe_min": round(float(np.min(probe)), 3), "ms_probe_max": round(float(np.max(probe)), 3),
                "ms_floor": round(8.0 * db_end * st["passes"] / rate, 3), "copy_GBps": round(rate / 1e6, 1), "calls_timed": reps}
        if with_baseline:
            ms_full, full_edges = baseline(keys, offsets, n_db + q, max(3, reps // 2))
            line.update({"ms_full_pass": round(ms_full, 3), "full_pass_edges": full_edges, "full_pass_edge_bytes": 16 * full_edges})
        print(json.dumps(line), flush=True)
        d_q.free()
        d_edges.free()
    d_db.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="bench,skewed,short")
    ap.add_argument("--qs", default="1,100,1000,10000")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--skewed-sources", type=int, default=5000)
    ap.add_argument("--short-sources", type=int, default=1000000)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("query_times: no GPU visible (there is nothing to time without one)")
    rate = copy_rate(a.reps)
    qs = [int(q) for q in a.qs.split(",") if q]
    for w in [w for w in a.workloads.split(",") if w]:
        if w == "bench":
            n_db = 10000
            keys, offsets = shuffled("C2", n_db + max(qs), 17)
            run(w, keys, offsets, n_db, qs, a.reps, rate, a.baseline)
        elif w == "skewed":
            keys, offsets = shuffled("C4", a.skewed_sources + 100, 18)
            run(w, keys, offsets, a.skewed_sources, [100], a.reps, rate, a.baseline)
        elif w == "short":
            keys, offsets = shuffled("C5", a.short_sources + 100, 19)
            run(w, keys, offsets, a.short_sources, [100], a.reps, rate, False)
        else:
            raise SystemExit(f"query_times: unknown workload {w}")
