#!/usr/bin/env python3
"""HIP-event times of classify beside the route that existed before it, on the same bytes:
    python tools/classify_times.py [--records 1000000] [--length 150] [--ksize 31] [--scaled 100] [--db-sources 10000]
                                   [--hit-rates 0,0.01,0.1] [--reps 5] [--cpu-records 20000]
The reads: --records seeded synthetic records of --length uniform ACGT bases, each followed by a newline.  The database: the bench
workload's shape (synth.generate("C2"): --db-sources sources, what tools/query_times.py uses), to which 16 references are added that hold
the sketch hashes of a share `hit rate` of the reads, so that this share of the reads hits and the rest does not.  Per hit rate:
    classify  two warm-up calls, then --reps calls of ksp_classify_host: the medians and the spread of ms_table, ms_hash, ms_finish
    before    ksp_sketch_host with every record a source (two warm-up calls, --reps calls), then ksp_query_host of those sketches
              against the database (one warm-up call, --reps calls): the medians of their HIP-event times (hash, select; table,
              probe, sort) and of the wall time of both calls
    floor     one byte per base at the copy rate measured in this run (device-to-device hipMemcpy of 1 GiB, read + write counted)
and whether both routes found the same (record, reference, hits) rows.  ksp_classify_cpu runs once over the first --cpu-records
records (one thread, wall clock).  One JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

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


def reads(n, length, seed=20261):
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n * (length + 1), dtype=np.uint8)]
    seq[length::length + 1] = ord("\n")
    return seq, np.arange(n + 1, dtype=np.uint64) * np.uint64(length + 1)


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1000000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--ksize", type=int, default=31)
    ap.add_argument("--scaled", type=int, default=100)
    ap.add_argument("--db-sources", type=int, default=10000)
    ap.add_argument("--hit-rates", default="0,0.01,0.1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-records", type=int, default=20000)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("classify_times: no GPU (a time is measured on the device or not at all)")
    max_hash = engine.sketch_max_hash(a.scaled)
    seq, off = reads(a.records, a.length)
    n_bytes = int(seq.size)
    # ---- the route before classify, first half: every record's sketch (the same for every hit rate)
    sk_times = {"ms_hash": [], "ms_select": [], "ms_upload": [], "wall_s": []}
    for r in range(2 + a.reps):   # (two warm-up calls, as for classify)
        t0 = time.perf_counter()
        q_keys, q_off, sk_st = engine.sketch_host(seq, off, a.ksize, max_hash=max_hash)
        if r >= 2:
            sk_times["wall_s"].append(time.perf_counter() - t0)
            for name in ("ms_hash", "ms_select", "ms_upload"):
                sk_times[name].append(sk_st[name])
    sk_med = {name: float(np.median(v)) for name, v in sk_times.items()}
    sketch_wall = sk_med["wall_s"]
    db = synth.generate("C2", n_sources=a.db_sources)
    # (the synthetic hashes spread over all 64 bits: divided by `scaled` they lie below max_hash, as a sketch at that `scaled` does)
    base_runs = [np.unique(db.keys[int(db.offsets[s]):int(db.offsets[s + 1])] // np.uint64(a.scaled)) for s in range(a.db_sources)]
    base_runs = [r[r <= max_hash] for r in base_runs]
    rate = copy_rate(5)
    out = {"workload": {"records": a.records, "length": a.length, "ksize": a.ksize, "scaled": a.scaled, "bytes": n_bytes, "db_sources": a.db_sources,
                        "db_hashes": int(sum(r.size for r in base_runs))},
           "sketch": dict({name: spread(v) for name, v in sk_times.items()}, kept=sk_st["kept"]),
           "floor_ms_one_byte_per_base": n_bytes / rate, "copy_rate_GBps": rate * 1e3 / 1e9, "rates": []}
    for text in a.hit_rates.split(","):
        share = float(text)
        n_hit = int(round(share * a.records))
        planted = np.unique(q_keys[:int(q_off[n_hit])])   # the hashes of the first n_hit reads
        runs = base_runs + [planted[i::16] for i in range(16)]
        ref_keys = np.concatenate(runs) if runs else np.zeros(0, np.uint64)
        ref_off = np.zeros(len(runs) + 1, dtype=np.uint64)
        ref_off[1:] = np.cumsum([r.size for r in runs])
        times = {"ms_table": [], "ms_hash": [], "ms_finish": []}
        for r in range(2 + a.reps):
            rows, arrays, st = engine.classify_host(seq, off, a.ksize, ref_keys, ref_off, max_hash=max_hash)
            if r >= 2:
                for name in times:
                    times[name].append(st[name])
        q_times = {"ms_table": [], "ms_probe": [], "ms_sort": [], "wall_s": []}
        for r in range(1 + a.reps):   # (one warm-up call)
            t0 = time.perf_counter()
            edges, qst = engine.query_host(ref_keys, ref_off, q_keys, q_off)
            if r >= 1:
                q_times["wall_s"].append(time.perf_counter() - t0)
                for name in ("ms_table", "ms_probe", "ms_sort"):
                    q_times[name].append(qst[name])
        q_med = {name: float(np.median(v)) for name, v in q_times.items()}
        query_wall = q_med["wall_s"]
        n_refs = len(runs)
        same = bool(rows.size == edges.size and (rows["reference"] == edges["source_1"]).all() and (rows["record"] + n_refs == edges["source_2"]).all() and
                    (rows["hits"] == edges["shared"]).all()) if rows.size == edges.size else False
        if rows.size == edges.size and not same:   # (the query's rows are ordered by (reference, record))
            order = np.lexsort((edges["source_1"], edges["source_2"]))
            e = edges[order]
            same = bool((rows["reference"] == e["source_1"]).all() and (rows["record"] + n_refs == e["source_2"]).all() and (rows["hits"] == e["shared"]).all())
        out["rates"].append({
            "hit_rate": share, "reads_hit": int((arrays["matched"] > 0).sum()), "rows": int(rows.size), "kept_windows": st["kept_windows"], "hit_words": st["hit_words"],
            "hit_words_unique": st["hit_words_unique"], "table_keys": st["table_keys"], "workgroups": st["workgroups"], "retries": st["retries"],
            "classify": {name: spread(v) for name, v in times.items()},
            "before": {"query_ms_table": q_med["ms_table"], "query_ms_probe": q_med["ms_probe"], "query_ms_sort": q_med["ms_sort"], "query_wall_s": query_wall,
                       "device_ms": sk_med["ms_hash"] + sk_med["ms_select"] + q_med["ms_table"] + q_med["ms_probe"] + q_med["ms_sort"], "wall_s": sketch_wall + query_wall},
            "hash_over_sketch_hash": float(np.median(times["ms_hash"])) / sk_med["ms_hash"], "same_rows": same})
    n_cpu = min(a.cpu_records, a.records)
    t0 = time.perf_counter()
    engine.classify_cpu(seq[:int(off[n_cpu])], off[:n_cpu + 1], a.ksize, ref_keys, ref_off, max_hash=max_hash)
    cpu_s = time.perf_counter() - t0
    out["cpu_one_thread"] = {"records": n_cpu, "seconds_with_table_build": cpu_s, "bases_per_s": int(off[n_cpu]) / cpu_s}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
