#!/usr/bin/env python3
"""Times of gather on the bench database, beside one query-mode call on the same inputs:
    python tools/gather_times.py [--reps 11] [--picks 50] [--noise 50000] [--min-hashes 50] [--sources 10000] [--abund]
The database has the bench workload's shape (synth.generate("C2"): 10 000 sources, 5 x 10^7 hashes) and stays resident in HBM.
The sample is synthetic: the union of random halves of --picks database sources plus --noise hashes that no source holds
(synth.gather_sample).  For each setting of the rounds — the default (the one-workgroup tail once few candidates are live),
KSP_GATHER_TAIL=0 (batches of rounds to the end) and KSP_GATHER_TAIL_CANDS=1048576 (the tail at once) — the size query, two
warm-up calls, then --reps calls of ksp_gather_device; one JSON line with the medians of the whole call (wall clock around the
call) and of its four phases (HIP events), the rounds, the batches (= reads of the live count) and which path ran the rounds.  The last line is ksp_query_device on the same inputs, the
baseline: it is one pass over the database, what a caller without gather pays per row found.
--abund: under every setting the weighted call ksp_gather_abund_device follows the unweighted one on the same inputs
in the same process — the sample's hashes get seeded log-normal abundances —, and its line also says what it costs more, as a
whole and in the rounds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine, synth  # noqa: E402


def timed(call, reps):
    """(the last result, wall ms of every timed call) after two warm-up calls"""
    out, wall = None, []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        out = call()
        if r >= 2:
            wall.append(1e3 * (time.perf_counter() - t0))
    return out, wall


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--picks", type=int, default=50)
    ap.add_argument("--noise", type=int, default=50000)
    ap.add_argument("--min-hashes", type=int, default=50)
    ap.add_argument("--sources", type=int, default=10000)
    ap.add_argument("--abund", action="store_true")
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("gather_times: no GPU visible (there is nothing to time without one)")
    sk = synth.generate("C2", n_sources=a.sources)
    sample = synth.gather_sample(sk, a.picks, a.noise, seed=23)
    q_off = np.array([0, sample.size], dtype=np.uint64)
    d_db, d_q = engine.DeviceBuffer.from_numpy(sk.keys), engine.DeviceBuffer.from_numpy(sample)
    abund = np.minimum(np.random.default_rng(29).lognormal(2.0, 1.5, size=sample.size) + 1, 2**32 - 1).astype(np.uint32)
    d_a = engine.DeviceBuffer.from_numpy(abund) if a.abund else None
    common = {"db_sources": sk.n_sources, "db_hashes": int(sk.keys.size), "sample_hashes": int(sample.size), "picks": a.picks, "min_hashes": a.min_hashes,
              "calls_timed": a.reps}
    rows = 0
    for setting, env in (("default", {}), ("KSP_GATHER_TAIL=0", {"KSP_GATHER_TAIL": "0"}), ("KSP_GATHER_TAIL_CANDS=1048576", {"KSP_GATHER_TAIL_CANDS": "1048576"})):
        os.environ.update(env)
        _, rows, _ = engine.gather_device(d_db.ptr, sk.offsets, d_q.ptr, q_off, None, 0, min_hashes=a.min_hashes)
        d_rows = engine.DeviceBuffer(24 * max(rows, 1))
        stats = []

        def call():
            rc, n, st = engine.gather_device(d_db.ptr, sk.offsets, d_q.ptr, q_off, d_rows.ptr, rows, min_hashes=a.min_hashes)
            assert rc == engine.KSP_OK and n == rows
            stats.append(st)
            return st
        st, wall = timed(call, a.reps)
        med = lambda k: round(float(np.median([s[k] for s in stats[2:]])), 3)   # noqa: E731
        in_batches = st["rounds"] - st["tail_rounds"]
        print(json.dumps({**common, "setting": setting, "rows": rows, "candidates": st["candidates"], "dropped": st["dropped"], "fell_below": st["fell_below"],
                          "slots": st["slots"], "rounds": st["rounds"], "rounds_in_batches": in_batches, "rounds_in_tail": st["tail_rounds"],
                          "live_at_tail": st["live_at_tail"], "batch_reads": st["batches"],
                          "rounds_per_batch_read": round(in_batches / st["batches"], 2) if st["batches"] else None,
                          "path": "tail" if in_batches == 0 else ("batches" if st["tail_rounds"] == 0 else "batches, then tail"),
                          "ms_call": round(float(np.median(wall)), 3), "ms_call_min": round(float(np.min(wall)), 3), "ms_table": med("ms_table"),
                          "ms_candidates": med("ms_candidates"), "ms_fill": med("ms_fill"), "ms_rounds": med("ms_rounds")}), flush=True)
        d_rows.free()
        if a.abund:
            d_wrows = engine.DeviceBuffer(64 * max(rows, 1))
            w_stats = []

            def wcall():
                rc, n, wst = engine.gather_abund_device(d_db.ptr, sk.offsets, d_q.ptr, d_a.ptr, q_off, d_wrows.ptr, rows, min_hashes=a.min_hashes)
                assert rc == engine.KSP_OK and n == rows
                w_stats.append(wst)
                return wst
            wst, w_wall = timed(wcall, a.reps)
            wmed = lambda k: round(float(np.median([s[k] for s in w_stats[2:]])), 3)   # noqa: E731
            taken = d_wrows.to_numpy(engine.GATHER_WROW_DTYPE, rows)["unique"] if rows else np.zeros(0, dtype=np.uint32)
            print(json.dumps({**common, "setting": setting, "call": "ksp_gather_abund_device", "rows": rows, "rounds": wst["rounds"], "rounds_in_tail": wst["tail_rounds"],
                              "largest_take": int(taken.max()) if rows else 0, "takes_above_64": int((taken > 64).sum()),
                              "ms_call": round(float(np.median(w_wall)), 3), "ms_call_min": round(float(np.min(w_wall)), 3), "ms_table": wmed("ms_table"),
                              "ms_candidates": wmed("ms_candidates"), "ms_fill": wmed("ms_fill"), "ms_rounds": wmed("ms_rounds"),
                              "ms_call_more_than_unweighted": round(float(np.median(w_wall)) - float(np.median(wall)), 3),
                              "ms_fill_more_than_unweighted": round(wmed("ms_fill") - med("ms_fill"), 3),
                              "ms_rounds_more_than_unweighted": round(wmed("ms_rounds") - med("ms_rounds"), 3)}), flush=True)
            d_wrows.free()
        for k in env:
            del os.environ[k]
    _, needed, _ = engine.query_device(d_db.ptr, sk.offsets, d_q.ptr, q_off, None, 0)
    d_edges = engine.DeviceBuffer(16 * max(needed, 1))
    q_stats = []

    def query():
        rc, n, st = engine.query_device(d_db.ptr, sk.offsets, d_q.ptr, q_off, d_edges.ptr, needed)
        assert rc == engine.KSP_OK and n == needed
        q_stats.append(st)
        return st
    _, wall = timed(query, a.reps)
    ms_query = float(np.median(wall))
    print(json.dumps({**common, "setting": "ksp_query_device (one pass, the baseline)", "edges": needed, "ms_call": round(ms_query, 3), "ms_call_min": round(float(np.min(wall)), 3),
                      "ms_table": round(float(np.median([s["ms_table"] for s in q_stats[2:]])), 3),
                      "ms_probe": round(float(np.median([s["ms_probe"] for s in q_stats[2:]])), 3),
                      "ms_one_query_call_per_row": round(ms_query * rows, 3)}), flush=True)
