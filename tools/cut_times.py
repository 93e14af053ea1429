#!/usr/bin/env python3
"""HIP-event times of the containment cut on synthetic edge lists:
    python tools/cut_times.py [--sizes 450000,45000000] [--reps 20] [--e2e N_SOURCES [--index PREFIX]]
For every size and a pass rate of about 10 %, 50 % and 100 % it times, alternating between them, count + scan + scatter with
the predicate evaluated in both passes ("twice"), with the count pass's ballots kept ("ballots"), and rocprim::select with
the same predicate as a functor ("select", the yardstick), and prints one JSON line each: median, minimum and maximum in
ms, and the achieved bytes per second of the algorithm's own traffic (16 bytes per record read in each pass that reads it,
16 bytes per kept record written, the ballots written once and read once).  The outputs of the three are compared first.
--e2e N: wall time of kspider_pairwise_cut at max_cont 0.5 and 0.8 against kspider_pairwise on a C2 index of N sources
(--index PREFIX: keep the index files there, and use them when they exist)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine, synth  # noqa: E402

NAMES = ("twice", "ballots", "select")


def records(n, seed=1):
    """n records over 20 000 sources of about 5 000 k-mers, `shared` uniform below the smaller count."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(4500, 5501, size=20000).astype(np.uint32)
    e = np.zeros(n, dtype=engine.EDGE_DTYPE)
    e["source_1"] = rng.integers(0, 10000, size=n, dtype=np.uint32)
    e["source_2"] = rng.integers(10000, 20000, size=n, dtype=np.uint32)
    small = np.minimum(cnt[e["source_1"]], cnt[e["source_2"]])
    e["shared"] = (rng.random(n) * small).astype(np.uint64)
    return e, cnt


def cut_times(L, which, reps, ed, n, cd, od, col, cutoff):
    ms = (ctypes.c_float * reps)()
    kept = ctypes.c_uint64(0)
    rc = L.ksp_debug_cut_times(0, ed.ptr, n, cd.ptr, col, cutoff, od.ptr, which, reps, ms, ctypes.byref(kept))
    if rc:
        raise engine.KspError(rc, L.ksp_last_error().decode())
    return list(ms), kept.value


def kernel_times(sizes, reps):
    L = engine.lib()
    L.ksp_debug_cut_times.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)]
    for n in sizes:
        e, cnt = records(n)
        ed, cd, od = engine.DeviceBuffer.from_numpy(e), engine.DeviceBuffer.from_numpy(cnt), engine.DeviceBuffer(n * 16)
        for cutoff in (0.9, 0.5, 0.0):          # max containment = shared / smaller count: uniform in [0, 1)
            outs = []
            for w in range(3):                  # warm-up, and the three ways agree
                _, kept = cut_times(L, w, 2, ed, n, cd, od, 5, cutoff)
                outs.append((kept, od.to_numpy(engine.EDGE_DTYPE, n)[:kept].tobytes() if n <= 1_000_000 else None))
            assert outs[0] == outs[1] == outs[2], "the three ways to cut disagree"
            ms = {w: [] for w in range(3)}
            for _ in range(reps):               # alternating: one run of each per round
                for w in range(3):
                    ms[w] += cut_times(L, w, 1, ed, n, cd, od, 5, cutoff)[0]
            kept = outs[0][0]
            for w in range(3):
                t = np.array(ms[w])
                # what the algorithm itself moves: every record read per pass, the kept ones written; with the ballots the
                # second pass reads the kept records only, and the ballots are written once and read once
                nbytes = (32 * n + 16 * kept, 16 * n + 32 * kept + 16 * (n // 64), 16 * n + 16 * kept)[w]
                print(json.dumps({"records": n, "cutoff": cutoff, "kept": kept, "pass_rate": round(kept / n, 4), "how": NAMES[w],
                                  "ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                                  "algorithm_GBps": round(nbytes / float(np.median(t)) / 1e6, 1)}), flush=True)
        for b in (ed, cd, od):
            b.free()


def end_to_end(n_sources, index=None, rounds=3):
    import oracle
    with tempfile.TemporaryDirectory() as d:
        prefix = index or os.path.join(d, "ix")
        if not os.path.exists(prefix + "_color_to_sources.bin"):
            sk = synth.generate("C2", n_sources=n_sources)
            oracle.index_from_sketches(prefix, sk.keys, sk.offsets)
        os.environ["KSPIDER_VERBOSE"] = "1"
        engine.pairwise(prefix, 16)             # warm-up: code objects, the file cache
        runs = [("pairwise", None), ("pairwise_cut", 0.5), ("pairwise_cut", 0.8)]
        wall = {r: [] for r in runs}
        for _ in range(rounds):
            for r in runs:
                t0 = time.perf_counter()
                if r[1] is None:
                    engine.pairwise(prefix, 16)
                else:
                    engine.pairwise_cut(prefix, 16, "max_cont", r[1])
                wall[r].append(time.perf_counter() - t0)
                rows = sum(1 for _ in open(prefix + "_kSpider_pairwise.tsv")) - 1
                size = os.path.getsize(prefix + "_kSpider_pairwise.tsv")
                print(json.dumps({"e2e": r[0], "cutoff": r[1], "sources": n_sources, "rows": rows, "tsv_bytes": size,
                                  "wall_s": round(wall[r][-1], 4)}), flush=True)
        for r in runs:
            print(json.dumps({"e2e_summary": r[0], "cutoff": r[1], "wall_s_median": round(float(np.median(wall[r])), 4),
                              "wall_s_min": round(min(wall[r]), 4), "wall_s_max": round(max(wall[r]), 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="450000,45000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=0)
    ap.add_argument("--index", default=None)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("cut_times: no GPU visible (there is nothing to time without one)")
    if a.sizes:
        kernel_times([int(s) for s in a.sizes.split(",") if s], a.reps)
    if a.e2e:
        end_to_end(a.e2e, a.index)
