#!/usr/bin/env python3
"""Times of the pairwise TSV's row text, made on the device against made by the host's writer threads:
    python tools/tsv_times.py [--sizes 450000,45000000] [--reps 7] [--threads 16] [--nodes 100000]
    python tools/tsv_times.py --sizes "" --e2e 10000 [--index PREFIX] [--other-lib PATH/libkspider_amd.so] [--rounds 6]

--sizes: for every size, that many valid seeded records are made ON THE DEVICE (ksp_debug_tsv_records): ends a < b among --nodes
sources whose ids are index + 1, k-mer counts of 10^3 .. 10^6, a shared count between 1 and the smaller of the two counts,
source_1 ascending.  ksp_debug_tsv_times (csrc/engine_internal.h) then runs, alternating from round to round after
one warm-up of each,
    device   the count, scan and write kernels and the copy of the text to pinned host memory (ksp_edges_tsv without its last
             memcpy); the kernels' own time by HIP events is reported separately
    host     the copy of the records to pinned host memory and the host writer's formatting with --threads threads
Neither writes a file: only what differs between the two writers is timed.  One JSON line per variant: median, minimum and
maximum over the rounds, the bytes of text, and the rates.

--e2e N: the wall time of kspider_pairwise on a C2 index of N sources (or the index at --index) with KSPIDER_TSV unset and
set to "device", and — with --other-lib — of another build's kspider_pairwise (the parent commit's), alternated in one
series; the three TSVs are compared."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kspider_amd import engine, synth  # noqa: E402

NAMES = ("device", "host")


def device_records(n, n_nodes, seed):
    """(records, counts, ids) in device memory, made there (ksp_debug_tsv_records)."""
    rec, counts, ids = engine.DeviceBuffer(16 * n), engine.DeviceBuffer(4 * n_nodes), engine.DeviceBuffer(4 * n_nodes)
    engine.tsv_records(n_nodes, n, seed, rec.ptr.value, counts.ptr.value, ids.ptr.value)
    return rec, counts, ids


def writer_times(sizes, reps, threads, n_nodes):
    for n in sizes:
        rec, counts, ids = device_records(n, n_nodes, seed=n)
        args = (n_nodes, rec.ptr.value, n, counts.ptr.value, ids.ptr.value)
        text_bytes = engine.edges_tsv_size(*args)
        if n <= 1 << 20:                                           # the two writers agree (small sizes: the whole text)
            import tsv_inputs as ti
            e = rec.to_numpy(engine.EDGE_DTYPE, n)
            assert (e["source_1"] < e["source_2"]).all() and (np.diff(e["source_1"].astype(np.int64)) >= 0).all()
            assert engine.edges_tsv(*args) == ti.rows_text(e, counts.to_numpy(np.uint32, n_nodes), ids.to_numpy(np.uint32, n_nodes))
        for w in range(2):                                         # warm-up: code objects, pinned allocations, the page cache
            engine.tsv_times(*args, w, 1, threads)
        ms = {w: [] for w in range(2)}
        for _ in range(reps):                                      # alternating: one run of each per round
            for w in range(2):
                ms[w].append(engine.tsv_times(*args, w, 1, threads)[0])
        for w in range(2):
            t = np.array(ms[w], dtype=np.float64)
            wall, part = t[:, 0], t[:, 1]
            line = {"records": n, "nodes": n_nodes, "writer": NAMES[w], "rounds_timed": reps, "text_bytes": text_bytes,
                    "bytes_per_row": round(text_bytes / n, 2),
                    "ms_median": round(float(np.median(wall)), 3), "ms_min": round(float(wall.min()), 3), "ms_max": round(float(wall.max()), 3)}
            if w == 0:
                rest = wall - part                                 # what is not kernel: the copies of the text, the pinned buffers
                line.update({"kernels_ms_median": round(float(np.median(part)), 3), "kernels_ms_min": round(float(part.min()), 3),
                             "kernels_ms_max": round(float(part.max()), 3),
                             # twice 16 bytes read per row (count pass, write pass) and the text written once
                             "kernels_GBps": round((32 * n + text_bytes) / float(np.median(part)) / 1e6, 1),
                             "copy_and_rest_ms_median": round(float(np.median(rest)), 3),
                             "text_out_GBps": round(text_bytes / float(np.median(rest)) / 1e6, 2)})
            else:
                line.update({"threads": threads, "copy_ms_median": round(float(np.median(part)), 3),
                             "records_out_GBps": round(16 * n / float(np.median(part)) / 1e6, 2),
                             "format_ms_median": round(float(np.median(wall - part)), 3)})
            print(json.dumps(line), flush=True)
        t0, t1 = float(np.median(np.array(ms[0])[:, 0])), float(np.median(np.array(ms[1])[:, 0]))
        print(json.dumps({"records": n, "host_over_device": round(t1 / t0, 2)}), flush=True)
        for buf in (rec, counts, ids):
            buf.free()


def end_to_end(n_sources, index, other_lib, rounds, threads):
    with tempfile.TemporaryDirectory() as d:
        prefix = index or os.path.join(d, "ix")
        if not os.path.exists(prefix + "_color_to_sources.bin"):
            import oracle
            sk = synth.generate("C2", n_sources=n_sources)
            oracle.index_from_sketches(prefix, sk.keys, sk.offsets)
        L = engine.lib()
        other = ctypes.CDLL(other_lib) if other_lib else None
        tsv = prefix + "_kSpider_pairwise.tsv"

        def run(which):
            os.environ.pop("KSPIDER_TSV", None)
            if which == "device":
                os.environ["KSPIDER_TSV"] = "device"
            t0 = time.perf_counter()
            rc = (other if which == "other" else L).kspider_pairwise(os.fsencode(prefix), threads)
            wall = time.perf_counter() - t0
            os.environ.pop("KSPIDER_TSV", None)
            if rc:
                raise SystemExit(f"kspider_pairwise ({which}) failed: {rc}")
            with open(tsv, "rb") as f:
                return wall, f.read()

        os.environ["KSPIDER_VERBOSE"] = "1"
        runs = ["host", "device"] + (["other"] if other else [])
        texts = {r: run(r)[1] for r in runs}                       # warm-up, and the files agree
        assert all(t == texts["host"] for t in texts.values()), "the TSVs differ"
        wall = {r: [] for r in runs}
        for _ in range(rounds):
            for r in runs:
                wall[r].append(run(r)[0])
        for r in runs:
            print(json.dumps({"e2e": "kspider_pairwise", "writer": r, "sources": n_sources, "rows": texts["host"].count(b"\n") - 1,
                              "tsv_bytes": len(texts["host"]), "threads": threads, "rounds_timed": rounds,
                              "wall_s_median": round(float(np.median(wall[r])), 4), "wall_s_min": round(min(wall[r]), 4),
                              "wall_s_max": round(max(wall[r]), 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="450000,45000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=100000)
    ap.add_argument("--e2e", type=int, default=0)
    ap.add_argument("--index", default=None)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("tsv_times: no GPU visible (there is nothing to time without one)")
    if a.sizes:
        writer_times([int(s) for s in a.sizes.split(",") if s], a.reps, a.threads, a.nodes)
    if a.e2e:
        end_to_end(a.e2e, a.index, a.other_lib, a.rounds, a.threads)
