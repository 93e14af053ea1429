#!/usr/bin/env python3
"""HIP-event times of the sketcher against the host loop and against the one-byte-per-base floor:
    python tools/sketch_times.py [--sources 64] [--mbp 5] [--ksize 31] [--scaled 1000] [--reps 11] [--cpu-sources N]
                                 [--moltype protein|dayhoff|hp [--translate]]
The workload: --sources seeded synthetic sources of --mbp million bases each (uniform ACGT, a newline every 60 000 bases as a
record end).  With the bytes resident in HBM: the size query, two warm-up calls, then --reps calls of ksp_sketch_device; the
medians and the spread (min, max) of ms_hash and ms_select (HIP events) and the bases per second of the hash pass.  The upload
is timed by three calls of ksp_sketch_host (ms_upload, from pageable host memory).  The same bytes — the first --cpu-sources
sources of them, all by default — go through ksp_sketch_cpu on one thread (wall clock); the yardstick is that rate times 16,
the CPUs a GPU job may use.  The floor: one byte per base at the copy rate measured in this run (device-to-device hipMemcpy of
1 GiB, read + write counted).  One JSON line.
With --moltype the same measurement of the protein hash passes: with --translate over the same DNA bytes, --ksize
being the residue k (two hashes per position); without it over a synthetic protein stream of the same byte count (uniform over
the 20 amino acids, the same newlines), through ksp_sketch_device_mol and ksp_sketch_cpu_mol."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kspider_amd import engine  # noqa: E402


def copy_rate(reps):
    """bytes per ms moved by a device-to-device copy (read + write)"""
    L = engine.lib()
    L.ksp_debug_copy_times.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    n = 1 << 30
    ms = (ctypes.c_float * (reps + 2))()
    engine._check(L.ksp_debug_copy_times(0, n, reps + 2, ms))
    return 2 * n / float(np.median(list(ms)[2:]))


def workload(n_sources, bases_each, seed=20260, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    seq = letters[rng.integers(0, len(alphabet), size=n_sources * bases_each, dtype=np.uint8)]
    seq[59999::60000] = ord("\n")
    seq[bases_each - 1::bases_each] = ord("\n")   # (a source ends with its last record's newline)
    offsets = np.arange(n_sources + 1, dtype=np.uint64) * np.uint64(bases_each)
    return seq, offsets


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--ksize", type=int, default=31)
    ap.add_argument("--scaled", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--cpu-sources", type=int, default=None)
    ap.add_argument("--moltype", choices=["dna", "protein", "dayhoff", "hp"], default="dna")
    ap.add_argument("--translate", action="store_true")
    a = ap.parse_args()
    if a.translate and a.moltype == "dna":
        raise SystemExit("sketch_times: --translate takes --moltype protein, dayhoff or hp")
    mol = a.moltype != "dna"
    if engine.device_count() < 1:
        raise SystemExit("sketch_times: no GPU (a time is measured on the device or not at all)")
    each = int(a.mbp * 1e6)
    seq, off = workload(a.sources, each, alphabet=b"ACDEFGHIKLMNPQRSTVWY" if mol and not a.translate else b"ACGT")

    def on_device(d_seq_ptr, d_keys_ptr, capacity):
        if mol:
            return engine.sketch_device_mol(d_seq_ptr, n_bytes, off, a.ksize, a.moltype, a.translate, max_hash, d_keys_ptr, 0, capacity)
        return engine.sketch_device(d_seq_ptr, n_bytes, off, a.ksize, max_hash, d_keys_ptr, capacity)

    max_hash = engine.sketch_max_hash(a.scaled)
    n_bytes = int(seq.size)
    # ---- the device, bytes resident
    padded = np.zeros(n_bytes + 16, dtype=np.uint8)
    padded[:n_bytes] = seq
    d_seq = engine.DeviceBuffer.from_numpy(padded)
    del padded
    rc, _, st = on_device(d_seq.ptr.value, 0, 0)
    capacity = st["needed"]
    d_keys = engine.DeviceBuffer(8 * max(capacity, 1))
    ms_hash, ms_select = [], []
    for r in range(2 + a.reps):
        rc, dev_off, st = on_device(d_seq.ptr.value, d_keys.ptr.value, capacity)
        assert rc == engine.KSP_OK
        if r >= 2:
            ms_hash.append(st["ms_hash"])
            ms_select.append(st["ms_select"])
    dev_keys = d_keys.to_numpy(np.uint64, int(dev_off[-1]))
    d_keys.free()
    d_seq.free()
    ms_upload = []
    for r in range(3):
        _, _, hst = engine.sketch_host_mol(seq, off, a.ksize, a.moltype, a.translate, max_hash=max_hash) if mol else engine.sketch_host(seq, off, a.ksize, max_hash=max_hash)
        ms_upload.append(hst["ms_upload"])
    rate = copy_rate(5)
    # ---- the host loop, one thread
    n_cpu = a.sources if a.cpu_sources is None else min(a.cpu_sources, a.sources)
    cpu_bytes = n_cpu * each
    cpu_keys = np.zeros(max(st["kept"], 1), dtype=np.uint64)   # (the survivors bound the keys: one pass, no size query)
    cpu_off = np.zeros(n_cpu + 1, dtype=np.uint64)
    needed = ctypes.c_uint64(0)
    cpu_seq = np.ascontiguousarray(seq[:cpu_bytes])
    t0 = time.perf_counter()
    if mol:
        engine._check(engine.lib().ksp_sketch_cpu_mol(cpu_seq.ctypes.data, cpu_bytes, off.ctypes.data, n_cpu, a.ksize, engine._moltype(a.moltype),
                                                      engine.SKETCH_TRANSLATE if a.translate else 0, max_hash, 42, cpu_keys.ctypes.data, None, cpu_keys.size, cpu_off.ctypes.data,
                                                      ctypes.byref(needed)))
    else:
        engine._check(engine.lib().ksp_sketch_cpu(cpu_seq.ctypes.data, cpu_bytes, off.ctypes.data, n_cpu, a.ksize, max_hash, 42, cpu_keys.ctypes.data, cpu_keys.size,
                                                  cpu_off.ctypes.data, ctypes.byref(needed)))
    cpu_s = time.perf_counter() - t0
    cpu_keys = cpu_keys[:needed.value]
    same = bool((cpu_off == dev_off[:n_cpu + 1]).all() and (cpu_keys == dev_keys[:cpu_keys.size]).all())
    hash_med = float(np.median(ms_hash))
    out = {
        "workload": {"sources": a.sources, "bases_each": each, "ksize": a.ksize, "scaled": a.scaled, "bytes": n_bytes, "moltype": a.moltype, "translate": a.translate},
        "valid_kmers": st["valid_kmers"], "kept": st["kept"], "distinct_out": st["distinct_out"], "workgroups": st["workgroups"],
        "ms_hash": spread(ms_hash), "ms_select": spread(ms_select), "ms_upload": spread(ms_upload),
        "hash_bases_per_s": n_bytes / (hash_med * 1e-3),
        "floor_ms_one_byte_per_base": n_bytes / rate, "copy_rate_GBps": rate * 1e3 / 1e9,
        "cpu_one_thread": {"sources": n_cpu, "seconds": cpu_s, "bases_per_s": cpu_bytes / cpu_s},
        "cpu_times_16_bases_per_s": 16 * cpu_bytes / cpu_s,
        "hash_over_cpu_times_16": (n_bytes / (hash_med * 1e-3)) / (16 * cpu_bytes / cpu_s),
        "device_equals_cpu": same,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
