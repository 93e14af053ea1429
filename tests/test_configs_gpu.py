"""Every BASELINE.json configuration at FULL size through the HIP engine on one MI355X.

  configs[0] C1   1 000 "FASTA" seqs x 980 hashes, H_max = 4^21   bit-exact: TSV bytes == oracle.ref_pairwise
                                                                  (src/pairwise.cpp:123-276 restated) and the
                                                                  edge set == brute-force |A n B|
  configs[1] C2  10 000 signatures (the bench workload)           bit-exact: full edge set == oracle.accumulate_mem
                                                                  (src/pairwise.cpp:194-237 restated)
  configs[2] C3 100 000 genomes, 5.0e8 hashes                     size-independent properties (below)
  configs[3] C4  50 000 bins, lognormal sizes up to ~1e6          size-independent properties
  configs[4] C5 1 000 000 read groups, <= 294 hashes              size-independent properties

Properties at the sizes the oracle cannot reach (what /root/reference/test/validate.py:100-108 checks per
key, restated so that it is independent of the size), from a host-side key index (tests/pair_probe.py):
  * sum of all shared counts == sum_k C(holders_k, 2) from an independent host-side inverted index;
  * every edge has source_1 < source_2 < N, no pair twice, shared >= 1, shared <= min(n_a, n_b);
  * COMPLETE ROWS of 300 sampled sources: sum_b shared(a, b) == sum_{k in K(a)} (holders_k - 1);
  * 300 sampled reported pairs and 300 sampled absent pairs by direct set intersection.
and the whole edge set by tests/pair_probe.check_edge_set: all N row sums and two random probes u^T S v of the pair
matrix, computed from the keys alone (an error that keeps the total and every row sum is caught too).
These runs reach the code the shrunken cases do not: > 2^32-thread launch chunking, the cell-index clamp,
T > 2^26 tiles (no work list), 32-bit tags above 65 536 sources, C4's ~10^6-hash sketch in the
32-bit-counter instantiation of the join.
"""
import os

import numpy as np
import pytest

from kspider_amd import engine, synth
from pair_probe import check_edge_set, config

pytestmark = pytest.mark.gpu


def _join_all(e, cap):
    """Every tile of a built engine; tile ranges are halved when the edge buffer overflows."""
    T = e.num_tiles
    de = engine.DeviceBuffer(cap * 16)
    parts, t0, step = [], 0, max(T, 1)
    while t0 < T:
        t1 = min(T, t0 + step)
        try:
            cnt = e.join(t0, t1, de.ptr.value, cap)
        except engine.KspError as ex:
            if ex.code != engine.KSP_E_OVERFLOW or t1 - t0 <= 1:
                raise
            step = (t1 - t0) // 2
            continue
        if cnt:
            parts.append(de.to_numpy(engine.EDGE_DTYPE, cnt))
        t0 = t1
    de.free()
    ev = np.concatenate(parts) if parts else np.zeros(0, dtype=engine.EDGE_DTYPE)
    key = ev["source_1"].astype(np.int64) * (1 << 32) + ev["source_2"].astype(np.int64)
    o = np.argsort(key, kind="stable")
    return ev[o], key[o]


def _properties(sk, idx, ev, key, seed):
    n = sk.n_sources
    sizes = sk.sizes
    assert len(ev) > 0
    assert (ev["source_1"] < ev["source_2"]).all() and int(ev["source_2"].max()) < n
    assert (np.diff(key) > 0).all()                       # sorted, and no pair twice
    assert (ev["shared"] > 0).all()
    assert (ev["shared"] <= np.minimum(sizes[ev["source_1"]], sizes[ev["source_2"]])).all()
    # independent inverted index on the host: every key held by m sources contributes C(m, 2) (keys held once: 0)
    counts = idx.counts
    assert int(ev["shared"].sum(dtype=np.uint64)) == int((counts * (counts - 1) // 2).sum())
    # complete rows of sampled sources
    row = np.bincount(ev["source_1"], weights=ev["shared"].astype(np.float64), minlength=n)
    row += np.bincount(ev["source_2"], weights=ev["shared"].astype(np.float64), minlength=n)
    rng = np.random.default_rng(seed)
    for a in rng.choice(n, size=300, replace=False):
        want = int((idx.holders_of(sk.run(int(a))) - 1).sum())
        assert int(row[a]) == want, f"row sum of source {a}"
    # sampled reported pairs / sampled absent pairs by direct intersection
    for i in rng.choice(len(ev), size=min(300, len(ev)), replace=False):
        a, b, s = int(ev["source_1"][i]), int(ev["source_2"][i]), int(ev["shared"][i])
        assert np.intersect1d(sk.run(a), sk.run(b), assume_unique=True).size == s
    absent = 0
    while absent < 300:
        a, b = sorted(rng.choice(n, size=2, replace=False).tolist())
        k = a * (1 << 32) + b
        j = int(np.searchsorted(key, k))
        if j < len(key) and key[j] == k:
            continue
        assert np.intersect1d(sk.run(a), sk.run(b), assume_unique=True).size == 0
        absent += 1
    # the whole edge set: all N rows, two random probes of the pair matrix
    check_edge_set(ev, idx, n, probes=2, seed=seed)


def test_c1_full_size_bit_exact(oracle_lib, tmp_path):
    """configs[0]: TSV bytes of the drop-in == the restated reference; edge set == brute force."""
    sk = synth.generate("C1")
    assert sk.n_sources == 1000
    edges, st = engine.pairwise_host(sk.keys, sk.offsets)
    ref = oracle_lib.brute_pairs(sk.keys, sk.offsets)
    assert len(edges) == len(ref) and (edges == ref).all()
    prefix = str(tmp_path / "c1")
    oracle_lib.index_from_sketches(prefix, sk.keys, sk.offsets)
    oracle_lib.ref_pairwise(prefix, 4)
    want_pw = open(prefix + "_kSpider_pairwise.tsv", "rb").read()
    want_sk = open(prefix + "_kSpider_seqToKmersNo.tsv", "rb").read()
    os.remove(prefix + "_kSpider_pairwise.tsv")
    os.remove(prefix + "_kSpider_seqToKmersNo.tsv")
    engine.pairwise(prefix, 4)
    assert open(prefix + "_kSpider_pairwise.tsv", "rb").read() == want_pw
    assert open(prefix + "_kSpider_seqToKmersNo.tsv", "rb").read() == want_sk
    assert want_pw.count(b"\n") == len(ref) + 1


def test_c2_full_size_edge_set_equals_restated_reference(oracle_lib):
    """configs[1], the bench workload: the FULL edge set against the restated reference accumulation
    (inverted-index walk + sharded pair map), not a sample."""
    sk = synth.generate("C2")
    assert sk.n_sources == 10000
    co, src, w = oracle_lib.build_colors(sk.keys, sk.offsets)           # group IDs = index + 1
    threads = max(1, min(32, len(os.sched_getaffinity(0))))
    _, n_edges, _, ref = oracle_lib.accumulate_mem(co, src, w, threads)
    ref = np.sort(ref, order=["source_1", "source_2"])
    dk = engine.DeviceBuffer.from_numpy(sk.keys)
    e = engine.Engine(0)
    e.build_blocks(dk.ptr.value, sk.offsets)
    st = e.stats()
    assert st["partition_kind"] == 3 and st["partition_fallback"] == 0, st   # the segment partition (level 1 read off the sorted runs), no fallback
    ev, _ = _join_all(e, int(e.edge_bound(0, e.num_tiles)) + 1)
    assert len(ev) == n_edges == len(ref)
    assert (ev["source_1"] + 1 == ref["source_1"]).all() and (ev["source_2"] + 1 == ref["source_2"]).all()
    assert (ev["shared"] == ref["shared"]).all()
    # and through the host-buffer convenience entry (H2D + both stages + D2H, sorted)
    edges, _ = engine.pairwise_host(sk.keys, sk.offsets)
    assert (edges == ev).all()


@pytest.mark.parametrize("cfg,n", [("C3", 100_000), ("C4", 50_000), ("C5", 1_000_000)])
def test_full_size_properties(cfg, n):
    """configs[2..4] at the sizes BASELINE.json names."""
    sk, idx = config(cfg)
    assert sk.n_sources == n
    dk = engine.DeviceBuffer.from_numpy(sk.keys)
    e = engine.Engine(0)
    e.build_blocks(dk.ptr.value, sk.offsets)
    st = e.stats()
    assert st["n_sources"] == n and st["n_entries"] == int(sk.offsets[-1])
    ev, key = _join_all(e, int(min(e.edge_bound(0, e.num_tiles), 1 << 26)) + 1)
    _properties(sk, idx, ev, key, seed=100 + synth.CONFIGS[cfg]["idx"])
    dk.free()
    e.close()
