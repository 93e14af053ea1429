"""Engine paths that only the shrunken shapes compared with a reference, run on the FULL-size BASELINE configs and checked
edge for edge by tests/pair_probe.check_edge_set against the pair matrix of the keys (all N row sums, two random probes).
Every config is generated and grouped once (pair_probe.config) and shared by the tests that follow one another.

  * weighted postings (ksp_pairwise_postings_host, per-key weights in [1, 1000]) on C4 and C5: weighted 64-bit tags at
    10^6 sources, the weighted 32-bit-counter join with C4's ~10^6-hash bins;
  * unweighted postings on C3 (the input shape of the drop-in's colour index);
  * several engines on one card: C3 through ksp_pairwise_host on devices [0, 0] (hash-range slices, device-to-device
    exchange, assembly), C5 through the postings entry on [0, 0, 0] (tile-range shards);
  * forced modes (the env knobs tests/test_fuzz_gpu.py sweeps on small shapes), each shown by stats() or the build's
    phases to have run:
      C3: KSP_REORDER=0, KSP_SEG=0, KSP_JOIN=matches, KSP_JOIN=window, KSP_KEY_GROUPS=0, KSP_COLLECT=0 / 1;
      C4: KSP_MS=1024 (its 391+ blocks take the split's 1 024-block tables), KSP_JOIN=matches;
      C2: KSP_FUSED=1 (bucket-resident stage 1, which only engages up to 256 blocks: C2's 79).
    Left out: KSP_MS=0 on C3 / C4 (above 256 blocks the library sort is already the default: the knob changes nothing);
    KSP_HASH_GROUP=0 and KSP_ALIGN=0 (nothing in stats() or the phases tells whether they engaged, and the GPU-time
    budget of the suite goes to the modes that can be shown to have run);
  * Engine.join_to_host (the pieces bench.py times for the other configs) on C3 and C5.
"""
import os

import numpy as np
import pytest

from kspider_amd import engine
from pair_probe import check_edge_set, config, key_index, sort_edges
from test_configs_gpu import _join_all

pytestmark = pytest.mark.gpu

KNOBS = ("KSP_REORDER", "KSP_SEG", "KSP_MS", "KSP_JOIN", "KSP_COLLECT", "KSP_KEY_GROUPS", "KSP_HASH_GROUP", "KSP_ALIGN",
         "KSP_FUSED", "KSP_NO_SCHED", "KSP_PARTITION", "KSP_PART_MIN")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _weights(idx, seed):
    w = np.random.default_rng(seed).integers(1, 1001, idx.keys.size).astype(np.uint32)
    # the documented precondition of weighted postings (include/kspider_amd.h, ksp_engine_build_postings)
    per_source = np.zeros(idx.n_sources, dtype=np.uint64)
    np.add.at(per_source, idx.sources, np.repeat(w.astype(np.uint64), idx.counts))
    assert int(per_source.max()) < (1 << 32), int(per_source.max())
    return w


# ---- C3 -------------------------------------------------------------------------------------------------------------

def _build_and_join(sk, profile=True):
    dk = engine.DeviceBuffer.from_numpy(sk.keys)
    e = engine.Engine(0)
    e.set_profiling(profile)
    e.build_blocks(dk.ptr.value, sk.offsets)
    st = e.stats()
    phases = [p for p, _ in e.phase_times()]
    ev, _ = _join_all(e, int(min(e.edge_bound(0, e.num_tiles), 1 << 26)) + 1)
    st_join = e.stats()
    dk.free()
    e.close()
    return ev, st, st_join, phases


C3_MODES = [
    ({"KSP_REORDER": "0"}, lambda n, st, sj, ph: st["n_blocks"] == (n + 127) // 128),      # caller's order: no spare blocks
    ({"KSP_SEG": "0"}, lambda n, st, sj, ph: st["partition_kind"] == 2 and st["partition_fallback"] == 0),   # paged partition
    ({"KSP_JOIN": "matches"}, lambda n, st, sj, ph: sj["n_match_records"] > 0),
    ({"KSP_JOIN": "window"}, lambda n, st, sj, ph: sj["n_match_records"] == 0),
    ({"KSP_KEY_GROUPS": "0"}, lambda n, st, sj, ph: "key groups" not in ph),                  # block lists sorted by block
    ({"KSP_COLLECT": "0"}, lambda n, st, sj, ph: st["weighted"] == 0),
    ({"KSP_COLLECT": "1"}, lambda n, st, sj, ph: st["weighted"] == 0),
]


@pytest.mark.parametrize("env,ran", C3_MODES, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in C3_MODES])
def test_c3_forced_modes(env, ran, monkeypatch):
    sk, idx = config("C3")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ev, st, st_join, phases = _build_and_join(sk)
    assert ran(sk.n_sources, st, st_join, phases), (env, st, st_join, phases)
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=303)


def test_c3_unweighted_postings():
    sk, idx = config("C3")
    key_off, sources = idx.postings
    ev, st = engine.pairwise_postings_host(key_off, sources, None, sk.n_sources)
    assert st["n_sources"] == sk.n_sources and st["partition_kind"] == 0 and st["weighted"] == 0, st
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=303)


def test_c3_two_engines_on_one_card():
    """Hash-range slices built by two engines on device 0, exchanged and assembled, tile ranges joined by both."""
    sk, idx = config("C3")
    ev, st = engine.pairwise_host(sk.keys, sk.offsets, devices=[0, 0])
    assert st["n_sources"] == sk.n_sources and st["n_entries"] == int(sk.offsets[-1]), st
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=303)


def _join_to_host(sk):
    dk = engine.DeviceBuffer.from_numpy(sk.keys)
    e = engine.Engine(0)
    e.build_blocks(dk.ptr.value, sk.offsets)
    T = e.num_tiles
    cap = int(e.edge_bound(0, T)) + 1
    host = np.empty(cap, dtype=engine.EDGE_DTYPE)    # (pages past the edge count are never touched)
    m = e.join_to_host(0, T, host.ctypes.data, cap)
    st = e.stats()
    dk.free()
    e.close()
    return sort_edges(host[:m]), st


def test_c3_join_to_host():
    sk, idx = config("C3")
    ev, st = _join_to_host(sk)
    assert st["n_sources"] == sk.n_sources, st
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=303)


# ---- C4 -------------------------------------------------------------------------------------------------------------

C4_MODES = [
    ({"KSP_MS": "1024"}, lambda n, st, sj, ph: 256 < st["n_blocks"] <= 1024),   # the split's 1 024-block tables
    ({"KSP_JOIN": "matches"}, lambda n, st, sj, ph: sj["n_match_records"] > 0),
]


@pytest.mark.parametrize("env,ran", C4_MODES, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m, _ in C4_MODES])
def test_c4_forced_modes(env, ran, monkeypatch):
    sk, idx = config("C4")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ev, st, st_join, phases = _build_and_join(sk)
    assert ran(sk.n_sources, st, st_join, phases), (env, st, st_join, phases)
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=404)


def test_c4_weighted_postings():
    sk, idx = config("C4")
    w = _weights(idx, 44)
    key_off, sources = idx.postings
    ev, st = engine.pairwise_postings_host(key_off, sources, w, sk.n_sources)
    assert st["weighted"] == 1 and st["partition_kind"] == 0, st
    check_edge_set(ev, idx, sk.n_sources, w=w, probes=2, seed=404)


# ---- C5 -------------------------------------------------------------------------------------------------------------

def test_c5_weighted_postings():
    sk, idx = config("C5")
    w = _weights(idx, 55)
    key_off, sources = idx.postings
    ev, st = engine.pairwise_postings_host(key_off, sources, w, sk.n_sources)
    assert st["weighted"] == 1 and st["partition_kind"] == 0, st
    check_edge_set(ev, idx, sk.n_sources, w=w, probes=2, seed=505)


def test_c5_three_engines_on_one_card_postings():
    """The postings entry on devices [0, 0, 0]: three engines each join a tile-range shard."""
    sk, idx = config("C5")
    key_off, sources = idx.postings
    ev, st = engine.pairwise_postings_host(key_off, sources, None, sk.n_sources, devices=[0, 0, 0])
    assert st["n_sources"] == sk.n_sources, st
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=505)


def test_c5_join_to_host():
    sk, idx = config("C5")
    ev, st = _join_to_host(sk)
    assert st["n_sources"] == sk.n_sources, st
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=505)


# ---- C2 -------------------------------------------------------------------------------------------------------------

def test_c2_bucket_resident_stage1(monkeypatch):
    """KSP_FUSED=1 at full C2 size: the bucket-resident stage 1 engages (stage1_kind 1) and gives the whole edge set."""
    sk, idx = config("C2")
    monkeypatch.setenv("KSP_FUSED", "1")
    ev, st, st_join, _ = _build_and_join(sk, profile=False)
    assert st["stage1_kind"] == 1 and st["partition_kind"] == 3 and st["partition_fallback"] == 0, st
    check_edge_set(ev, idx, sk.n_sources, probes=2, seed=202)
