"""Counted sketches on the GPU (csrc/sketcher.hip: ksp_sketch_host_abund / ksp_sketch_device_abund) against the host loop
ksp_sketch_cpu_abund — which tests/test_sketch_abund_cpu.py holds against the restatement —, compared with ==, on the inputs of
tests/sketch_abund_restate.py: one hash very often, a k-mer and its reverse complement, abutting sources, a run of equal survivors
that comes from two tiles, the overflow retry, one-word and two-word k-mers."""
import numpy as np
import pytest

import sketch_abund_restate as A
import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

pytestmark = pytest.mark.gpu
FULL = 2**64 - 1
GUARD64, GUARD32 = 0xD15EA5ED0DDBA11, 0xA5A5A5A5


def _same(case, k, max_hash=FULL):
    keys, abund, off, st = engine.sketch_host_abund(case.seq, case.offsets, k, max_hash=max_hash)
    want_keys, want_abund, want_off = engine.sketch_cpu_abund(case.seq, case.offsets, k, max_hash=max_hash)
    assert (off == want_off).all() and (keys == want_keys).all() and (abund == want_abund).all(), (case.name, k)
    plain, plain_off, plain_st = engine.sketch_host(case.seq, case.offsets, k, max_hash=max_hash)       # the keys are the unweighted call's
    assert (plain == keys).all() and (plain_off == off).all()
    assert st["kept"] == plain_st["kept"] == int(abund.astype(np.uint64).sum()) and st["distinct_out"] == keys.size
    return keys, abund, off, st


@pytest.mark.parametrize("k", [21, 31, 33, 64])
def test_one_hash_very_often(k):
    keys, abund, _, _ = _same(A.homopolymer(k, 9000), k)          # over two tile edges
    assert keys.tolist() == [R.kmer_hash("A" * k)] and abund.tolist() == [9000 - k + 1]


@pytest.mark.parametrize("k", [1, 21, 31, 32, 33, 51, 64])
def test_against_the_host_loop(k):
    """k = 31 and k > 32; a k-mer and its reverse complement in one source; two abutting sources that share a k-mer — the counts
    stay per source; reads at depths 1, 6 and 25 as one source and cut into three"""
    keys, abund, _, _ = _same(A.mirror(k), k)
    if k % 2:
        assert abund.tolist() == [3]
    keys, abund, off, _ = _same(A.abutting(k), k)
    if k > 10:
        shared = R.kmer_hash(A.abutting(k).seq[:k].decode())
        first, second = keys[:int(off[1])].tolist(), keys[int(off[1]):].tolist()
        assert abund[first.index(shared)] == 2 and abund[int(off[1]) + second.index(shared)] == 1
    for case in A.reads():
        for mh in (FULL, R.max_hash_of(4)):
            _same(case, k, mh)
    _same(I.mixed(), k)


@pytest.mark.parametrize("cap", [None, "1", "2"])
def test_a_repeat_over_the_tile_edge(monkeypatch, cap):
    """The same few hashes on both sides of the boundary between two tiles, hashed by one workgroup after the other
    (KSPIDER_SKETCH_MAX_WGS=1), by two, and by one per tile"""
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    for k in (21, 40):
        _, abund, _, st = _same(A.repeat_over_tile_edge(k), k)
        assert (abund > 20).sum() == 7 and st["workgroups"] == (int(cap) if cap else 3)


def test_overflow_retry_size_query_and_guards(monkeypatch):
    one, three = A.reads()
    k = 21
    want_keys, want_abund, want_off = engine.sketch_cpu_abund(three.seq, three.offsets, k, max_hash=FULL)
    seq = np.zeros(len(three.seq) + 16, dtype=np.uint8)
    seq[:len(three.seq)] = np.frombuffer(three.seq, dtype=np.uint8)
    d_seq = engine.DeviceBuffer.from_numpy(seq)
    rc, _, st = engine.sketch_device_abund(d_seq.ptr.value, len(three.seq), three.offsets, k, FULL, 0, 0, 0)      # the size query
    assert rc == engine.KSP_E_OVERFLOW
    needed = st["needed"]
    assert needed == int(want_abund.astype(np.uint64).sum()) > want_keys.size
    rc, _, st_plain = engine.sketch_device(d_seq.ptr.value, len(three.seq), three.offsets, k, FULL, 0, 0)
    assert st_plain["needed"] == needed
    for capacity in (needed - 1, needed):
        d_keys = engine.DeviceBuffer.from_numpy(np.full(capacity + 8, GUARD64, dtype=np.uint64))
        d_abund = engine.DeviceBuffer.from_numpy(np.full(capacity + 8, GUARD32, dtype=np.uint32))
        rc, off, st = engine.sketch_device_abund(d_seq.ptr.value, len(three.seq), three.offsets, k, FULL, d_keys.ptr.value, d_abund.ptr.value, capacity)
        got, got_a = d_keys.to_numpy(np.uint64, capacity + 8), d_abund.to_numpy(np.uint32, capacity + 8)
        d_keys.free()
        d_abund.free()
        assert st["needed"] == needed
        if capacity < needed:
            assert rc == engine.KSP_E_OVERFLOW and "survivors" in engine.lib().ksp_last_error().decode()
            assert (got == GUARD64).all() and (got_a == GUARD32).all()                     # nothing at all was written
        else:
            n = want_keys.size
            assert rc == engine.KSP_OK and (off == want_off).all()
            assert (got[:n] == want_keys).all() and (got_a[:n] == want_abund).all() and (got[capacity:] == GUARD64).all() and (got_a[capacity:] == GUARD32).all()
    d_keys = engine.DeviceBuffer(64)
    with pytest.raises(engine.KspError) as ei:                                             # the counts missing with a capacity
        engine.sketch_device_abund(d_seq.ptr.value, len(three.seq), three.offsets, k, FULL, d_keys.ptr.value, 0, 4)
    assert ei.value.code == engine.KSP_E_ARG and "ksp_sketch_device_abund: d_out_abund is NULL" in str(ei.value)
    d_keys.free()
    d_seq.free()
    # the host call retries at the exact size
    monkeypatch.setenv("KSPIDER_SKETCH_FIRST_CAPACITY", str(needed - 1))
    keys, abund, off, st = engine.sketch_host_abund(three.seq, three.offsets, k, max_hash=FULL)
    assert st["retries"] == 1 and (keys == want_keys).all() and (abund == want_abund).all() and (off == want_off).all()
    monkeypatch.setenv("KSPIDER_SKETCH_FIRST_CAPACITY", str(needed))
    keys, abund, off, st = engine.sketch_host_abund(three.seq, three.offsets, k, max_hash=FULL)
    assert st["retries"] == 0 and (keys == want_keys).all() and (abund == want_abund).all()
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_host_abund(one.seq, one.offsets, k, max_hash=FULL, device=99)
    assert ei.value.code == engine.KSP_E_HIP and "ksp_sketch_host_abund: no such device" in str(ei.value)
