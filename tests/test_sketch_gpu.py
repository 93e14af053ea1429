"""The device part of the sketcher (csrc/sketcher.hip: ksp_sketch_device / ksp_sketch_host) against the restatement of the
definition (tests/sketch_restate.py) on the inputs of tests/sketch_inputs.py: every ksize, the tile edges with grids that make
every workgroup loop, source boundaries, many short records, the threshold at an exact value, duplicates, overflow."""
import functools

import numpy as np
import pytest

import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

pytestmark = pytest.mark.gpu

FULL = 2**64 - 1
GUARD = 0xD15EA5ED0DDBA11


@functools.lru_cache(maxsize=None)
def _mixed():
    return I.mixed()


@functools.lru_cache(maxsize=None)
def _edge_cases(k):
    """The tile-edge and boundary cases of a ksize with their restated sketches, made once."""
    cases = I.tile_edges(k) + I.boundaries(k)
    return [(c, R.flat(R.sketch(c.seq, c.offsets, k, FULL))) for c in cases]


def _same(case, k, max_hash=FULL, want=None):
    keys, off, st = engine.sketch_host(case.seq, case.offsets, k, max_hash=max_hash)
    want_keys, want_off = want if want is not None else R.flat(R.sketch(case.seq, case.offsets, k, max_hash))
    assert (off == want_off).all(), (case.name, k)
    assert (keys == want_keys).all(), (case.name, k)
    assert st["distinct_out"] == keys.size and st["kept"] == st["needed"] >= keys.size
    assert st["bases"] == sum(chr(b) in R.BASES for b in case.seq)
    return keys, off, st


@pytest.mark.parametrize("k", range(1, 65))
def test_every_ksize(k):
    """About 3 000 bytes with N, lower case and other break bytes, everything kept: all 15 tail lengths, zero to four body blocks,
    one-word and two-word k-mers."""
    c = _mixed()
    _, _, st = _same(c, k)
    assert st["valid_kmers"] == len(R.source_kmers(c.seq, k))   # the stream as one source: the windows without a break byte


@pytest.mark.parametrize("cap", [None, "1", "3"])
@pytest.mark.parametrize("k", [1, 31, 32, 33, 64])
def test_tile_edges_and_source_boundaries(monkeypatch, k, cap):
    """Sources of T - 1, T, T + 1, T + k - 1 and 2T + 1 bases without and with a break byte at T - 1, T and T + k - 2; a source
    boundary on and beside a tile edge, a source shorter than ksize, empty sources first, last and in the middle.  With a grid
    of 1 and of 3 every workgroup loops over tiles."""
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    for case, want in _edge_cases(k):
        _, _, st = _same(case, k, want=want)
        tiles = -(-len(case.seq) // I.TILE)
        assert st["workgroups"] == (min(int(cap), tiles) if cap else tiles)


@pytest.mark.parametrize("k", [21, 31, 51])
def test_no_kmer_crosses_a_source_boundary(k):
    c = I.junction(k)
    keys, off, st = _same(c, k)
    one = R.sketch(c.seq, [0, len(c.seq)], k, FULL)[0]   # as one source the junction's k-mers are there
    assert len(one) == keys.size + (k - 1)
    assert st["valid_kmers"] == len(c.seq) - k + 1 and st["kept"] == st["valid_kmers"] - (k - 1)


def test_many_short_records():
    one, many = I.short_reads()
    mh = R.max_hash_of(8)
    a, _, _ = _same(one, 21, mh)
    b, off, _ = _same(many, 21, mh)
    assert off.size == 2001 and set(a.tolist()) == set(b.tolist())
    _same(many, 64, FULL)


def test_threshold_is_inclusive():
    c = _mixed()
    hashes = sorted({h for run in R.sketch(c.seq, c.offsets, 21, FULL) for h in run})
    m = hashes[len(hashes) // 2]
    at, _, _ = _same(c, 21, m)
    below, _, _ = _same(c, 21, m - 1)
    assert m in at.tolist() and m not in below.tolist()
    assert set(at.tolist()) - set(below.tolist()) == {m}
    nothing, off, st = _same(c, 21, 0)
    assert nothing.size == 0 and not off.any() and st["kept"] == 0


@pytest.mark.parametrize("k", [1, 21, 40])
def test_duplicates(k):
    twice, shared, mirror = I.duplicates(k)
    keys, off, st = _same(twice, k)
    assert st["kept"] == 2 * (400 - k + 1) and keys.size <= 400 - k + 1
    keys, off, _ = _same(shared, k)
    assert (keys[:int(off[1])] == keys[int(off[1]):]).all() and off[1] > 0
    keys, off, _ = _same(mirror, k)
    assert (keys[:int(off[1])] == keys[int(off[1]):]).all() and off[1] > 0
    if k % 2 == 0:
        _same(I.palindrome(k)[0], k)
    _same(I.ordered_pair(k)[0], k)


def test_overflow_reports_the_exact_size_and_leaves_the_guards(monkeypatch):
    c = _mixed()
    k = 21
    want_keys, want_off = R.flat(R.sketch(c.seq, c.offsets, k, FULL))
    seq = np.zeros(len(c.seq) + 16, dtype=np.uint8)
    seq[:len(c.seq)] = np.frombuffer(c.seq, dtype=np.uint8)
    d_seq = engine.DeviceBuffer.from_numpy(seq)
    rc, _, st = engine.sketch_device(d_seq.ptr.value, len(c.seq), c.offsets, k, FULL, 0, 0)       # the size query
    assert rc == engine.KSP_E_OVERFLOW
    needed = st["needed"]
    # the survivors are the k-mers of the sources, repeats included; the keys are the distinct ones
    assert needed == sum(len(R.source_kmers(c.seq[c.offsets[s]:c.offsets[s + 1]], k)) for s in range(3)) >= want_keys.size > 0
    for capacity in (needed - 1, needed):
        room = np.full(capacity + 8, GUARD, dtype=np.uint64)
        d_keys = engine.DeviceBuffer.from_numpy(room)
        rc, off, st = engine.sketch_device(d_seq.ptr.value, len(c.seq), c.offsets, k, FULL, d_keys.ptr.value, capacity)
        got = d_keys.to_numpy(np.uint64, capacity + 8)
        d_keys.free()
        assert st["needed"] == needed
        if capacity < needed:
            assert rc == engine.KSP_E_OVERFLOW and "survivors" in engine.lib().ksp_last_error().decode()
            assert (got == GUARD).all()                     # nothing at all was written
        else:
            assert rc == engine.KSP_OK and (off == want_off).all()
            assert (got[:want_keys.size] == want_keys).all() and (got[capacity:] == GUARD).all()
    d_seq.free()
    # the host call retries at the exact size
    monkeypatch.setenv("KSPIDER_SKETCH_FIRST_CAPACITY", str(needed - 1))
    keys, off, st = engine.sketch_host(c.seq, c.offsets, k, max_hash=FULL)
    assert st["retries"] == 1 and (keys == want_keys).all() and (off == want_off).all()
    monkeypatch.setenv("KSPIDER_SKETCH_FIRST_CAPACITY", str(needed))
    keys, off, st = engine.sketch_host(c.seq, c.offsets, k, max_hash=FULL)
    assert st["retries"] == 0 and (keys == want_keys).all()


@pytest.mark.parametrize("k", [21, 31, 51])
def test_generic_switch_changes_nothing(monkeypatch, k):
    """There is one runtime-ksize path and no specialisation; KSPIDER_SKETCH_GENERIC=1 must give the same keys all the same."""
    c = _mixed()
    a, off_a, _ = _same(c, k, R.max_hash_of(2))
    monkeypatch.setenv("KSPIDER_SKETCH_GENERIC", "1")
    b, off_b, _ = _same(c, k, R.max_hash_of(2))
    assert (a == b).all() and (off_a == off_b).all()


def test_refusals():
    c = _mixed()
    for bad_k in (0, 65, -3):
        with pytest.raises(engine.KspError) as ei:
            engine.sketch_host(c.seq, c.offsets, bad_k, max_hash=FULL)
        assert ei.value.code == engine.KSP_E_ARG
    for bad in ([0, 2000, 1000, 3000], [1, 1000, 2000, 3000], [0, 1000, 2000, 2999], [0]):
        with pytest.raises(engine.KspError) as ei:
            engine.sketch_host(c.seq, bad, 21, max_hash=FULL)
        assert ei.value.code == engine.KSP_E_ARG
    d_seq = engine.DeviceBuffer(4096)
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_device(d_seq.ptr.value + 4, 100, [0, 100], 21, FULL, 0, 0)
    assert ei.value.code == engine.KSP_E_ARG and "aligned" in str(ei.value)
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_device(d_seq.ptr.value, 100, [0, 100], 21, FULL, 0, 5)
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_host(c.seq, c.offsets, 21, max_hash=FULL, device=99)
    assert ei.value.code == engine.KSP_E_HIP and "no such device" in str(ei.value)
    d_seq.free()
