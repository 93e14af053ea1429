"""The host side of the sketcher (csrc/sketch_hash.h through csrc/sketch_cpu.cpp) against the restatement of the definition
(tests/sketch_restate.py): Murmur's two published anchors, every input length 0 .. 64, the threshold table, one k-mer's hash, and
ksp_sketch_cpu on every generator of tests/sketch_inputs.py.  No GPU."""
import random

import numpy as np
import pytest

import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

FULL = 2**64 - 1


def _signed(x):
    return x - 2**64 if x >= 2**63 else x


def test_restatement_reproduces_both_anchors():
    assert R.smhasher_verification() == 0x6384BA69
    assert tuple(_signed(h) for h in R.murmur3_x64_128(b"foo", 0)) == (-2129773440516405919, 9128664383759220103)


def test_library_murmur_reproduces_both_anchors():
    out = b""
    for i in range(256):
        h1, h2 = engine.murmur64(bytes(range(i)), 256 - i)
        out += h1.to_bytes(8, "little") + h2.to_bytes(8, "little")
    assert engine.murmur64(out, 0)[0] & 0xFFFFFFFF == 0x6384BA69
    assert tuple(_signed(h) for h in engine.murmur64(b"foo", 0)) == (-2129773440516405919, 9128664383759220103)


def test_library_murmur_equals_restatement_at_every_length():
    rng = random.Random(3)
    for n in range(65):
        for seed in (0, 42, 0xFFFFFFFF):
            data = bytes(rng.randrange(256) for _ in range(n))
            assert engine.murmur64(data, seed) == R.murmur3_x64_128(data, seed), (n, seed)


def test_max_hash_table():
    table = {1: FULL, 1000: 18446744073709552, 2: 9223372036854775808, 10000: 1844674407370955, 100: 184467440737095520, 3: 6148914691236516864}
    for scaled, want in table.items():
        assert engine.sketch_max_hash(scaled) == want == R.max_hash_of(scaled)
    with pytest.raises(engine.KspError) as ei:
        engine.sketch_max_hash(0)
    assert ei.value.code == engine.KSP_E_ARG


@pytest.mark.parametrize("k", range(1, 65))
def test_kmer_hash(k):
    rng = random.Random(100 + k)
    for _ in range(8):
        x = I.bases(rng, k, lower=0.3)
        h, valid = engine.sketch_kmer_hash(x)
        assert valid and h == R.kmer_hash(x)
        assert engine.sketch_kmer_hash(R.revcomp(x)) == (h, True)
        assert engine.sketch_kmer_hash(x, seed=7) == (R.kmer_hash(x, 7), True)
    x = I.bases(rng, k)
    for at in {0, k // 2, k - 1}:
        for bad in "NnRYUu\n\0 -@[`{":
            assert engine.sketch_kmer_hash((x[:at] + bad + x[at + 1:]).encode("latin-1")) == (0, False)


def test_kmer_hash_reports_every_non_base_byte():
    for b in range(256):
        _, valid = engine.sketch_kmer_hash(b"AC" + bytes([b]) + b"GT")
        assert valid == (chr(b) in R.BASES), b


def _same(case, k, max_hash=FULL):
    keys, off = engine.sketch_cpu(case.seq, case.offsets, k, max_hash=max_hash)
    want_keys, want_off = R.flat(R.sketch(case.seq, case.offsets, k, max_hash))
    assert (off == want_off).all(), (case.name, k)
    assert (keys == want_keys).all(), (case.name, k)
    return keys


@pytest.mark.parametrize("k", range(1, 65))
def test_cpu_sketch_equals_restatement(k):
    """Every generator at every ksize.  (The tile-edge, boundary and read sets are cut from one sequence per ksize, so the
    restatement hashes most k-mers once.)"""
    for case in I.all_cases(k) + I.tile_edges(k) + I.boundaries(k):
        _same(case, k)
    _same(I.mixed(), k, max_hash=R.max_hash_of(3))


@pytest.mark.parametrize("k", [21, 40])
def test_cpu_sketch_short_reads(k):
    one, many = I.short_reads()
    a = _same(one, k, R.max_hash_of(10))
    b = _same(many, k, R.max_hash_of(10))
    assert set(a.tolist()) == set(b.tolist())


def test_cpu_sketch_size_query_overflow_and_arguments():
    c = I.mixed()
    keys, off = engine.sketch_cpu(c.seq, c.offsets, 21, max_hash=FULL)
    L = engine.lib()
    buf = np.frombuffer(c.seq, dtype=np.uint8)
    offs = np.array(c.offsets, dtype=np.uint64)
    out_off = np.zeros(len(c.offsets), dtype=np.uint64)
    needed = engine.ctypes.c_uint64(0)
    room = np.full(keys.size + 4, 0xABAD1DEA, dtype=np.uint64)

    def call(ksize=21, offsets=offs, capacity=keys.size - 1, out=room):
        return L.ksp_sketch_cpu(buf.ctypes.data, buf.size, offsets.ctypes.data, offsets.size - 1, ksize, FULL, 42, out.ctypes.data if out is not None else None,
                                capacity, out_off.ctypes.data, engine.ctypes.byref(needed))

    assert call() == engine.KSP_E_OVERFLOW and needed.value == keys.size and (room == 0xABAD1DEA).all()
    assert call(capacity=0, out=None) == engine.KSP_E_OVERFLOW and needed.value == keys.size
    assert call(capacity=keys.size) == engine.KSP_OK and (room[:keys.size] == keys).all() and (room[keys.size:] == 0xABAD1DEA).all()
    assert (out_off == off).all()
    for bad_k in (0, 65, -1):
        assert call(ksize=bad_k) == engine.KSP_E_ARG
    for bad in ([0, 2000, 1000, 3000], [1, 1000, 2000, 3000], [0, 1000, 2000, 2999]):
        assert call(offsets=np.array(bad, dtype=np.uint64)) == engine.KSP_E_ARG
    assert call(capacity=5, out=None) == engine.KSP_E_ARG
