"""The device hash passes of the protein, dayhoff and hp sketches (csrc/sketch_kernels.hip.h behind ksp_sketch_host_mol /
ksp_sketch_device_mol) against the host loop ksp_sketch_cpu_mol — which tests/test_sketch_protein_cpu.py holds to the restatement
— keys and counts, on the inputs of tests/sketch_protein_inputs.py: the k lists, streams of two to three tiles that end 1 .. 15
bytes into a 16-byte piece, abutting sources, one hash some thousand times over a tile edge, both strands surviving at every
position, a grid of one workgroup, the retry, the size query."""
import functools

import numpy as np
import pytest

import sketch_protein_inputs as I
import sketch_protein_restate as P
from kspider_amd import engine

pytestmark = pytest.mark.gpu

FULL = 2**64 - 1
FEW = P.max_hash_of(25)
GUARD = 0xD15EA5ED0DDBA11
MOLS = [P.PROTEIN, P.DAYHOFF, P.HP]


def _same(case, k, mol, translated, max_hash=FULL):
    want_keys, want_abund, want_off = engine.sketch_cpu_mol(case.seq, case.offsets, k, mol, translated, max_hash=max_hash, abund=True)
    keys, abund, off, st = engine.sketch_host_mol(case.seq, case.offsets, k, mol, translated, max_hash=max_hash, abund=True)
    assert (off == want_off).all(), (case.name, k, mol, translated)
    assert (keys == want_keys).all() and (abund == want_abund).all(), (case.name, k, mol, translated)
    assert st["distinct_out"] == keys.size and st["kept"] == st["needed"] == int(abund.sum())   # (no count near 2^32 here)
    assert st["valid_kmers"] == P.n_windows(case.seq, k, translated)                             # windows of the stream, not strands
    plain_keys, plain_off, _ = engine.sketch_host_mol(case.seq, case.offsets, k, mol, translated, max_hash=max_hash)
    assert (plain_keys == keys).all() and (plain_off == off).all()
    return keys, abund, off, st


@functools.lru_cache(maxsize=None)
def _streams(dna):
    return I.tile_streams(dna=dna) + [I.three_tiles(dna=dna)]


@pytest.mark.parametrize("mol", MOLS)
@pytest.mark.parametrize("k", I.RESIDUE_K)
def test_protein_input_every_k(k, mol):
    _same(I.protein_mixed(), k, mol, False)
    _same(I.all_byte_values(), k, mol, False, FEW)


@pytest.mark.parametrize("mol", MOLS)
@pytest.mark.parametrize("k", I.TRANSLATED_K)
def test_translated_input_every_k(k, mol):
    """At scaled 1 both strands survive at every position."""
    c = I.dna_mixed()
    _, abund, _, st = _same(c, k, mol, True)
    inside = sum(P.n_windows(c.seq[c.offsets[s]:c.offsets[s + 1]], k, True) for s in range(3))   # (valid_kmers also counts the windows over a seam)
    assert st["kept"] == 2 * inside > 0 and st["valid_kmers"] >= inside
    _same(c, k, mol, True, FEW)
    _same(I.break_at_every_offset(k), k, mol, True)


@pytest.mark.parametrize("cap", [None, "1"])
@pytest.mark.parametrize("k", I.TRANSLATED_K)
def test_translated_tile_edges_and_stream_ends(monkeypatch, k, cap):
    """Two tiles and 1 .. 15 bytes, and three tiles exactly: windows over both edges in every codon phase, the last window ending
    at the stream's end, the positions behind it reaching into the halo beyond it.  With a grid of 1 the workgroup loops."""
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    for c in _streams(True):
        _, _, _, st = _same(c, k, P.PROTEIN, True)
        assert st["workgroups"] == (1 if cap else 3)
    for c in I.abutting(3 * k):
        _same(c, k, P.HP, True)


@pytest.mark.parametrize("cap", [None, "1"])
@pytest.mark.parametrize("k", I.RESIDUE_K)
def test_protein_tile_edges_and_stream_ends(monkeypatch, k, cap):
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    for c in _streams(False):
        _, _, _, st = _same(c, k, P.DAYHOFF if k > 8 else P.PROTEIN, False)   # (few distinct dayhoff k-mers at a small k: counts in the thousands)
        assert st["workgroups"] == (1 if cap else 3)
    for c in I.abutting(k, dna=False):
        _same(c, k, P.PROTEIN, False)


@pytest.mark.parametrize("k", [1, 10, 21])
def test_one_hash_some_thousand_times_over_a_tile_edge(k):
    c = I.poly_a()
    keys, abund, _, st = _same(c, k, P.PROTEIN, True)
    n = len(c.seq) - 3 * k + 1
    want = {engine.sketch_text_hash("K" * k, "protein")[0]: n, engine.sketch_text_hash("F" * k, "protein")[0]: n}
    assert dict(zip(keys.tolist(), abund.tolist())) == want and n > I.TILE + 1900
    keys, abund, _, _ = _same(I.Case("poly_m", b"M" * (I.TILE + 2000), [0, I.TILE + 2000]), k, P.HP, False)
    assert keys.tolist() == [engine.sketch_text_hash("M" * k, "hp")[0]] and abund.tolist() == [I.TILE + 2000 - k + 1]


@pytest.mark.parametrize("k", [2, 10])
def test_strands_that_translate_alike_count_twice(k):
    keys, abund, _, _ = _same(I.alike_on_both_strands(k), k, P.PROTEIN, True)
    assert keys.size == 1 and abund.tolist() == [2]


@pytest.mark.parametrize("mol,k,translated", [(P.PROTEIN, 10, True), (P.HP, 21, True), (P.DAYHOFF, 17, False)])
def test_retry_size_query_and_guards(monkeypatch, mol, k, translated):
    c = I.three_tiles(dna=translated)
    want_keys, want_abund, want_off = engine.sketch_cpu_mol(c.seq, c.offsets, k, mol, translated, max_hash=FULL, abund=True)
    needed = int(want_abund.sum())
    # the size query: capacity 0, NULL outputs -> the exact number of survivors
    seq = np.zeros(len(c.seq) + 16, dtype=np.uint8)
    seq[:len(c.seq)] = np.frombuffer(c.seq, dtype=np.uint8)
    d_seq = engine.DeviceBuffer.from_numpy(seq)
    rc, _, st = engine.sketch_device_mol(d_seq.ptr.value, len(c.seq), c.offsets, k, mol, translated, FULL, 0, 0, 0)
    assert rc == engine.KSP_E_OVERFLOW and st["needed"] == needed
    for capacity in (needed - 1, needed):
        d_keys = engine.DeviceBuffer.from_numpy(np.full(capacity + 8, GUARD, dtype=np.uint64))
        d_abund = engine.DeviceBuffer.from_numpy(np.full(capacity + 8, 0xABCD1234, dtype=np.uint32))
        rc, off, st = engine.sketch_device_mol(d_seq.ptr.value, len(c.seq), c.offsets, k, mol, translated, FULL, d_keys.ptr.value, d_abund.ptr.value, capacity)
        got, got_abund = d_keys.to_numpy(np.uint64, capacity + 8), d_abund.to_numpy(np.uint32, capacity + 8)
        d_keys.free()
        d_abund.free()
        assert st["needed"] == needed
        if capacity < needed:
            assert rc == engine.KSP_E_OVERFLOW and (got == GUARD).all() and (got_abund == 0xABCD1234).all()   # nothing at all was written
        else:
            assert rc == engine.KSP_OK and (off == want_off).all()
            assert (got[:want_keys.size] == want_keys).all() and (got[capacity:] == GUARD).all()
            assert (got_abund[:want_keys.size] == want_abund).all() and (got_abund[capacity:] == 0xABCD1234).all()
    d_seq.free()
    # the host call: a small first capacity makes the retry run; the default one doubles for translated input and does not
    monkeypatch.setenv("KSPIDER_SKETCH_FIRST_CAPACITY", "100")
    keys, abund, off, st = engine.sketch_host_mol(c.seq, c.offsets, k, mol, translated, max_hash=FULL, abund=True)
    assert st["retries"] == 1 and (keys == want_keys).all() and (abund == want_abund).all() and (off == want_off).all()
    monkeypatch.delenv("KSPIDER_SKETCH_FIRST_CAPACITY")
    _, _, st = engine.sketch_host_mol(c.seq, c.offsets, k, mol, translated, max_hash=FULL)
    assert st["retries"] == 0 and st["kept"] == needed


def test_moltype_0_and_refusals():
    c = I.dna_mixed()
    keys, abund, off, _ = engine.sketch_host_mol(c.seq, c.offsets, 21, 0, max_hash=FEW, abund=True)
    want = engine.sketch_host_abund(c.seq, c.offsets, 21, max_hash=FEW)
    assert (keys == want[0]).all() and (abund == want[1]).all() and (off == want[2]).all()
    for k, mol, translated in [(22, P.PROTEIN, True), (0, P.PROTEIN, True), (65, P.PROTEIN, False), (10, 0, True), (10, 4, False)]:
        with pytest.raises(engine.KspError) as ei:
            engine.sketch_host_mol(c.seq, c.offsets, k, mol, translated, max_hash=FULL, device=99)   # refused before a device is chosen
        assert ei.value.code == engine.KSP_E_ARG
