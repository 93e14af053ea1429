"""The device hash passes of the protein, dayhoff and hp sketches (k_sketch_hash_protein and k_sketch_hash_translated,
csrc/sketch_kernels.hip.h, behind ksp_sketch_host_mol) at the edges that tests/test_sketch_protein_gpu.py leaves out, against
the restatement (tests/sketch_protein_restate.py) itself and not the host loop, which shares sketch_mol.h with the kernels:
proteome-shaped streams of a thousand abutting sources, hash seeds other than 42, max_hash exactly at one strand's hash, the six
frames as protein input on the device, a retry that the input and not the environment forces, the default grid with more tiles
than workgroups, and a seeded sweep.  Every comparison also holds the counters bases, valid_kmers, kept and needed, and the plain
call, to the restatement."""
import functools
import random
import subprocess
import sys

import numpy as np
import pytest

import sketch_protein_inputs as I
import sketch_protein_restate as P
from kspider_amd import engine

pytestmark = pytest.mark.gpu

FULL = 2**64 - 1
FEW = P.max_hash_of(25)
T = I.TILE

_restated = {}


def _want(case, k, mol, translated, max_hash, seed):
    """The restatement's (keys, abund, offsets, bases, windows) of a case: computed once, shared, left unchanged."""
    key = (case.name, len(case.seq), k, mol, translated, max_hash, seed)
    if key not in _restated:
        flat = P.flat(P.counted_sketch(case.seq, case.offsets, k, mol, translated, max_hash, seed))
        alphabet = P.BASES if translated else P.RESIDUES
        _restated[key] = flat + (sum(chr(x) in alphabet for x in case.seq), P.n_windows(case.seq, k, translated))
    return _restated[key]


def _same(case, k, mol, translated, max_hash=FULL, seed=42, note=None):
    note = note or (case.name, k, mol, translated, max_hash, seed)
    want_keys, want_abund, want_off, bases, windows = _want(case, k, mol, translated, max_hash, seed)
    keys, abund, off, st = engine.sketch_host_mol(case.seq, case.offsets, k, mol, translated, max_hash=max_hash, seed=seed, abund=True)
    assert off.tolist() == want_off.tolist(), note
    assert keys.tolist() == want_keys.tolist() and abund.tolist() == want_abund.tolist(), note
    assert st["bases"] == bases, note                                  # the tile's bytes, not the halo's
    assert st["valid_kmers"] == windows, note                          # windows of the stream, not strands
    assert st["kept"] == st["needed"] == int(abund.sum()) and st["distinct_out"] == keys.size, note
    plain_keys, plain_off, plain_st = engine.sketch_host_mol(case.seq, case.offsets, k, mol, translated, max_hash=max_hash, seed=seed)
    assert plain_keys.tolist() == keys.tolist() and plain_off.tolist() == off.tolist(), note
    assert plain_st["bases"] == bases and plain_st["valid_kmers"] == windows, note
    return keys, abund, off, st


# ---- a. proteome-shaped streams

@pytest.mark.parametrize("cap", [None, "2"])
@pytest.mark.parametrize("k,mol,translated", [(1, P.PROTEIN, False), (7, P.DAYHOFF, False), (16, P.HP, False), (33, P.PROTEIN, False), (64, P.DAYHOFF, False),
                                              (1, P.HP, True), (7, P.PROTEIN, True), (21, P.DAYHOFF, True)])
def test_many_abutting_sources(monkeypatch, k, mol, translated, cap):
    """Hundreds to thousands of sources in four tiles, their ends at every offset of a 16-byte piece and on both sides of the tile
    edges, most of them empty or shorter than a window: the source search of the mol kernels and k_sketch_offsets over empty
    sources.  With a cap of 2 the two workgroups loop over two tiles each."""
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    else:
        monkeypatch.delenv("KSPIDER_SKETCH_MAX_WGS", raising=False)
    c = I.many_sources(3 * k if translated else k, translated)
    for max_hash in (FULL, FEW):
        keys, _, off, st = _same(c, k, mol, translated, max_hash)
        assert st["workgroups"] == (2 if cap else 4)
        assert max_hash == FEW or (keys.size > 0 and off[-1] == keys.size and len(off) - 1 > 100)


# ---- b. the seed

@pytest.mark.parametrize("k,mol,translated", [(9, P.PROTEIN, False), (33, P.HP, False), (10, P.DAYHOFF, True), (11, P.PROTEIN, True)])
def test_the_seed_is_live(k, mol, translated):
    c = I.dna_mixed() if translated else I.protein_mixed()
    keys_of = {}
    for seed in (42, 0, 1, 2**32 - 1, random.Random(5).getrandbits(32)):
        for max_hash in (FULL, FEW):
            keys_of[(seed, max_hash)] = _same(c, k, mol, translated, max_hash, seed)[0].tolist()
    want0, want42 = _want(c, k, mol, translated, FULL, 0)[0], _want(c, k, mol, translated, FULL, 42)[0]
    assert want0.tolist() != want42.tolist() and keys_of[(0, FULL)] != keys_of[(42, FULL)]   # live in the restatement, too


# ---- c. the threshold, per strand

def _exactly_at(c, k, mol, translated, m):
    at, _, _, _ = _same(c, k, mol, translated, m)
    below, _, _, _ = _same(c, k, mol, translated, m - 1)
    assert set(at.tolist()) - set(below.tolist()) == {m} and set(below.tolist()) <= set(at.tolist())
    assert 0 < below.size and at.size < _want(c, k, mol, translated, FULL, 42)[0].size


def test_threshold_is_inclusive_for_each_strand():
    """m1 is the hash of k-mers that only forward strands spell, m2 of k-mers that only reverse strands spell: at max_hash = m1 a
    position's forward hash is exactly at the threshold while its reverse hash is not, at m2 the other way round."""
    c = I.dna_mixed()
    m1, m2 = I.strand_thresholds(c, 10, P.PROTEIN)
    _exactly_at(c, 10, P.PROTEIN, True, m1)
    _exactly_at(c, 10, P.PROTEIN, True, m2)


def test_threshold_is_inclusive_for_protein_input():
    c = I.protein_mixed()
    _exactly_at(c, 17, P.PROTEIN, False, I.median_hash(c, 17, P.PROTEIN, False))


@pytest.mark.parametrize("k,mol,translated", [(10, P.PROTEIN, True), (17, P.PROTEIN, False)])
def test_max_hash_0_keeps_nothing(k, mol, translated):
    c = I.dna_mixed() if translated else I.protein_mixed()
    keys, abund, off, st = _same(c, k, mol, translated, 0)
    assert keys.size == 0 and abund.size == 0 and not off.any() and st["kept"] == 0
    assert st["valid_kmers"] == P.n_windows(c.seq, k, translated) > 0


# ---- d. six frames on the device

@pytest.mark.parametrize("k", [1, 7, 11, 21])
def test_translated_equals_protein_input_of_the_six_frames_on_the_device(k):
    """The translated kernel (codons off a packed k-mer through the 64-byte table) against the protein kernel (letters from LDS
    through funnel shifts) on the six frame translations of the same records, all frames in one source: the same hashes, and the
    same counts, a hash's translated abundance being the sum over the six frames."""
    long_record = I.bases(random.Random(80 + k), 2 * T + 5, lower=0.1)
    for records in ([long_record], I.clean_records(I.dna_mixed())):
        dna = "\n".join(records).encode()
        protein = I.six_frames(records)
        for mol in (P.PROTEIN, P.HP):
            for max_hash in (FULL, FEW):
                keys, abund, _, st = engine.sketch_host_mol(dna, [0, len(dna)], k, mol, True, max_hash=max_hash, abund=True)
                want_keys, want_abund, _, want_st = engine.sketch_host_mol(protein, [0, len(protein)], k, mol, False, max_hash=max_hash, abund=True)
                assert keys.tolist() == want_keys.tolist() and abund.tolist() == want_abund.tolist(), (k, mol, max_hash, len(records))
                assert st["kept"] == want_st["kept"] and (keys.size > 0 or max_hash == FEW or not any(len(r) >= 3 * k for r in records))
                plain, _, _ = engine.sketch_host_mol(dna, [0, len(dna)], k, mol, True, max_hash=max_hash)
                assert plain.tolist() == keys.tolist()


# ---- e. a retry that the input forces

@pytest.mark.parametrize("translated", [False, True])
def test_natural_retry(monkeypatch, translated):
    """Low-complexity input at scaled 1000 and k = 8 beats the first capacity of sketch_host (sketch_protein_inputs.first_capacity_guess,
    pinned by tests/test_sketch_protein_inputs_cpu.py): 12 281 survivors against 4 111, translated 9 550 against 8 262."""
    monkeypatch.delenv("KSPIDER_SKETCH_FIRST_CAPACITY", raising=False)
    c = I.low_complexity(translated)
    max_hash = P.max_hash_of(1000)
    keys, abund, off, st = engine.sketch_host_mol(c.seq, c.offsets, 8, P.PROTEIN, translated, scaled=1000, abund=True)
    assert st["retries"] == 1
    assert keys.tolist() == [72033104883516] and abund.tolist() == [9550 if translated else 12281] and off.tolist() == [0, 1]
    assert st["needed"] > I.first_capacity_guess(len(c.seq), max_hash, translated)
    _, _, _, st = _same(c, 8, P.PROTEIN, translated, max_hash)
    assert st["retries"] == 1


# ---- f. the default grid, looping

@functools.lru_cache(maxsize=None)
def _compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once and in a process of its own: torch brings a HIP runtime
    of its own, which finds no device in a process where the library has already initialised one."""
    done = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    return int(done.stdout.split()[-1])


@pytest.mark.parametrize("translated", [False, True])
def test_default_grid_with_more_tiles_than_workgroups(monkeypatch, translated):
    """8 CUs + 3 tiles and 9 bytes under the default cap of 8 workgroups per CU: three workgroups take a second tile.  The
    restatement is too slow for this length; the reference is the host loop, which test_many_abutting_sources ties to the
    restatement at the tile edges through the device."""
    monkeypatch.delenv("KSPIDER_SKETCH_MAX_WGS", raising=False)
    cus = _compute_units()
    assert cus >= 1
    c = I.long_stream(8 * cus + 3, translated)
    want_keys, want_abund, want_off = engine.sketch_cpu_mol(c.seq, c.offsets, 10, P.PROTEIN, translated, scaled=1000, abund=True)
    keys, abund, off, st = engine.sketch_host_mol(c.seq, c.offsets, 10, P.PROTEIN, translated, scaled=1000, abund=True)
    assert st["workgroups"] == 8 * cus
    assert (off == want_off).all() and (keys == want_keys).all() and (abund == want_abund).all() and keys.size > 1000
    bases, windows = int((np.frombuffer(c.seq, dtype=np.uint8) != 10).sum()), P.n_windows(c.seq, 10, translated)   # (0.6 s on 8.4 MB)
    assert st["bases"] == bases and st["valid_kmers"] == windows > 0 and st["kept"] == st["needed"] == int(abund.sum())
    plain_keys, plain_off, plain_st = engine.sketch_host_mol(c.seq, c.offsets, 10, P.PROTEIN, translated, scaled=1000)
    assert (plain_keys == keys).all() and (plain_off == off).all()
    assert plain_st["bases"] == bases and plain_st["valid_kmers"] == windows and plain_st["workgroups"] == 8 * cus


# ---- g. a seeded sweep

@pytest.mark.parametrize("seed", I.SWEEP_SEEDS)
def test_seeded_sweep(monkeypatch, seed):
    """12 random cases per seed (sketch_protein_inputs.sweep_cases); the message of a failure holds what replays the case alone."""
    for i, d in enumerate(I.sweep_cases(seed)):
        c = d["case"]
        if d["cap"]:
            monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", d["cap"])
        else:
            monkeypatch.delenv("KSPIDER_SKETCH_MAX_WGS", raising=False)
        note = dict(sweep_seed=seed, index=i, n_bytes=len(c.seq), n_sources=len(c.offsets) - 1, **{x: d[x] for x in ("k", "mol", "translated", "max_hash", "seed", "cap", "density")})
        _, _, _, st = _same(c, d["k"], d["mol"], d["translated"], d["max_hash"], d["seed"], note=note)
        n_tiles = (len(c.seq) + T - 1) // T
        assert st["workgroups"] == (min(int(d["cap"]), n_tiles) if d["cap"] else n_tiles), note
