"""The device path of classify in one batch (csrc/classify.hip: ksp_classify_host; the kernel k_classify_hash of
csrc/classify_kernels.hip.h) against the restatement of the definition (tests/classify_restate.py), rows and all six arrays, at
the smallest shapes where the kernel can go wrong: windows on and beside the tile edge under grids that make every workgroup
loop, records that abut on a tile edge, many short records, the LDS list at its fullest, the threshold at an exact value, the
hit buffer one word too small, a reference hash above max_hash, the cut at min_hits."""
import pytest

import classify_inputs as CI
import classify_restate as CR
import sketch_inputs as I
from kspider_amd import engine

pytestmark = pytest.mark.gpu

FULL = CI.FULL
same = CI.check_result


def _run(key, k, max_hash=FULL, min_hits=1):
    """ksp_classify_host on a named case against the restatement; the references are those of max_hash = FULL."""
    case, kept, refs, (ref_keys, ref_off) = CI.restated(key, k)
    cut = kept if max_hash == FULL else [[h for h in run if h <= max_hash] for run in kept]
    st = same(engine.classify_host(case.seq, case.offsets, k, ref_keys, ref_off, min_hits=min_hits, max_hash=max_hash), CR.from_kept(cut, refs, min_hits), (key, k, max_hash))
    assert st["bases"] == sum(chr(b) in "ACGTacgt" for b in case.seq) and st["batches"] == 1
    assert st["hit_words"] == CI.hit_words(cut, [[h for h in q if h <= max_hash] for q in refs])
    return case, cut, refs, st


@pytest.mark.parametrize("cap", [None, "1", "3"])
@pytest.mark.parametrize("k", [1, 31, 32, 33, 64])
def test_tile_edges_and_abutting_records(monkeypatch, k, cap):
    """One record of T - 1, T, T + 1, T + k - 1 and 2T + 1 bases without and with a break byte at T - 1, T and T + k - 2; records
    that abut without a break byte on and beside a tile edge, one shorter than k, empty ones.  With a grid of 1 and of 3 every
    workgroup loops over tiles and carries its list from one tile into the next."""
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    for key in CI.edge_keys(k) + [("boundaries", i) for i in range(3)]:
        case, _, _, st = _run(key, k)
        tiles = -(-len(case.seq) // I.TILE)
        assert st["workgroups"] == (min(int(cap), tiles) if cap else tiles)
        assert st["retries"] == 0 and st["compactions"] == 0


@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 21, 47, 48, 49, 63])
def test_other_ksizes(k):
    """Bases in both cases, N and other break bytes, three records; repeated k-mers on both strands, a record without a hit."""
    _run(("mixed", 0), k)
    _run(("repeats", 0), k)


def test_no_window_crosses_a_record_boundary():
    case, kept, _, st = _run(("junction", 0), 31)
    assert st["valid_kmers"] == len(case.seq) - 31 + 1 and st["kept_windows"] == st["valid_kmers"] - 30 == sum(len(run) for run in kept)


def test_two_thousand_short_records():
    _, kept, _, st = _run(("reads", 0), 21)
    assert len(kept) == 2000 and st["rows"] > 2000


@pytest.mark.parametrize("cap", [None, "1"])
def test_full_tile_fills_the_list(monkeypatch, cap):
    """max_hash = 2^64 - 1 on T + k - 1 bases without a break: every position of one whole tile survives, the list in LDS is
    drained at its capacity; then 2T + 1 bases, where a grid of 1 drains in the middle of its second tile."""
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    k = 31
    lengths = I.tile_lengths(k)
    keys = CI.edge_keys(k)
    unbroken = [key for key in keys if "breakNone" in CI.restated(key, k)[0].name]
    assert [len(CI.restated(key, k)[0].seq) for key in unbroken] == lengths
    for key, n in zip(unbroken, lengths):
        _, kept, _, st = _run(key, k)
        assert st["kept_windows"] == n - k + 1 == len(kept[0])
    assert lengths[3] - k + 1 == I.TILE


def test_threshold_at_an_exact_hash_and_a_reference_hash_above_it():
    k = 21
    _, kept, refs, _ = CI.restated(("repeats", 0), k)
    hashes = sorted({h for q in refs[:2] for h in q})
    m = hashes[len(hashes) // 2]   # a hash the records and the references hold
    _, at, _, st_at = _run(("repeats", 0), k, max_hash=m)
    _, below, _, st_below = _run(("repeats", 0), k, max_hash=m - 1)
    assert st_at["kept_windows"] > st_below["kept_windows"] and st_at["hit_words"] > st_below["hit_words"]
    above = {h for q in refs for h in q if h > m}
    assert above and st_at["table_keys"] == len({h for q in refs for h in q} - above)   # the table holds no reference hash above max_hash
    _, nothing, _, st = _run(("repeats", 0), k, max_hash=0)
    assert st["kept_windows"] == 0 and st["hit_words"] == 0 and st["rows"] == 0


def test_min_hits_on_both_sides():
    _, kept, refs, _ = CI.restated(("repeats", 0), 21)
    m = CI.middle_hits(CR.from_kept(kept, refs)["rows"])
    rows = [_run(("repeats", 0), 21, min_hits=x)[3]["rows"] for x in (m - 1, m, m + 1)]
    assert rows[0] >= rows[1] >= rows[2] and rows[0] > rows[2]


def test_first_capacity_one_word_too_small(monkeypatch):
    """$KSPIDER_CLASSIFY_FIRST_CAPACITY of 1 and of the need - 1: the words past the room are counted and not written, the buffer
    grows to the counted need and the batch runs again with its tallies off; at the need itself nothing runs twice."""
    key, k = ("mixed", 0), 21
    case, kept, refs, _ = CI.restated(key, k)
    need = CI.hit_words(kept, refs)
    assert need > 2
    for first, retries in ((1, 1), (need - 1, 1), (need, 0), (need + 1, 0)):
        monkeypatch.setenv("KSPIDER_CLASSIFY_FIRST_CAPACITY", str(first))
        _, _, _, st = _run(key, k)
        assert st["retries"] == retries and st["compactions"] == 0 and st["hit_words"] == need   # (nothing is held yet: no compaction)
    monkeypatch.setenv("KSPIDER_CLASSIFY_FIRST_CAPACITY", "0")
    with pytest.raises(engine.KspError) as ei:
        engine.classify_host(case.seq, case.offsets, k, [1], [0, 1], max_hash=FULL)
    assert ei.value.code == engine.KSP_E_ARG and "KSPIDER_CLASSIFY_FIRST_CAPACITY" in str(ei.value)


def test_no_reference_and_no_base():
    case = I.mixed()
    rows, arrays, st = engine.classify_host(case.seq, case.offsets, 21, [], [0], max_hash=FULL)
    want = CR.classify(case.seq, case.offsets, 21, FULL, [])
    assert rows.size == 0 and arrays["kept_windows"].tolist() == want["kept_windows"] and (arrays["best_ref"] == engine.CLASSIFY_NO_REF).all()
    assert st["table_keys"] == 0 and st["hit_words"] == 0
    rows, arrays, st = engine.classify_host(b"NNNN\n\n", [0, 5, 6], 3, [5, 6], [0, 1, 2], max_hash=FULL)
    assert rows.size == 0 and st["valid_kmers"] == 0 and arrays["kept_windows"].tolist() == [0, 0]


def test_refusals():
    case, _, _, (ref_keys, ref_off) = CI.restated(("repeats", 0), 21)

    def refuse(code, *args, **kwargs):
        with pytest.raises(engine.KspError) as ei:
            engine.classify_host(*args, **kwargs)
        assert ei.value.code == code, str(ei.value)
        return str(ei.value)

    refuse(engine.KSP_E_ARG, case.seq, case.offsets, 65, ref_keys, ref_off, max_hash=FULL)
    refuse(engine.KSP_E_ARG, case.seq, case.offsets, 21, ref_keys, ref_off, min_hits=0, max_hash=FULL)
    refuse(engine.KSP_E_ARG, case.seq, [0, 5], 21, ref_keys, ref_off, max_hash=FULL)
    assert "strictly ascending" in refuse(engine.KSP_E_ARG, case.seq, case.offsets, 21, [3, 3], [0, 2], max_hash=FULL)
    assert "no such device" in refuse(engine.KSP_E_HIP, case.seq, case.offsets, 21, ref_keys, ref_off, max_hash=FULL, device=99)
