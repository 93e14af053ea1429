"""The inputs of the second classify suite (tests/classify_edge_inputs.py) really contain the edges they are named for — the drain
schedule, the table shapes, the hit matrix: checked with the restatement alone (engine.query_directory is a host-only call) —
and ksp_classify_cpu gives the restatement's result on every one of them.  No GPU."""
import statistics

import pytest

import classify_edge_inputs as E
import classify_inputs as CI
import classify_restate as CR
import sketch_inputs as I
import sketch_restate as R
from kspider_amd import engine

FULL = CI.FULL
same = CI.check_result


def _schedule(k, s, grid):
    return E.drains(E.keep_positions("sparse", k, R.max_hash_of(s)), E.N_BYTES, grid)


def _partial(n):
    """A drain whose second trip is partial."""
    return E.K_ROUND < n < E.K_LIST_CAP and n % E.K_ROUND != 0


def test_the_streams_are_what_they_say():
    for k in (21, 33):
        one, cut = E.case_of("sparse", k), E.case_of("sparse_records", k)
        assert len(one.seq) == len(cut.seq) == 6 * E.T + 101 and one.seq.count(b"N") == 40 and one.seq.endswith(b"\n")
        assert any(chr(b) in "acgt" for b in one.seq)
        lengths = [b - a for a, b in zip(cut.offsets, cut.offsets[1:])]
        contigs = [r for r, n in enumerate(lengths) if n == 601]
        assert len(contigs) == 2 and 280 <= len(lengths) - 2 <= 360
        for r, edge in zip(contigs, (E.T, 5 * E.T)):
            assert cut.offsets[r] < edge - k and cut.offsets[r + 1] > edge + k   # windows on both sides of a tile edge, and over it
        texts = [cut.seq[a:b] for a, b in zip(cut.offsets, cut.offsets[1:])]
        assert b"" in texts and b"\n" in texts and any(0 < len(t.strip()) < k for t in texts)
        assert any(t and not t.endswith(b"\n") for t in texts[:-1])              # a record that abuts the next base to base
        assert set(cut.seq) <= set(b"ACGTacgt\n")
        for case, name in ((one, "sparse"), (cut, "sparse_records")):   # kept_of is record_hashes, with the positions beside
            for mh in (FULL, R.max_hash_of(3)):
                assert E.kept_of(name, k, mh) == CR.record_hashes(case.seq, case.offsets, k, mh)


@pytest.mark.parametrize("k", [21, 33])
def test_drain_schedule_of_sparse(k):
    for s in (2, 3, 7):
        (inside, last), = _schedule(k, s, 1)
        assert any(_partial(n) for n in inside), (s, inside)
        assert sum(inside) + last == len(E.keep_positions("sparse", k, R.max_hash_of(s)))
    per_wg = _schedule(k, 2, 3)
    assert len(per_wg) == 3 and all(inside and last > 0 for inside, last in per_wg), per_wg
    (inside, last), = _schedule(k, 100, 1)
    assert inside == [] and 1 <= last <= E.K_ROUND
    assert len({p // E.T for p in E.keep_positions("sparse", k, R.max_hash_of(100))}) >= 5   # one list carried over all the tiles


def test_sparse_records_put_boundaries_into_rounds_and_next_to_drains():
    for s in (1, 3):
        case = E.case_of("sparse_records", 21)
        (inside, last), = E.drains(E.keep_positions("sparse_records", 21, R.max_hash_of(s)), E.N_BYTES, 1)
        assert any(_partial(n) for n in inside), inside
        assert len({o // E.K_ROUND for o in case.offsets}) == -(-E.N_BYTES // E.K_ROUND)   # a record boundary in every round


@pytest.fixture(scope="module")
def kept():
    return E.kept_of("sparse_records", 21)


def test_near_miss(kept):
    refs = E.near_miss(kept)
    have = set(E.distinct(kept))
    beside = set(refs[E.BESIDE])
    assert not beside & have and len(beside) > 1000
    assert all(h - 1 in beside and h + 1 in beside for h in E.distinct(kept)[::3])
    res = CR.from_kept(kept, refs)
    assert {q for _, q, _ in res["rows"]} == {E.EVERY_2ND}   # BESIDE and ENDS hit nothing, the hits are beside the misses
    m = E.distinct(kept)[len(have) // 2]
    at = E.near_miss(kept, at=m)
    assert at[E.AT_M] == [m, m + 1] and m in have and any(h > m for q in at for h in q)
    for q in refs + at:
        assert q == sorted(set(q))


def test_skewed(kept):
    refs = E.skewed(kept)
    star = E.skew_target(kept)
    have = set(E.distinct(kept))
    assert len(refs[E.DECOYS]) == 5000 and not set(refs[E.DECOYS]) & have
    assert all(x >> 16 == star >> 16 for x in refs[E.DECOYS]) and star in refs[E.REAL] and star in have
    keys = sorted(set(refs[E.DECOYS]) | set(refs[E.REAL]))
    bits, shift = engine.query_directory(keys[-1], len(keys))
    assert shift > 16   # so the decoys and h* share a bucket; the others hold a handful
    crowd = sum(1 for x in keys if x >> shift == star >> shift)
    assert crowd >= 5001 and statistics.median(sum(1 for x in keys if x >> shift == b) for b in {x >> shift for x in keys}) <= 4


def test_sized(kept):
    have = E.distinct(kept)
    bits = {}
    for U, which in E.SIZES:
        refs = E.sized(kept, U, which)
        keys = sorted({h for q in refs for h in q})
        assert len(keys) == U and all(q == sorted(set(q)) for q in refs)
        bits[(U, which)] = engine.query_directory(keys[-1], U)[0]
        if U > 1:
            assert set(keys) & set(have) and set(keys) - set(have)
            assert sum(len(q) for q in refs) > U   # a key with two holders
    assert bits[(8, None)] != bits[(9, None)] and bits[(4096, None)] != bits[(4097, None)]
    median = statistics.median(have)
    assert E.sized(kept, 1, "smallest")[1][0] < median < E.sized(kept, 1, "largest")[1][0]
    assert E.sized(kept, 1, "smallest")[1][0] in have and E.sized(kept, 1, "largest")[1][0] in have


def test_many(kept):
    refs = E.many(kept)
    assert len(refs) == 2051 > engine.QUERY_TILE_MAX
    assert [q for q, keys in enumerate(refs) if not keys] == sorted(E.MANY_EMPTY) and {0, 1, 2050} < set(E.MANY_EMPTY)
    shared = E.many_shared(kept)
    assert sum(1 for q in refs if shared in set(q)) == 2051 - 13 > 2000
    held = {}
    for q in refs:
        for h in q:
            held[h] = held.get(h, 0) + 1
    assert set(held) == set(E.distinct(kept)) and {n for h, n in held.items() if h != shared} == {1, 2}
    res, cut = CR.from_kept(kept, refs), CR.from_kept(kept, refs, 2)
    with_shared = [r for r, run in enumerate(kept) if shared in run]
    only_shared = [x for x in res["rows"] if x[0] in with_shared and x[2] == 1]
    assert len(only_shared) > 1000 and len(cut["rows"]) < len(res["rows"]) - 1000 and cut["rows"]


def test_hit_matrix():
    kept = E.kept_of("matrix_records", 21)
    m = E.MATRIX
    assert len(m) > 256 and len(m[0]) == 5
    assert not any(m[0]) and not any(m[-1]) and all(not any(m[r]) for r in E.ZEROS_AT) and all(any(m[r + 1]) for r in E.ZEROS_AT)
    refs = E.hit_matrix(kept, m)
    res = CR.from_kept(kept, refs)
    assert res["rows"] == [(r, q, m[r][q]) for r in range(len(m)) for q in range(5) if m[r][q]]
    for i, (row, (best, second)) in enumerate(zip(E.NAMED_ROWS, E.NAMED_SUMMARY)):
        r = E.NAMED_AT + i
        assert m[r] == row and (res["best_ref"][r], res["second_hits"][r]) == (best, second) and res["best_hits"][r] == max(row)
    none = CR.from_kept(kept, refs, 8)
    assert none["rows"] == [] and sum(none["matched"]) > 0 and none["matched"] == res["matched"] and set(none["best_ref"]) == {CR.NO_REF}
    for min_hits in (4, 5):
        cut = CR.from_kept(kept, refs, min_hits)
        assert cut["rows"] and len(cut["rows"]) < len(res["rows"]) and cut["best_ref"] != res["best_ref"]


def test_session_batches():
    batches, texts = E.session_batches(21)
    assert [ids for _, _, ids in batches] == [[5, 2, 5, 0], [1], [70000, 3], [4]]
    assert sorted(texts) == [0, 1, 2, 3, 4, 5, 70000] and texts[5].count("\n") == 2
    seq, off = E.records_of(texts, 70001)
    kept = CR.record_hashes(seq, off, 21, FULL)
    assert len(kept) == 70001 and not kept[4] and all(kept[r] for r in (0, 1, 2, 3, 5, 70000)) and not any(kept[6:70000])
    # the windows of a record are those of its segments: none spans the break between them
    by_segment = {}
    for data, seg_off, ids in batches:
        for r, run in zip(ids, CR.record_hashes(data, seg_off, 21, FULL)):
            by_segment[r] = by_segment.get(r, []) + run
    assert all(by_segment[r] == kept[r] for r in by_segment)


def _cpu(case, k, refs, want, what, **kw):
    ref_keys, ref_off = CR.flat_refs(refs)
    return same(engine.classify_cpu(case.seq, case.offsets, k, ref_keys, ref_off, **kw), want, what)


@pytest.mark.parametrize("k", [21, 33])
def test_classify_cpu_on_the_sparse_streams(k):
    for name, scaled in [("sparse", s) for s in (2, 3, 7, 100)] + [("sparse_records", s) for s in (1, 3)]:
        mh = R.max_hash_of(scaled)
        kept = E.kept_of(name, k, mh)
        refs = CI.references(kept)
        _cpu(E.case_of(name, k), k, refs, CR.from_kept(kept, refs), (name, k, scaled), max_hash=mh)


def test_classify_cpu_on_the_table_shapes(kept):
    case = E.case_of("sparse_records", 21)
    for name, refs in E.table_cases(kept) + [("many", E.many(kept))]:
        st = _cpu(case, 21, refs, CR.from_kept(kept, refs), name, max_hash=FULL)
        assert st["table_keys"] == len({h for q in refs for h in q}) and st["table_holders"] == sum(len(q) for q in refs)
    refs = E.many(kept)
    _cpu(case, 21, refs, CR.from_kept(kept, refs, 2), "many, min_hits 2", max_hash=FULL, min_hits=2)
    m = E.distinct(kept)[len(E.distinct(kept)) // 2]
    refs = E.near_miss(kept, at=m)
    st = _cpu(case, 21, refs, CR.from_kept([[h for h in run if h <= m] for run in kept], refs), "near_miss at m", max_hash=m)
    assert st["table_keys"] == len({h for q in refs for h in q if h <= m})


def test_classify_cpu_on_the_hit_matrix_and_the_session_records():
    kept = E.kept_of("matrix_records", 21)
    refs = E.hit_matrix(kept, E.MATRIX)
    for min_hits in (1, 4, 5, 8, 2**32 - 1):
        _cpu(E.case_of("matrix_records", 21), 21, refs, CR.from_kept(kept, refs, min_hits), min_hits, max_hash=FULL, min_hits=min_hits)
    _, texts = E.session_batches(21)
    seq, off = E.records_of(texts, 70001)
    kept = CR.record_hashes(seq, off, 21, FULL)
    refs = CI.references(kept)
    _cpu(I.Case("session_records", seq, off), 21, refs, CR.from_kept(kept, refs), "session records", max_hash=FULL)
