"""The device path of classify (csrc/classify.hip, csrc/classify_kernels.hip.h, csrc/query_table.hip.h) where its first suite
stops, on the inputs of tests/classify_edge_inputs.py against the restatement (tests/classify_restate.py), rows and all six
arrays: sparse survivors over seven tiles — drains inside the loop whose second trip is partial, one list carried over every
tile and drained once —, record boundaries inside rounds, several workgroups past the hit buffer's room, tables with keys one
beside a probed hash, one crowded bucket, 1, 8, 9, 4 096 and 4 097 keys, 2 051 references and a key with 2 038 holders, a
designed matrix of hit counts under five values of min_hits, and a session with unsorted, repeated, descending and sparse ids."""
import functools

import pytest

import classify_edge_inputs as E
import classify_inputs as CI
import classify_restate as CR
import sketch_restate as R
from kspider_amd import engine

pytestmark = pytest.mark.gpu

FULL = CI.FULL
same = CI.check_result
N_TILES = -(-E.N_BYTES // E.T)
N_REFS_OF_SHARED = E.N_MANY - len(E.MANY_EMPTY)   # the holders of many()'s shared hash


@functools.lru_cache(maxsize=None)
def _sparse(name, k, scaled):
    """(case, max_hash, kept, references, flat references, the restatement's result) of a sparse stream, made once."""
    mh = R.max_hash_of(scaled)
    kept = E.kept_of(name, k, mh)
    refs = CI.references(kept)
    return E.case_of(name, k), mh, kept, refs, CR.flat_refs(refs), CR.from_kept(kept, refs)


def _run_sparse(name, k, scaled, cap, monkeypatch):
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    case, mh, kept, refs, (ref_keys, ref_off), want = _sparse(name, k, scaled)
    st = same(engine.classify_host(case.seq, case.offsets, k, ref_keys, ref_off, max_hash=mh), want, (name, k, scaled, cap))
    assert st["bases"] == sum(chr(b) in "ACGTacgt" for b in case.seq)
    # valid_kmers: the windows without a break byte in the stream, those over two records that abut base to base included
    assert st["valid_kmers"] == len(R.source_kmers(case.seq, k)) >= sum(len(run) for run in E.windows_of(name, k))
    assert st["kept_windows"] == sum(len(run) for run in kept)
    assert st["hit_words"] == CI.hit_words(kept, refs) > 0
    assert st["workgroups"] == (min(int(cap), N_TILES) if cap else N_TILES)
    assert st["retries"] == 0 and st["compactions"] == 0 and st["batches"] == 1
    return st


@pytest.mark.parametrize("cap", [None, "1", "3"])
@pytest.mark.parametrize("scaled", [2, 3, 7, 100])
@pytest.mark.parametrize("k", [21, 33])
def test_sparse_drains(monkeypatch, k, scaled, cap):
    """scaled 2, 3 and 7 under a grid of 1: drains inside the loop of more than kRound and fewer than kListCap entries, no
    multiple of kRound; scaled 2 under a grid of 3: every workgroup drains inside the loop and at the end; scaled 100 under a
    grid of 1: one list carried over all seven tiles and drained once (tests/test_classify_edge_inputs_cpu.py has the schedule)."""
    _run_sparse("sparse", k, scaled, cap, monkeypatch)


@pytest.mark.parametrize("cap", [None, "1"])
@pytest.mark.parametrize("scaled", [1, 3])
@pytest.mark.parametrize("k", [21, 33])
def test_sparse_records(monkeypatch, k, scaled, cap):
    """About 300 records in the same seven tiles: a record boundary in every round and next to every drain, records that abut
    base to base, empty ones, ones shorter than k, two contigs over a tile edge."""
    _run_sparse("sparse_records", k, scaled, cap, monkeypatch)


@pytest.mark.parametrize("cap", [None, "3"])
def test_overflow_across_workgroups(monkeypatch, cap):
    """Seven (and three) workgroups add to the hit counter past the room: what does not fit is counted and not written, the batch
    runs again in the grown buffer, and the result is the one without a second run."""
    case, mh, kept, refs, (ref_keys, ref_off), want = _sparse("sparse", 21, 2)
    need = CI.hit_words(kept, refs)
    assert need // 2 > E.K_LIST_CAP   # at the smallest room, more words are past it than one workgroup's tile can give
    if cap:
        monkeypatch.setenv("KSPIDER_SKETCH_MAX_WGS", cap)
    results = []
    for first, retries in ((need // 2, 1), (need - 1, 1), (need, 0)):
        monkeypatch.setenv("KSPIDER_CLASSIFY_FIRST_CAPACITY", str(first))
        got = engine.classify_host(case.seq, case.offsets, 21, ref_keys, ref_off, max_hash=mh)
        st = same(got, want, (cap, first))
        assert st["retries"] == retries and st["compactions"] == 0 and st["hit_words"] == need and st["workgroups"] == (int(cap) if cap else N_TILES)
        assert st["kept_windows"] == sum(len(run) for run in kept)   # (the second run tallies nothing)
        results.append(got)
    for rows, arrays, _ in results[1:]:
        assert (rows == results[0][0]).all() and all((arrays[name] == results[0][1][name]).all() for name in arrays)


# ---- table shapes, on sparse_records(21) at scaled = 1
@functools.lru_cache(maxsize=None)
def _records():
    kept = E.kept_of("sparse_records", 21)
    return E.case_of("sparse_records", 21), kept, dict(E.table_cases(kept))


def _host(case, k, refs, want, what, **kw):
    ref_keys, ref_off = CR.flat_refs(refs)
    rows, arrays, st = got = engine.classify_host(case.seq, case.offsets, k, ref_keys, ref_off, **kw)
    same(got, want, what)
    return rows, arrays, st


@pytest.mark.parametrize("name", ["near_miss", "skewed"] + [f"sized{U}{which or ''}" for U, which in E.SIZES])
def test_table_shapes(name):
    """near_miss: the compare behind the search decides every miss of BESIDE.  skewed: one of a lane's look-ups halves a bucket
    of 5 001 keys while the others halve a handful.  sized: the directory on both sides of n_keys = 4 << b at 8 | 9 and
    4 096 | 4 097, and a table of one key, the smallest record hash (every other probe is cut at max_key) or the largest."""
    case, kept, tables = _records()
    refs = tables[name]
    rows, _, st = _host(case, 21, refs, CR.from_kept(kept, refs), name, max_hash=FULL)
    designed = {"near_miss": len({h for q in refs for h in q}), "skewed": 5000 + len(refs[-1])}
    designed.update({f"sized{U}{which or ''}": U for U, which in E.SIZES})
    assert st["table_keys"] == designed[name] and st["table_holders"] == sum(len(q) for q in refs)
    assert st["hit_words"] == CI.hit_words(kept, refs) > 0
    if name == "skewed":
        star = E.skew_target(kept)
        holders = [r for r, run in enumerate(kept) if star in run]
        assert holders
        for r in holders:
            assert [int(x["reference"]) for x in rows if x["record"] == r] == [E.REAL]   # h* is found among the decoys, and no decoy is
        assert not (rows["reference"] == E.DECOYS).any()
    if name.startswith("sized1"):
        assert st["hit_words"] == sum(run.count(refs[1][0]) for run in kept) and st["rows"] >= 1


def test_near_miss_under_a_max_hash_that_is_a_key():
    """max_hash = m, a record hash that a reference holds beside m + 1: m is the table's largest key and is hit, every key above
    it is out of the table."""
    case, kept, _ = _records()
    m = E.distinct(kept)[len(E.distinct(kept)) // 2]
    refs = E.near_miss(kept, at=m)
    cut = [[h for h in run if h <= m] for run in kept]
    want = CR.from_kept(cut, refs)
    rows, _, st = _host(case, 21, refs, want, "near_miss at m", max_hash=m)
    everything = {h for q in refs for h in q}
    assert st["table_keys"] == len({h for h in everything if h <= m}) < len(everything)
    assert any(q == E.AT_M and n == 1 for _, q, n in want["rows"]) and (rows["reference"] == E.AT_M).sum() == sum(1 for run in kept if m in run)


def test_many_references():
    """2 051 references in the one tile of the table, empty ones first, last and in the middle; a key whose 2 038 pairs span
    eight blocks of k_classify_expand; min_hits = 2 drops the rows that exist through that key alone."""
    case, kept, _ = _records()
    refs = E.many(kept)
    whole = CR.from_kept(kept, refs)
    _, arrays, st = _host(case, 21, refs, whole, "many", max_hash=FULL)
    assert st["table_keys"] == len(E.distinct(kept)) and st["table_holders"] == sum(len(q) for q in refs)
    assert int(arrays["n_refs_hit"].max()) >= N_REFS_OF_SHARED
    cut = CR.from_kept(kept, refs, 2)
    assert len(cut["rows"]) < len(whole["rows"]) - 1000
    _host(case, 21, refs, cut, "many, min_hits 2", max_hash=FULL, min_hits=2)



@functools.lru_cache(maxsize=None)
def _matrix():
    kept = E.kept_of("matrix_records", 21)
    return E.case_of("matrix_records", 21), kept, E.hit_matrix(kept, E.MATRIX)


@pytest.mark.parametrize("min_hits", [1, 4, 5, 8, 2**32 - 1])
def test_hit_matrix(min_hits):
    """hits(r, q) = MATRIX[r][q] by construction: three- and five-way ties for best and for second, a best in every column,
    all-zero records first, last and alternating, over two blocks of k_classify_summary; min_hits above every count: no row at
    all while the runs exist."""
    case, kept, refs = _matrix()
    want = CR.from_kept(kept, refs, min_hits)
    rows, arrays, st = _host(case, 21, refs, want, min_hits, max_hash=FULL, min_hits=min_hits)
    assert arrays["matched"].tolist() == [max(row) for row in E.MATRIX]
    if min_hits == 1:
        for i, (best, second) in enumerate(E.NAMED_SUMMARY):
            r = E.NAMED_AT + i
            assert (int(arrays["best_ref"][r]), int(arrays["second_hits"][r])) == (best, second)
    if min_hits >= 8:
        assert rows.size == 0 and st["rows"] == 0 and (arrays["best_ref"] == engine.CLASSIFY_NO_REF).all() and st["hit_words_unique"] > 0
        assert not arrays["n_refs_hit"].any() and not arrays["best_hits"].any() and not arrays["second_hits"].any()


def _session(batches, texts, n_records, k=21):
    """The batches through a session against the restatement of the records' joined texts."""
    seq, off = E.records_of(texts, n_records)
    kept = CR.record_hashes(seq, off, k, FULL)
    refs = CI.references(kept)
    ref_keys, ref_off = CR.flat_refs(refs)
    with engine.ClassifySession(k, ref_keys, ref_off, max_hash=FULL) as s:
        for data, seg_off, ids in batches:
            s.add(data, seg_off, ids)
        got = s.finish(n_records)
    st = same(got, CR.from_kept(kept, refs), "session")
    assert st["batches"] == len(batches) and st["hit_words"] == CI.hit_words(kept, refs) > 0
    return got, kept


def test_session_ids_unsorted_repeated_descending_and_sparse():
    """Ids [5, 2, 5, 0] in one batch (record 5 is two segments with another between them), then [1], then [70000, 3], then break
    bytes alone for record 4; finish(70001).  The kept-window counters grow from none to 6 and from 6 to 70 001 between adds
    and keep what they held; records 6 .. 69 999 are empty."""
    batches, texts = E.session_batches(21)
    (rows, arrays, _), kept = _session(batches, texts, 70001)
    assert set(rows["record"].tolist()) == {0, 1, 2, 3, 5, 70000}
    assert not arrays["kept_windows"][6:70000].any() and (arrays["best_ref"][6:70000] == engine.CLASSIFY_NO_REF).all()
    segments_of_5 = [CR.record_hashes(batches[0][0], batches[0][1], 21, FULL)[s] for s in (0, 2)]
    assert int(arrays["kept_windows"][5]) == sum(map(len, segments_of_5)) and all(segments_of_5) and int(arrays["kept_windows"][4]) == 0


def test_kept_windows_survive_five_growths_of_their_counters():
    """One record per batch with ids 0, 1, 3, 9, 40 — each beyond twice the room there is, so every add but the last grows the
    counters (to 1, 2, 4, 10, 41) and copies what they held — and then 2, below them all."""
    batches, texts = E.session_batches(21, plan=E.GROWTH_PLAN, breaks_only=())
    (_, arrays, _), kept = _session(batches, texts, 41)
    assert [r for r in range(41) if arrays["kept_windows"][r]] == [0, 1, 2, 3, 9, 40]
