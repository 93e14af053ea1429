"""The inputs of the classify tests (tests/classify_inputs.py) really contain the edges they are named for — checked with the
restatement (tests/classify_restate.py) alone, no library call."""
import pytest

import classify_inputs as CI
import classify_restate as CR
import sketch_restate as R

K = 21


@pytest.fixture(scope="module")
def repeats():
    case, kept, refs, _ = CI.restated(("repeats", 0), K)
    return case, kept, refs, CR.from_kept(kept, refs)


def test_repeated_kmers_forward_and_by_the_other_strand(repeats):
    case, kept, _, res = repeats
    for r in (0, 1):
        assert res["kept_windows"][r] == len(kept[r]) == len(set(kept[r])) + 6   # k + 5 repeated bases: six k-mers twice
    text = case.seq[case.offsets[1]:case.offsets[2]].decode()
    head, tail = text.split("N")
    assert tail.strip() == R.revcomp(head[:K + 5]) and tail.strip() != head[:K + 5]   # record 1 repeats by its reverse complement
    first = R.source_kmers(text.encode(), K)
    assert len({kmer for _, kmer in first}) == len(first)   # ... so no k-mer TEXT occurs twice: only the canonical forms do


def test_tie_second_no_hit_and_short_record(repeats):
    case, kept, refs, res = repeats
    assert refs[CI.HALF] == refs[CI.COPY] and refs[CI.HALF]
    for r in (0, 1):
        by_ref = {q: n for rr, q, n in res["rows"] if rr == r}
        assert by_ref[CI.HALF] == by_ref[CI.COPY] == res["best_hits"][r] == res["second_hits"][r] > 0   # a tie for best ...
        assert res["best_ref"][r] == CI.HALF                                                            # ... goes to the smaller index
        assert CI.EMPTY not in by_ref and CI.NOWHERE not in by_ref
        assert res["matched"][r] > res["best_hits"][r]   # HALF and THIRD overlap only in part: the union is larger than any one
    assert case.offsets[3] - case.offsets[2] - 1 == K - 1 and kept[2] == []   # shorter than k: no window
    assert res["kept_windows"][2] == 0 and res["best_ref"][2] == CR.NO_REF
    assert len(kept[CI.LONELY]) > 0 and res["matched"][CI.LONELY] == 0 and res["n_refs_hit"][CI.LONELY] == 0   # kept windows, no hit
    assert res["best_ref"][CI.LONELY] == CR.NO_REF and res["second_hits"][CI.LONELY] == 0


def test_one_hash_has_four_holders(repeats):
    _, _, refs, _ = repeats
    shared = refs[CI.PAIR][0]
    assert [q for q in range(len(refs)) if shared in set(refs[q])] == [CI.HALF, CI.THIRD, CI.COPY, CI.PAIR]
    for q in refs:
        assert list(q) == sorted(set(q))   # strictly ascending, as the library wants them


def test_rows_on_both_sides_of_min_hits(repeats):
    _, kept, refs, res = repeats
    m = CI.middle_hits(res["rows"])
    below = [x for x in res["rows"] if x[2] < m]
    assert below and len(below) < len(res["rows"])
    cut = CR.from_kept(kept, refs, m)
    assert cut["rows"] == [x for x in res["rows"] if x[2] >= m]
    assert cut["matched"] == res["matched"] and cut["kept_windows"] == res["kept_windows"]   # the cut touches the rows and their summary only
    assert any(a != b for a, b in zip(cut["n_refs_hit"], res["n_refs_hit"]))
    # a non-zero second_hits that is smaller than best_hits: PAIR's rows against the others
    assert any(0 < s < b for s, b in zip(CR.from_kept(kept, [refs[CI.HALF], refs[CI.PAIR]])["second_hits"], res["best_hits"]))


def test_every_small_case_has_hits_and_references_above_a_threshold():
    for key in CI.small_keys(K):
        _, kept, refs, _ = CI.restated(key, K)
        res = CR.from_kept(kept, refs)
        assert res["rows"], key
        hashes = sorted({h for run in kept for h in run})
        mid = hashes[len(hashes) // 2]
        assert any(h > mid for h in refs[CI.HALF]) and any(h <= mid for h in refs[CI.HALF])   # max_hash = mid cuts the references too
