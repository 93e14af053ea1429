"""tests/slice_inputs.py checked on the CPU: the cuts are partitions, part_of agrees with them on the cut keys, the
postings cuts follow the documented rule, and cut_input's promised edges are what the brute-force oracle finds."""
import numpy as np
import pytest

import slice_inputs as S

BIG_SPANS = [1 << 32, 1 << 63, (1 << 64) - 1, 1 << 64]


def _is_partition(span, nparts):
    cuts = S.key_cuts(span, nparts)
    assert len(cuts) == nparts and cuts[0][0] == 0 and cuts[-1][1] == span
    for (lo, end), (lo2, _) in zip(cuts, cuts[1:]):
        assert lo <= end == lo2
    assert all(lo <= end for lo, end in cuts)
    return cuts


def test_key_cuts_partition_small_spans():
    for span in range(1, 131):
        for nparts in range(1, 65):
            cuts = _is_partition(span, nparts)
            owner = np.full(span, -1)
            for p, (lo, end) in enumerate(cuts):
                assert (owner[lo:end] == -1).all()
                owner[lo:end] = p
            assert (owner >= 0).all()
            assert (S.part_of(np.arange(span, dtype=np.uint64), span, nparts) == owner).all(), (span, nparts)
            # sizes differ by one at most; exactly span parts hold a key when span < nparts
            width = np.array([end - lo for lo, end in cuts])
            assert width.max() - width.min() <= 1 and (width > 0).sum() == min(span, nparts)


@pytest.mark.parametrize("span", BIG_SPANS)
@pytest.mark.parametrize("nparts", [2, 3, 7, 64])
def test_key_cuts_partition_big_spans(span, nparts):
    cuts = _is_partition(span, nparts)
    ks, want = [], []
    for p, (lo, end) in enumerate(cuts):
        assert end > lo
        for k in (lo, lo + 1, (lo + end) // 2, end - 2, end - 1):
            ks.append(k)
            want.append(p)
    assert max(ks) == span - 1 <= S.M64
    got = S.part_of(np.array(ks, dtype=np.uint64), span, nparts)
    assert (got == np.array(want)).all()
    assert S.boundary_keys(span, nparts)[-1][-1] == span - 1


def test_issue_table_of_wrapped_bounds():
    """What lo <= key <= (end - 1) mod 2^64 keeps when the end of a part is 0: the reading the GPU tests decide on."""
    def kept(span, nparts, k):
        n = 0
        for lo, end in S.key_cuts(span, nparts):
            n += lo <= k <= ((end - 1) & S.M64)
        return n
    assert [kept(1, 2, 0)] == [2]
    assert [kept(2, 3, k) for k in range(2)] == [2, 2]
    assert [kept(3, 8, k) for k in range(3)] == [3, 3, 3]
    assert [kept(6, 2, k) for k in range(6)] == [1] * 6
    # the contract gives every key to one part
    for span, nparts in ((1, 2), (2, 3), (3, 8)):
        assert np.bincount(S.part_of(np.arange(span), span, nparts), minlength=nparts).sum() == span


def test_postings_cuts():
    rng = np.random.default_rng(5)
    shapes = {
        "uniform": np.full(200, 3),
        "ragged": rng.integers(2, 40, size=300),
        "first half": np.concatenate([[1000], np.full(500, 2)]),
        "last half": np.concatenate([np.full(500, 2), [1000]]),
        "middle half": np.concatenate([np.full(250, 2), [1000], np.full(250, 2)]),
        "few": np.array([2, 5, 2]),
    }
    for name, cnt in shapes.items():
        key_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        n_keys, n = cnt.size, int(key_off[-1])
        for nd in (1, 2, 3, 5, 7, 64):
            cuts = S.postings_cuts(key_off, nd)
            if nd == 1 or nd > n_keys:
                assert cuts == [0, n_keys], (name, nd)
                continue
            assert len(cuts) == nd + 1 and cuts[0] == 0 and cuts[-1] == n_keys, (name, nd)
            assert all(a < b for a, b in zip(cuts, cuts[1:])), (name, nd, cuts)
            for s in range(1, nd):   # the rule: the first key at or past the goal, unless a neighbour's minimum moves it
                goal = n // nd * s
                free = cuts[s] > cuts[s - 1] + 1 and cuts[s] < n_keys - (nd - s)
                if free:
                    assert key_off[cuts[s]] >= goal > key_off[cuts[s] - 1], (name, nd, s)
    # n_keys == nd: one key each
    assert S.postings_cuts([0, 2, 4, 9], 3) == [0, 1, 2, 3]
    assert S.postings_cuts([0, 2, 4, 9], 4) == [0, 3]
    # a key holding half of everything, first: slice 0 is that key alone
    assert S.postings_cuts(np.concatenate([[0], np.cumsum([100] + [2] * 50)]), 2)[1] == 1


@pytest.mark.parametrize("span", [5, 64, 65, (1 << 20) + 1, 1 << 63, 1 << 64])
@pytest.mark.parametrize("nparts", [2, 3, 7, 64])
def test_cut_input_promise_equals_brute_force(oracle_lib, span, nparts):
    for n_sources, empty in ((0, ()), (10, ()), (0, (0,)), (7, (1,))):
        if any(p >= nparts - 1 for p in empty):   # (the last part keeps key span - 1)
            continue
        keys, offsets, want, kept = S.cut_input(span, nparts, n_sources, empty_parts=empty)
        ref = oracle_lib.brute_pairs(keys, offsets)
        assert len(ref) == len(want) and (ref == want).all(), (span, nparts, n_sources)
        assert int(want["shared"].sum()) == int(kept.sum())
        assert (S.kept_keys_per_part(keys, span, nparts) == kept).all()
        assert int(keys.max()) == span - 1       # the engine derives this span from the data
        if span >= 8 * nparts and not empty:      # every cut key is there, on its side of the cut
            uk = set(np.unique(keys).tolist())
            for lo, end in S.key_cuts(span, nparts):
                assert {lo, lo + 1, end - 2, end - 1} <= uk


def test_small_span_input(oracle_lib):
    for span in (1, 2, 3, 4):
        for holders in (2, 3):
            keys, offsets, who = S.small_span_input(span, holders)
            assert int(keys.max()) == span - 1
            ref = oracle_lib.brute_pairs(keys, offsets)
            want = S.pairs_from_holders(who)
            assert len(ref) == len(want) and (ref == want).all()
