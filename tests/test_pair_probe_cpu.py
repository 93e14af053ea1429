"""tests/pair_probe.py itself: the key side of the pair-matrix fingerprint agrees with the restated reference on seeded small
sets (unweighted, and with per-key weights), and every kind of wrong edge set is reported — among them a 4-cycle of +-1
that keeps the total and every row sum, so that only the random probes see it."""
import numpy as np
import pytest

import oracle
from kspider_amd import synth
from pair_probe import check_edge_set, edge_fingerprint, edge_rows, key_fingerprint, key_index, key_rows

TOP = (1 << 64) - 1


def _small_set(seed, n, universe=300, lo=0, hi=60, extremes=True):
    """n sources drawn from a small universe (many shared keys); keys 0 and 2^64 - 1 are in it, some sources empty."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(1, TOP, universe, dtype=np.uint64, endpoint=False)
    if extremes:
        pool[:2] = (0, TOP)
    runs = []
    for _ in range(n):
        m = int(rng.integers(lo, hi + 1))
        runs.append(rng.choice(pool, size=min(m, universe), replace=False))
    return synth.from_runs(runs, "probe")


CASES = [(1, 0), (2, 1), (3, 2), (4, 127), (5, 128), (6, 129), (7, 40), (8, 200)]


@pytest.mark.parametrize("seed,n", CASES)
def test_brute_pairs_pass_unweighted(oracle_lib, seed, n):
    sk = _small_set(seed, n)
    idx = key_index(sk.keys, sk.offsets, threads=3)
    ref = oracle_lib.brute_pairs(sk.keys, sk.offsets)
    check_edge_set(ref, idx, n, probes=3, seed=seed)
    # the identity for arbitrary vectors, and the rows / total
    rng = np.random.default_rng(seed + 100)
    for _ in range(3):
        u = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        v = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        assert key_fingerprint(idx, u, v) == edge_fingerprint(ref, u, v)
    rows, total = key_rows(idx)
    assert (rows == edge_rows(ref, n)).all() and total == int(ref["shared"].sum())


def test_empty_input_and_extreme_keys(oracle_lib):
    sk = synth.from_runs([[], [0, TOP], [TOP], [], [0, 5, TOP]])
    idx = key_index(sk.keys, sk.offsets)
    assert idx.keys.tolist() == [0, TOP] and idx.counts.tolist() == [2, 3]
    assert idx.holders_of(np.array([0, 5, TOP, 7], dtype=np.uint64)).tolist() == [2, 1, 3, 1]
    ref = oracle_lib.brute_pairs(sk.keys, sk.offsets)
    assert [tuple(e) for e in ref.tolist()] == [(1, 2, 1), (1, 4, 2), (2, 4, 1)]
    check_edge_set(ref, idx)
    sk0 = synth.from_runs([])
    check_edge_set(np.zeros(0, dtype=oracle.EDGE_DTYPE), key_index(sk0.keys, sk0.offsets))


def test_a_key_held_twice_by_one_source_is_refused():
    keys = np.array([3, 3, 4], dtype=np.uint64)
    with pytest.raises(RuntimeError, match="holds key 3 twice"):
        key_index(keys, np.array([0, 2, 3], dtype=np.uint64))


@pytest.mark.parametrize("seed,n", CASES)
def test_accumulate_mem_passes_with_per_key_weights(oracle_lib, seed, n):
    """Per-key weights: the colour index of the restated reference, every colour weighing the sum of its keys' weights."""
    sk = _small_set(seed, n)
    idx = key_index(sk.keys, sk.offsets, threads=2)
    rng = np.random.default_rng(seed + 7)
    w = rng.integers(1, 1001, idx.keys.size).astype(np.uint32)
    co, src, cw = oracle_lib.build_colors(sk.keys, sk.offsets)
    colour_of = {tuple((src[co[c]:co[c + 1]] - 1).tolist()): c for c in range(cw.size)}
    cw = np.zeros(cw.size, dtype=np.uint32)
    for k in range(idx.keys.size):
        cw[colour_of[tuple(idx.sources[idx.key_off[k]:idx.key_off[k + 1]].tolist())]] += w[k]
    _, _, _, ref = oracle_lib.accumulate_mem(co, src, cw, 2)
    ref = np.sort(ref, order=["source_1", "source_2"])
    ref["source_1"] -= 1
    ref["source_2"] -= 1
    check_edge_set(ref, idx, n, w=w, seed=seed)
    # and the unweighted expectation does not pass it (unless there is nothing to weigh)
    if idx.keys.size and (w > 1).any():
        with pytest.raises(AssertionError):
            check_edge_set(ref, idx, n, seed=seed)


# ---- corruptions ----------------------------------------------------------------------------------------------------

def _dense(seed):
    """40 sources of 40..70 keys out of 120: almost every pair shares several keys."""
    sk = _small_set(1000 + seed, 40, universe=120, lo=40, hi=70, extremes=seed % 2 == 0)
    return sk, key_index(sk.keys, sk.offsets), oracle.brute_pairs(sk.keys, sk.offsets)


def _resort(e):
    return np.sort(e, order=["source_1", "source_2"])


def _corrupt(kind, e, rng, n):
    e = e.copy()
    i = int(rng.integers(len(e)))
    if kind == "plus_one":
        e["shared"][i] += 1
    elif kind == "minus_one":
        e["shared"][i] -= 1
    elif kind == "dropped":
        e = np.delete(e, i)
    elif kind == "spurious":
        present = set(zip(e["source_1"].tolist(), e["source_2"].tolist()))
        absent = [(a, b) for a in range(n) for b in range(a + 1, n) if (a, b) not in present]
        if not absent:   # every pair shares something: make room for one
            a, b = int(e["source_1"][i]), int(e["source_2"][i])
            e = np.delete(e, i)
        else:
            a, b = absent[int(rng.integers(len(absent)))]
        e = _resort(np.concatenate([e, np.array([(a, b, 1)], dtype=e.dtype)]))
    elif kind == "moved":
        a, b = int(e["source_1"][i]), int(e["source_2"][i])
        e["source_2"][i] = b + 1 if b + 1 < n and (b - 1 <= a or rng.integers(2)) else b - 1
        e = _resort(e)
    elif kind == "swapped":
        j = int(rng.choice(np.flatnonzero(e["shared"] != e["shared"][i])))
        e["shared"][i], e["shared"][j] = e["shared"][j], e["shared"][i]
    elif kind == "split":
        i = int(rng.choice(np.flatnonzero(e["shared"] >= 2)))
        s = int(e["shared"][i])
        e["shared"][i] = 1
        e = _resort(np.concatenate([e, np.array([(e["source_1"][i], e["source_2"][i], s - 1)], dtype=e.dtype)]))
    elif kind == "reversed":
        e["source_1"][i], e["source_2"][i] = e["source_2"][i], e["source_1"][i]
    elif kind == "four_cycle":
        e = _four_cycle(e, rng)
    return e


def _four_cycle(e, rng):
    """+1 on (a, b) and (c, d), -1 on (a, d) and (c, b): four distinct sources, every row sum and the total kept."""
    pos = {(int(x), int(y)): k for k, (x, y) in enumerate(zip(e["source_1"], e["source_2"]))}
    n = int(e["source_2"].max()) + 1
    while True:
        a, b, c, d = (int(x) for x in rng.choice(n, size=4, replace=False))
        p = [pos.get(tuple(sorted(q))) for q in ((a, b), (c, d), (a, d), (c, b))]
        if None in p or e["shared"][p[2]] < 2 or e["shared"][p[3]] < 2:
            continue
        e = e.copy()
        e["shared"][p[0]] += 1
        e["shared"][p[1]] += 1
        e["shared"][p[2]] -= 1
        e["shared"][p[3]] -= 1
        return e


KINDS = ["plus_one", "minus_one", "dropped", "spurious", "moved", "swapped", "split", "reversed", "four_cycle"]


@pytest.mark.parametrize("kind", KINDS)
def test_every_corruption_is_reported(kind):
    messages = set()
    for seed in range(24):
        sk, idx, ref = _dense(seed)
        check_edge_set(ref, idx, seed=seed)
        bad = _corrupt(kind, ref, np.random.default_rng([seed, KINDS.index(kind)]), sk.n_sources)
        with pytest.raises(AssertionError) as ei:
            check_edge_set(bad, idx, seed=seed)
        messages.add(str(ei.value).split(":")[0])
    if kind == "four_cycle":
        assert all(m.startswith("probe") for m in messages), messages   # (nothing else can see it)


def test_the_four_cycle_passes_every_property_but_the_probes():
    """The gap the probes close: the 4-cycle keeps order, uniqueness, shared > 0, shared <= min(n_a, n_b), the total and
    every row sum — all that the full-size tests asserted before (on all rows, not 300 sampled ones) — and the sampled pairs
    of those tests hit one of its four edges with probability ~4 * 300 / #edges.  Only u^T S v tells it apart."""
    for seed in range(24):
        sk, idx, ref = _dense(seed)
        bad = _four_cycle(ref, np.random.default_rng(seed))
        assert (bad["shared"] != ref["shared"]).sum() == 4
        assert int(bad["shared"].sum()) == int(ref["shared"].sum())
        assert (edge_rows(bad, sk.n_sources) == edge_rows(ref, sk.n_sources)).all()
        check_edge_set(bad, idx, probes=0, seed=seed)            # the properties alone pass it
        with pytest.raises(AssertionError, match="^probe 0"):
            check_edge_set(bad, idx, probes=2, seed=seed)
