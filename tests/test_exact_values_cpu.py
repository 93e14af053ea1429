"""tests/exact_values.py without a GPU: the exact roundings against numpy's casts and division (which pins numpy as a yardstick
at this range), the exact column against repr_restate.column_values on the whole hostile list (after which every restatement
under tests/ may be used on that list unchanged), the critical floats, the floors of every population the list promises, and the
sensitivity proof: each deliberately wrong column of exact_values.WRONG changes an observable of every family of consumers, as
the restatements compute it, on this very list."""
from fractions import Fraction

import numpy as np
import pytest

import ani_restate
import cut_restate as cr
import derep_restate as dr
import exact_values as xv
import repr_restate as rr
import tree_restate as tr
from kspider_amd import engine

TRUE = rr.column_values          # (the sensitivity proof puts other functions in its place for a while)


@pytest.fixture(scope="module")
def hostile():
    return xv.hostile_edges(1)


def _bits(a):
    return xv.bits_of(a).tolist()


# ---- the roundings against numpy -----------------------------------------------------------------------------------------------

def test_f32_of_int_equals_the_numpy_cast():
    rng = np.random.default_rng(1)
    named = list(xv.NAMED_COUNTS + xv.EXACT_COUNTS + xv.NAMED_SHARED) + [2**24 - 1, 2**24 + 2, 2**25 + 1, 2**25 + 3, 2**53 + 1, 2**64 - 2**39, 2**64 - 2**39 - 1]
    wide = rng.integers(0, 1 << 64, size=50_000, dtype=np.uint64)
    narrow = rng.integers(0, 1 << 64, size=50_000, dtype=np.uint64) >> rng.integers(0, 64, size=50_000).astype(np.uint64)   # every magnitude
    v = np.concatenate([np.array(named, dtype=np.uint64), wide, narrow])
    assert [xv.f32_of_int(x) for x in v.tolist()] == _bits(v.astype(np.float32))
    assert xv.f32_of_int(2**24 + 1) == xv.f32_of_int(2**24) and xv.f32_of_int(2**24 + 3) == xv.f32_of_int(2**24 + 4)       # ties, to even both ways
    assert xv.f32_of_int(2**32 - 1) == xv.f32_of_int(2**32) and xv.f32_of_int(2**64 - 1) == xv.f32_of_int(2**63) + (1 << 23)
    through_double = xv.bits_of(np.array([2**63 + 2**39 + 1], dtype=np.uint64).astype(np.float64).astype(np.float32))[0]
    assert xv.f32_of_int(2**63 + 2**39 + 1) == through_double + 1                       # 2^63 + 2^39 + 1: a double drops the 1, and what is left is a tie that goes down


def test_f32_div_equals_numpy_division():
    rng = np.random.default_rng(2)
    a = rng.integers(0, xv.INF + 1, size=50_000, dtype=np.uint32)                       # every non-negative float, +inf and subnormals included
    b = rng.integers(0, xv.INF + 1, size=50_000, dtype=np.uint32)
    a[:8], b[:8] = [0, 1, 0, xv.INF, xv.INF, 5, 0x3F800000, 1], [0, 0, 7, xv.INF, 3, xv.INF, 3, 0x7F7FFFFF]
    # and the range of the columns: integers below 2^64 as floats over counts as floats
    ai = (rng.integers(0, 1 << 64, size=50_000, dtype=np.uint64) >> rng.integers(0, 64, size=50_000).astype(np.uint64)).astype(np.float32)
    bi = rng.integers(0, 1 << 32, size=50_000, dtype=np.uint64).astype(np.float32)
    a, b = np.concatenate([a, ai.view(np.uint32)]), np.concatenate([b, bi.view(np.uint32)])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        want = _bits(a.view(np.float32) / b.view(np.float32))
    assert [xv.f32_div(x, y) for x, y in zip(a.tolist(), b.tolist())] == want
    assert xv.f32_div(0, 0) == xv.NAN and xv.f32_div(5, 0) == xv.INF


def test_the_exact_column_equals_the_numpy_restatement_on_the_hostile_list(hostile):
    for col in (3, 4, 5):
        assert xv.columns(hostile.edges, hostile.kmer_counts, col) == _bits(TRUE(hostile.edges, hostile.kmer_counts, col)), col
    # the NaN asymmetry of std::min / std::max: a NaN c12 (= shared / n2) wins, a NaN c21 loses
    assert [xv.column(0, 9, 0, c) for c in (3, 4, 5)] == [xv.NAN, xv.NAN, xv.NAN]
    assert [xv.column(0, 0, 9, c) for c in (3, 4, 5)] == [0, xv.NAN, 0]
    assert [xv.column(4, 0, 8, c) for c in (3, 4, 5)] == [0x3F000000, xv.INF, xv.INF]


def test_critical_floats():
    assert xv.critical_cc(0.2) == 0x3E4CCCAC and xv.text(0x3E4CCCAC) == "0.2" and xv.text(0x3E4CCCAB) == "0.199999"
    assert xv.critical_repr(0.20) == 0x3E4CCCAC                                          # what tests/test_repr_cpu.py pins for ksp_repr_critical
    assert xv.text(xv.critical_repr(0.5)) == "0.500001" and xv.text(xv.critical_cc(0.5)) == "0.5"
    assert xv.critical_cc(-1.0) == 0 and xv.critical_repr(float("inf")) is None


# ---- what the hostile list promises ----------------------------------------------------------------------------------------------

def test_sizes_and_counts(hostile):
    C = xv.CUT_CHUNK_EDGES
    assert C == engine.CUT_CHUNK_EDGES == engine.SWEEP_CHUNK_EDGES == engine.TREE_CHUNK_EDGES == engine.DEREP_CHUNK_EDGES
    assert len(hostile.edges) == 3 * C + 17 and 550 <= len(hostile.kmer_counts) <= 650
    assert (hostile.edges["source_1"] < hostile.edges["source_2"]).all() and int(hostile.edges["source_2"].max()) == len(hostile.kmer_counts) - 1
    cnt = hostile.kmer_counts.tolist()
    for c in xv.NAMED_COUNTS + xv.EXACT_COUNTS:
        assert c in cnt, c
    for c in xv.NAMED_COUNTS:
        assert xv.frac(xv.f32_of_int(c)) != c
    assert sum(1 for c in cnt if c % 2 and 2**24 < c < 2**32 and c not in xv.NAMED_COUNTS) >= 200
    used = set(hostile.edges["source_1"].tolist()) | set(hostile.edges["source_2"].tolist())
    assert used == set(range(len(cnt)))                                                  # every count is some record's


def test_shared_populations(hostile):
    e, cnt = hostile.edges, hostile.kmer_counts
    sh = e["shared"].tolist()
    for s in xv.NAMED_SHARED:
        assert sh.count(s) >= 3, s
    low = np.minimum(cnt[e["source_1"]], cnt[e["source_2"]]).tolist()
    assert sum(1 for s, m in zip(sh, low) if 0 < s <= m) >= 3000
    assert sum(1 for s in sh if 2**24 < s < 2**32 and xv.frac(xv.f32_of_int(s)) != s) >= 1000
    assert (hostile.from_join == (e["shared"] < np.uint64(2**32))).all() and 100 <= int((~hostile.from_join).sum()) <= 400


def _away(c12, c21):
    """The two quotients differ by a tenth at least."""
    lo, hi = sorted((xv.frac(c12), xv.frac(c21)))
    return 10 * lo <= 9 * hi


def test_boundary_rows(hostile):
    e, cnt = hostile.edges, hostile.kmer_counts.tolist()
    assert hostile.cutoffs[:4] == list(xv.CUTOFFS) and len(hostile.cutoffs) == 5
    row = hostile.printed_row
    s, n1, n2 = int(e["shared"][row]), cnt[e["source_1"][row]], cnt[e["source_2"][row]]
    assert float(xv.text(xv.column(s, n1, n2, 5))) == hostile.cutoffs[4] and xv.critical_cc(hostile.cutoffs[4]) == xv.column(s, n1, n2, 5)
    quot = [xv.quotients(s, cnt[a], cnt[b]) for a, b, s in zip(e["source_1"].tolist(), e["source_2"].tolist(), e["shared"].tolist())]
    inexact = [xv.frac(xv.f32_of_int(cnt[a])) != cnt[a] and xv.frac(xv.f32_of_int(cnt[b])) != cnt[b] for a, b in zip(e["source_1"].tolist(), e["source_2"].tolist())]
    crit = {("cc", c): xv.critical_cc(c) for c in hostile.cutoffs}
    crit.update({("repr", t): xv.critical_repr(t) for t in xv.REPR_THRESHOLDS})
    for col in (3, 4, 5):
        vals = xv.columns(e, cnt, col)
        for what, c in crit.items():
            for target in (c, c - 1):
                assert xv.text(c) != xv.text(c - 1)
                rows = [i for i, v in enumerate(vals) if v == target and inexact[i] and (col == 4 or (not xv.is_nan(quot[i][0]) and quot[i][0] < xv.INF
                                                                                                   and quot[i][1] < xv.INF and _away(*quot[i])))]
                assert len(rows) >= 32, (col, what, hex(target), len(rows))
                if col == 4:
                    assert sum(quot[i][0] != quot[i][1] for i in rows) >= 24               # both quotients take part


def test_forest_pairs(hostile):
    e, cnt = hostile.edges, hostile.kmer_counts.tolist()
    degree = np.bincount(np.concatenate([e["source_1"], e["source_2"]]), minlength=len(cnt))
    pairs = {}
    for i, tag in enumerate(hostile.tags):
        if tag:
            pairs.setdefault(tag, []).append(i)
    found = {"same": 0, "ulp": 0, "double": 0}
    for (kind, _, col), (i, j) in pairs.items():
        rec = [(int(e["shared"][x]), cnt[e["source_1"][x]], cnt[e["source_2"][x]]) for x in (i, j)]
        assert rec[0] != rec[1] and (rec[0][0], rec[0][2], rec[0][1]) != rec[1]
        for x in (i, j):
            assert min(degree[e["source_1"][x]], degree[e["source_2"][x]]) == 1          # the only connection of a leaf: in every forest
        vi, vj = (xv.column(*r, col) for r in rec)
        assert abs(vi - vj) == (1 if kind == "ulp" else 0) and 0 < vi < xv.INF
        found[kind] += 1
    assert found["same"] >= 32 and found["ulp"] >= 32 and found["double"] == 1
    (i, j), = [p for t, p in pairs.items() if t[0] == "double"]
    assert i < j and i == hostile.printed_row                                            # a conversion through a double moves record i behind record j
    forest = set(tr.forest(len(cnt), e, hostile.kmer_counts, 5).tolist())
    assert all(i in forest for p in pairs.values() for i in p)


def test_nan_inf_and_ani_rows(hostile):
    e, cnt = hostile.edges, hostile.kmer_counts.tolist()
    kinds = {"c12": 0, "c21": 0, "both": 0, "inf": 0}
    for a, b, s in zip(e["source_1"].tolist(), e["source_2"].tolist(), e["shared"].tolist()):
        c12, c21 = xv.quotients(s, cnt[a], cnt[b])
        if xv.is_nan(c12) or xv.is_nan(c21):
            kinds["both" if xv.is_nan(c12) and xv.is_nan(c21) else "c12" if xv.is_nan(c12) else "c21"] += 1
        elif xv.INF in (c12, c21):
            kinds["inf"] += 1
    assert kinds["c12"] >= 4 and kinds["c21"] >= 4 and kinds["both"] >= 1 and kinds["inf"] >= 8, kinds
    col3, col5 = xv.columns(e, cnt, 3), xv.columns(e, cnt, 5)
    assert (hostile.nan_rows == np.array([xv.is_nan(a) or xv.is_nan(b) for a, b in zip(col3, col5)])).all() and 4 <= int(hostile.nan_rows.sum()) <= 64
    finite = [v for v in col3 + col5 if not xv.is_nan(v) and v < xv.INF]
    ties = {v for v in finite if Fraction(1, 10) <= xv.frac(v) < 1 and (xv.frac(v) * 10**6) % 1 == Fraction(1, 2)}
    assert len(ties) >= 15 and xv._round(Fraction(13, 128)) in ties                      # 0.1015625 = 13 x 2^18 / 2^25
    for edge in (Fraction(1, 10000), Fraction(9999, 10000)):
        near = xv._round(edge)
        close = {v for v in finite if abs(v - near) <= 64}
        assert len(close) >= 6 and any(v < near for v in close) and any(v > near for v in close), (edge, len(close))


# ---- the sensitivity proof -------------------------------------------------------------------------------------------------------

FAMILIES = ("cut", "repr", "forest", "ani")
# The structurally impossible (variant, family) pairs; the test asserts that these show NO difference.
EXEMPT = {
    # (double)c12 + (double)c21 is exact whenever the two exponents are within 29 of each other, and where they are further apart the
    # smaller quotient is below a quarter ulp of the larger in either computation; halving is exact (no value here is below 2^-32 or
    # above 2^64): both orders round the same real number once.  test_the_double_average_is_the_same_function checks it.
    ("double_average", "cut"): "identical to the reference's average for every value a record can have",
    ("double_average", "repr"): "identical to the reference's average for every value a record can have",
    ("double_average", "forest"): "identical to the reference's average for every value a record can have",
    ("double_average", "ani"): "ANI reads columns 3 and 5 only",
    ("fmin_fmax", "ani"): "ANI refuses NaN rows",
    # a NaN quotient is 0 / 0, so shared = 0 and the other quotient is 0 (or a NaN): fminf / fmaxf put 0 where the NaN was, and
    # neither a NaN nor 0 passes a threshold above 0
    ("fmin_fmax", "repr"): "a NaN becomes 0, and neither passes 0.2 or 0.5",
    # a conversion through a double differs from the direct one only for shared >= 2^53: over a count below 2^32 that is a value
    # of 2^21 at least, which passes every threshold and is an ANI of 1 either way
    ("shared_through_double", "repr"): "differs only where the value is 2^21 or more",
    ("shared_through_double", "ani"): "differs only where the value is 2^21 or more",
}


def _observables(h, monkeypatch, values):
    """Per family the observables of the restatements, with `values` in place of their column function."""
    for mod in (cr, rr, tr):
        monkeypatch.setattr(mod, "column_values", values)
    e, cnt, n = h.edges, h.kmer_counts, len(h.kmer_counts)
    out = {"cut": [cr.edge_mask(e, cnt, col, c).tolist() for col in (3, 4, 5) for c in h.cutoffs],
           "repr": [dr.kept_records(e, cnt, col, t) for col in (3, 4, 5) for t in xv.REPR_THRESHOLDS],
           "forest": [tr.forest(n, e, cnt, col).tolist() for col in (3, 4, 5)]}
    ok = e[~h.nan_rows]
    out["ani"] = [[ani_restate.ani_of_floats(a, b, k) for a, b in zip(values(ok, cnt, 3).tolist(), values(ok, cnt, 5).tolist())] for k in (21, 31)]
    return out


def test_every_wrong_column_changes_every_family(hostile, monkeypatch):
    want = _observables(hostile, monkeypatch, TRUE)
    assert set(EXEMPT) <= {(v, f) for v in xv.WRONG for f in FAMILIES}
    for name, values in xv.WRONG.items():
        got = _observables(hostile, monkeypatch, values)
        for family in FAMILIES:
            assert (got[family] == want[family]) == ((name, family) in EXEMPT), (name, family)


def test_the_double_average_is_the_same_function(hostile):
    """Why ("double_average", *) is exempt: on the list and on 10^5 random records the variant equals the reference's average bit for bit."""
    rng = np.random.default_rng(3)
    e = np.zeros(100_000, dtype=xv.EDGE_DTYPE)
    e["source_1"], e["source_2"] = rng.integers(0, 1000, size=len(e)), rng.integers(0, 1000, size=len(e))
    e["shared"] = rng.integers(0, 1 << 64, size=len(e), dtype=np.uint64) >> rng.integers(0, 64, size=len(e)).astype(np.uint64)
    cnt = (rng.integers(0, 1 << 32, size=1000, dtype=np.uint64) >> rng.integers(0, 32, size=1000).astype(np.uint64)).astype(np.uint32)
    for edges, counts in ((hostile.edges, hostile.kmer_counts), (e, cnt)):
        assert _bits(xv.WRONG["double_average"](edges, counts, 4)) == _bits(TRUE(edges, counts, 4))
