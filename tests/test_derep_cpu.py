"""The dereplication's definition without a GPU: the restatement of tests/derep_restate.py on hand-written
graphs with hand-written answers, the four consequences as predicates on random graphs, the file renderer, and the shapes of
the inputs tests/test_derep_gpu.py hands to the device — the live-pair counts of its tail cases by the round simulation of
tests/derep_inputs.py, its boundary floats, and what its hostile multigraphs plant: repeated pairs in both orientations whose first
copy is dropped, self pairs, ends out of range, nodes of 0 k-mers, stars whose centres tie."""
import numpy as np
import pytest

import derep_inputs as di
import derep_restate as dr
import repr_restate as rr
from kspider_amd import engine

NONE = dr.NONE


def _run(n, e, cnt=None, col=4, threshold=0.20):
    cnt = di.same(n) if cnt is None else cnt
    res = dr.dereplicate(e, cnt, col, threshold, n)
    di.consequences(n, e, np.array(dr.kept_records(e, cnt, col, threshold, n), dtype=np.int64), res)
    return res


def test_star_and_two_stars_whose_centres_share_a_record():
    res = _run(6, di.star(5))
    assert res["rep"].tolist() == [0] * 6 and res["n_reps"] == 1 and res["via"].tolist() == [NONE, 0, 1, 2, 3, 4]
    assert res["rank"].tolist() == [0, 1, 2, 3, 4, 5] and res["degree"].tolist() == [5, 1, 1, 1, 1, 1]
    # centre 0 with leaves 2, 3, 4, 5 and centre 1 with leaves 6, 7, 8; the record 0 - 1 joins the centres: degrees 5 and 4
    e = di.edges([0, 0, 0, 0, 1, 1, 1, 0], [2, 3, 4, 5, 6, 7, 8, 1])
    res = _run(9, e)
    assert res["degree"].tolist()[:2] == [5, 4]
    assert res["rep"].tolist() == [0, 0, 0, 0, 0, 0, 6, 7, 8]            # the other centre is a member, its leaves stand for themselves
    assert res["via"].tolist()[1] == 7 and res["n_reps"] == 4


def test_triangle_of_equal_degrees_and_path_of_7():
    res = _run(3, di.edges([0, 1, 0], [1, 2, 2]))
    assert res["rep"].tolist() == [0, 0, 0] and res["via"].tolist() == [NONE, 0, 2]
    # a path of 7: the inner nodes (degree 2) rank before the ends; 1 is IN, 2 OUT, 3 IN, 4 OUT, 5 IN; the ends 0 and 6 are OUT
    res = _run(7, di.path(7))
    assert res["rank"].tolist() == [5, 0, 1, 2, 3, 4, 6]
    assert res["rep"].tolist() == [1, 1, 1, 3, 3, 5, 5] and res["n_reps"] == 3
    for order in ("reversed", "random"):
        assert _run(7, di.path(7, order))["rep"].tolist() == res["rep"].tolist()


def test_later_smaller_ranked_representative():
    n, e = di.later_smaller_rep()
    L = di.LATER
    res = _run(n, e)
    assert [int(res["rank"][L[k]]) for k in ("c1", "c2", "u2", "u1", "h")] == [0, 1, 2, 3, 4]
    assert res["rep"][L["c2"]] == L["c1"] and res["rep"][L["u2"]] == L["u2"] and res["rep"][L["u1"]] == L["u1"]
    assert res["rep"][L["h"]] == L["u2"] and res["via"][L["h"]] == 1
    # in the rounds u1 is IN first and u2 only later: the assignment cannot be made when h is knocked out
    is_rep, lives = di.simulate_rounds(n, list(zip(e["source_1"].tolist(), e["source_2"].tolist())))
    assert is_rep == (res["rep"] == np.arange(n)).tolist() and len(lives) >= 3


def test_repeats_and_self_pairs():
    # the pair 0 - 1 three times with different `shared`, the first one dropped: via is the lowest KEPT index
    e = di.edges([0, 1, 0, 0], [1, 0, 1, 2], [di.DROP, di.KEEP, di.KEEP + 5, di.KEEP])
    res = _run(3, e)
    assert res["degree"].tolist() == [3, 2, 1] and res["rep"].tolist() == [0, 0, 0] and res["via"].tolist() == [NONE, 1, 3]
    # self pairs add 2 to the degree and take no part: node 2 ranks first on its self pairs alone and is a representative
    e = di.edges([2, 2, 0, 2], [2, 2, 1, 1])
    res = _run(3, e)
    assert res["degree"].tolist() == [1, 2, 5] and res["rep"].tolist() == [0, 2, 2]
    res = _run(3, di.edges([1, 2], [1, 2]))
    assert res["rep"].tolist() == [0, 1, 2] and res["n_reps"] == 3 and res["degree"].tolist() == [0, 2, 2]
    # an endpoint >= n_nodes: the record is ignored
    res = _run(3, di.edges([0, 1], [7, 2]))
    assert res["degree"].tolist() == [0, 1, 1] and res["rep"].tolist() == [0, 1, 1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_consequences_and_order_independence_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n, m = 300, 1500
    cnt = rng.integers(3000, 4001, size=n).astype(np.uint32)
    s1, s2 = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    e = di.edges(s1, s2, (rng.uniform(0.05, 0.4, size=m) * 3000).astype(np.uint64))
    for col in (3, 4, 5):
        res = _run(n, e, cnt, col)
        assert 1 < res["n_reps"] < n
        e2, p = di.permuted(e, seed)
        res2 = _run(n, e2, cnt, col)
        for k in ("rep", "rank", "degree"):
            assert (res[k] == res2[k]).all(), k
        members = res["rep"] != np.arange(n)
        pair = lambda ee, i: {int(ee["source_1"][i]), int(ee["source_2"][i])}
        assert all(pair(e, res["via"][v]) == pair(e2, res2["via"][v]) for v in np.nonzero(members)[0])
        is_rep, _ = di.simulate_rounds(n, [(int(e["source_1"][i]), int(e["source_2"][i])) for i in dr.kept_records(e, cnt, col, 0.20, n)])
        assert is_rep == (~members).tolist()


def test_file_renderer():
    names = ["a", "b", "c", "d", "e"]
    tsv = "source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n" \
          "1\t2\t5\t0.1\t0.3\t0.5\n1\t3\t5\t0.1\t0.25\t0.5\n2\t3\t1\t0.01\t0.2\t0.5\n4\t5\t2\t0.3\t0.200001\t0.1\n"
    want = "source\trepresentative\tavg_cont\tneighbours\trank\n" \
           "a\ta\t-\t2\t0\nb\ta\t0.3\t2\t1\nc\ta\t0.25\t2\t2\nd\td\t-\t1\t3\ne\td\t0.200001\t1\t4\n"
    assert dr.dereplicated_tsv(tsv, names).decode() == want               # (the row 2 - 3 passes too: "0.2" reads as 0.2f > 0.20)
    # min_cont at 0.2: only the row 4 - 5 passes
    got = dr.dereplicated_tsv(tsv, names, 3, 0.2, "min_cont").decode().split("\n")
    assert got[1] == "a\ta\t-\t0\t2" and got[4] == "d\td\t-\t1\t0" and got[5] == "e\td\t0.3\t1\t1"


def test_shapes_of_the_gpu_inputs():
    """What tests/test_derep_gpu.py relies on: the live pairs of the tail cases after the first round, the rounds of a path,
    and the boundary floats."""
    K = engine.DEREP_TAIL_PAIRS
    assert K == 65536 and engine.DEREP_CHUNK_EDGES == 2048
    for total in (K - 1, K, K + 1):
        n, e = di.disjoint_paths(total)
        assert len(e) == total and (e["source_1"] != e["source_2"]).all() and int(max(e["source_2"])) == n - 1
    n, e = di.disjoint_paths(100, 8)
    _, lives = di.simulate_rounds(n, list(zip(e["source_1"].tolist(), e["source_2"].tolist())))
    assert lives[0] == 100 and lives[-1] == 0 and all(x >= y for x, y in zip(lives, lives[1:]))
    for order in ("ascending", "reversed", "random"):
        e = di.path(300, order)
        _, lives = di.simulate_rounds(300, list(zip(e["source_1"].tolist(), e["source_2"].tolist())))
        assert len(lives) > 100 and lives[0] == 299
    for col in (3, 4, 5):
        cnt, e = di.boundary_case(col)
        assert (cnt[e["source_1"][:2]] != cnt[e["source_2"][:2]]).all()
        vals = rr.column_values(e, cnt, col)
        assert ["%.6g" % v for v in vals.tolist()][:3] == ["0.2", "0.199999", "nan"], col
        assert vals[0] < np.float32(0.2) and vals[3] >= 0.5
        assert dr.kept_records(e, cnt, col, 0.20) == [0, 3]


C = engine.DEREP_CHUNK_EDGES
HOSTILE_SIZES = ((700, 3 * C - 7), (20000, 2 * C + 1))           # (nodes, records) of tests/test_derep_gpu.py


@pytest.mark.parametrize("n_nodes,n_records", HOSTILE_SIZES)
def test_hostile_multigraph_plants_what_it_says(n_nodes, n_records):
    e, cnt, meta = di.hostile(11, n_nodes, n_records)
    e_again, cnt_again, _ = di.hostile(11, n_nodes, n_records)
    assert len(e) == n_records and (e == e_again).all() and (cnt == cnt_again).all() and (di.hostile(12, n_nodes, n_records)[0] != e).any()
    s1, s2 = e["source_1"].astype(np.int64), e["source_2"].astype(np.int64)
    outside = (s1 >= n_nodes) | (s2 >= n_nodes)
    assert 0.008 * n_records <= outside.sum() == meta["n_outside"] <= 0.012 * n_records
    assert (s1 == 0xFFFFFFFF).any() and (s2 == 0xFFFFFFFF).any() and (s1 == n_nodes).any() and (s2 == n_nodes).any()
    assert not ((s1 >= n_nodes) & (s2 >= n_nodes)).any()
    selfs = np.nonzero((s1 == s2) & ~outside)[0]
    assert 0.018 * n_records <= meta["n_self"] <= len(selfs) <= 0.03 * n_records       # (the random records add a few)
    assert len(meta["zero"]) >= 20 and (cnt[meta["zero"]] == 0).all() and (cnt == 0).sum() == len(meta["zero"])
    where = {}
    for i, (a, b) in enumerate(zip(s1.tolist(), s2.tolist())):
        where.setdefault((min(a, b), max(a, b)), []).append(i)
    assert len(meta["repeated"]) == len(set(meta["repeated"])) >= 200
    for col in (3, 4, 5):
        kept = dr.kept_records(e, cnt, col, 0.20, n_nodes)
        kept_set = set(kept)
        assert any(i in kept_set for i in selfs.tolist()) and any(i not in kept_set for i in selfs.tolist())
        vals = rr.column_values(e[~outside], cnt, col)
        assert np.isinf(vals).any() and np.isnan(vals).any()
        first_dropped = 0
        for pair in meta["repeated"]:
            idx = where[pair]
            flags = [i in kept_set for i in idx]
            assert 2 <= len(idx) <= 6 and True in flags and False in flags, pair
            assert len({(int(s1[i]), int(s2[i])) for i in idx}) == 2                     # both orientations
            assert len({int(e["shared"][i]) for i in idx}) == len(idx)                   # every copy its own `shared`
            first_dropped += not flags[0]
        assert first_dropped >= 50 and all(where[p][0] not in kept_set for p in meta["first_dropped"])
        # the stars: no other record names their nodes, every centre has its 5 leaves and 2 ring neighbours, the ranks follow the ids
        res = dr.dereplicate(e, cnt, col, 0.20, n_nodes)
        di.consequences(n_nodes, e, np.array(kept, dtype=np.int64), res)
        centres = meta["centres"]
        assert len(centres) == 30 and centres == sorted(centres) and (res["degree"][centres] == 7).all()
        assert (np.diff(res["rank"][centres].astype(np.int64)) > 0).all()
        assert (res["degree"][sorted(set(meta["star_nodes"]) - set(centres))] == 1).all()
        assert 1 < res["n_reps"] < n_nodes and len(kept) > n_records // 4
    # copies of one pair in different 512-entry wave ranges and in different chunks
    assert sum(len({i // 512 for i in where[p]}) > 1 for p in meta["repeated"]) >= 150
    assert sum(len({i // C for i in where[p]}) > 1 for p in meta["repeated"]) >= 100


@pytest.mark.parametrize("n_nodes,n_records", HOSTILE_SIZES)
def test_hostile_multigraph_permuted(n_nodes, n_records):
    e, cnt, _ = di.hostile(11, n_nodes, n_records)
    e2, _ = di.permuted(e, 3)
    for col in (3, 4, 5):
        res, res2 = dr.dereplicate(e, cnt, col, 0.20, n_nodes), dr.dereplicate(e2, cnt, col, 0.20, n_nodes)
        kept2 = dr.kept_records(e2, cnt, col, 0.20, n_nodes)
        di.consequences(n_nodes, e2, np.array(kept2, dtype=np.int64), res2)
        di.via_after_permutation(e2, kept2, res, res2)
        assert (res["via"] != res2["via"]).any()
