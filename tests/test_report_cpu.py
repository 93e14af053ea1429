"""The cluster report without a GPU: the restatement (tests/report_restate.py) against hand-written answers on graphs of at most
6 nodes, the stated properties of every input builder of tests/report_inputs.py, the struct sizes and the four symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import report_inputs as ri
import report_restate as rs
import repr_restate as rr
from kspider_amd import engine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kspider_amd.h")
UNIT = 1 << 30          # (the hand-written strengths count quarters)


@pytest.mark.parametrize("name", sorted(ri.SMALL))
def test_the_restatement_against_hand_written_answers(name):
    n, a, b, v, want = ri.SMALL[name]
    assert n <= 6
    cluster, member = rs.report(n, a, b, v)
    assert member["label"].tolist() == want["label"] and member["degree"].tolist() == want["degree"]
    assert member["strength"].tolist() == [s * UNIT for s in want["strength"]]
    assert member["via"].tolist() == [rs.NONE if x is None else x for x in want["via"]] and (member["reserved"] == 0).all()
    assert len(cluster) == len(want["cluster"])
    for c, (root, size, edges, nans, sum_q, lo, hi, medoid, covered) in zip(cluster, want["cluster"]):
        assert (int(c["root"]), int(c["size"]), int(c["edges"]), int(c["nan_edges"]), int(c["sum_q"])) == (root, size, edges, nans, sum_q * UNIT)
        assert (int(c["medoid"]), int(c["covered"])) == (medoid, covered)
        for got, w in ((c["min"], lo), (c["max"], hi)):
            assert (np.isnan(got) and w != w) or float(got) == w
    # the same graph as records gives the same answer in every column
    e, cnt, n_nodes = ri.small_records(name)
    for col in (3, 4, 5):
        rs.same(rs.report_edges(e, cnt, col, 0.0, n_nodes), (cluster, member), (name, col))


def test_small_graph_stories():
    assert rs.report(*ri.SMALL["path3"][:4])[0]["medoid"].tolist() == [1]                  # the middle of a path of 3
    assert rs.report(*ri.SMALL["clique4"][:4])[0]["medoid"].tolist() == [0]                # equal values: the smallest node
    _, m = rs.report(*ri.SMALL["two_equal"][:4])
    assert m["strength"][1] == m["strength"][2] == m["strength"].max()                     # two equal strengths
    c, _ = rs.report(*ri.SMALL["nan_only"][:4])
    assert c["edges"][0] == c["nan_edges"][0] == 2 and np.isnan(c["min"][0]) and np.isnan(c["max"][0])
    assert set(zip(ri.SMALL["repeated"][1][:3], ri.SMALL["repeated"][2][:3])) == {(0, 1), (1, 0)}   # both orientations


def test_q_is_the_floor_by_integer_arithmetic():
    assert rs.q_exact(1.0) == 1 << 32 and rs.q_exact(0.5) == 1 << 31 and rs.q_exact(0.0) == 0
    assert rs.q_exact(np.float32(2.0**-20)) == 1 << 12
    v = np.float32(1) / np.float32(3072)
    exact = rs.q_exact(v)
    assert exact * 2.0**-32 < float(v) and (exact + 1) * 2.0**-32 > float(v)              # truncated: v * 2^32 is no integer
    assert exact == int(float(v) * 4294967296.0)                                           # (the header's formula)
    for x in np.random.default_rng(1).random(200).astype(np.float32).tolist() + [2.0**-8, 2.0**-9 * 1.5, 1e-30]:
        assert rs.q_exact(x) == int(float(np.float32(x)) * 4294967296.0)


def test_input_builders():
    C = engine.REPORT_CHUNK_EDGES
    assert ri.CHUNK == C and ri.PATH_SIZES == [1, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 + 1]
    for n in ri.PATH_SIZES:
        e, cnt, n_nodes = ri.path_case(n)
        assert len(e) == n and n_nodes == n + 1 and (e["source_2"] == e["source_1"] + 1).all() and len(cnt) == n_nodes
    for first in (True, False):
        e, cnt, n_nodes = ri.star_case(first)
        centre = e["source_1"] if first else e["source_2"]
        assert len(e) == 5000 > 2 * C and (centre == 0).all() and n_nodes == 5001
        c, m = rs.report_edges(e, cnt, 5, 0.0, n_nodes)
        assert c["medoid"].tolist() == [0] and c["covered"].tolist() == [5000]
    e, cnt, n_nodes = ri.clique_case()
    assert len(e) == 2415 == 70 * 69 // 2 and C < len(e) < 2 * C
    assert (np.lexsort((e["source_2"], e["source_1"])) == np.arange(len(e))).all()        # ascending
    e2, cnt2, n2, part = ri.clique_and_paths()
    assert len(e2) == 2415 + 80 and n2 == 70 + 90 and len(part) == 2415
    assert sorted(map(tuple, part.tolist())) == sorted(map(tuple, e.tolist())) and part.tolist() != e.tolist()
    c, _ = rs.report_edges(e2, cnt2, 5, 0.0, n2)
    assert sorted(c["size"].tolist()) == [9] * 10 + [70]


def test_hostile_stays_hostile_inside_the_domain():
    e, cnt, meta = ri.hostile()
    n_nodes = 20000
    assert len(e) == 2 * ri.CHUNK + 1 and len(cnt) == n_nodes
    inside = (e["source_1"] < n_nodes) & (e["source_2"] < n_nodes)
    assert (~inside).sum() >= 4 and (e["source_1"] == e["source_2"]).sum() >= 2
    for col in (3, 4, 5):
        v = rr.column_values(e[inside], cnt, col)
        assert np.isnan(v).any() and not (v[~np.isnan(v)] > 1).any()
        assert rs.report_edges(e, cnt, col, 0.2, n_nodes) is not None
    pairs = {}
    for a, b in zip(e["source_1"].tolist(), e["source_2"].tolist()):
        pairs.setdefault((min(a, b), max(a, b)), set()).add(a < b)
    assert sum(1 for k in meta["repeated"] if pairs[k] == {True, False}) == len(meta["repeated"])   # both orientations
    o = ri.orders(e)
    assert o["ascending"].tolist() == o["reversed"][::-1].tolist() and sorted(map(tuple, o["shuffled"].tolist())) == sorted(map(tuple, o["ascending"].tolist()))
    assert o["shuffled"].tolist() != o["ascending"].tolist()


def test_specials_boundary_quantised_and_domain_inputs():
    e, cnt, n, notes = ri.specials()
    assert all(e["source_1"][i] == e["source_2"][i] for i in notes["self_pairs"])
    assert all(max(e["source_1"][i], e["source_2"][i]) >= n for i in notes["outside"])
    v = rr.column_values(e[:11], cnt, 5)
    assert np.isnan(v[[5, 6, 7]]).all() and v[4] > 1 and np.isinf(v[10])                   # the self pairs above 1 are no refusal
    for cutoff, zero_kept in ((0.0, True), (0.2, False)):
        c, m = rs.report_edges(e, cnt, 5, cutoff, n)
        assert (m["label"][[9, 10, 11]].tolist() == [9, 9, 9]) == zero_kept                # value 0: kept only at cut-off 0
        nan = c[c["root"] == 6][0]
        assert nan["size"] == 3 and nan["edges"] == nan["nan_edges"] == 2                  # one cluster of NaN records alone
        assert m["degree"][0] == 3 and m["degree"][2] == 1                                 # the repeated pair counts again; self and outside do not
    e, cnt, cutoff = ri.boundary()
    v = rr.column_values(e, cnt, 5)
    assert np.nextafter(v[0], np.float32(0)) == v[1] and float("%.6g" % float(v[0])) == cutoff
    assert rs.kept_mask(e, cnt, 5, cutoff, 4).tolist() == [True, False]
    e, cnt = ri.quantised()
    assert rr.column_values(e, cnt, 3).tolist() == [2.0**-20, float(np.float32(1) / np.float32(3072))]
    e, cnt = ri.out_of_domain()
    assert rr.column_values(e, cnt, 4).tolist() == [0.5, 1.5]
    assert rs.report_edges(e, cnt, 4, 0.0, 4) is None and rs.report_edges(e, cnt, 4, 2.0, 4) is not None
    e, cnt, n = ri.heavy(1000)
    assert (e["source_1"] == 0).all() and rr.column_values(e, cnt, 3).tolist() == [1.0] * 1000 and 3_000_000 << 32 > 1 << 53


@pytest.mark.parametrize("col", [3, 4, 5])
def test_every_value_of_the_short_index_has_at_most_6_digits(col):
    color_off, sources, weights, counts = ri.short_index(col)
    assert len(counts) == 400 and set(counts.tolist()) <= {16, 32, 64} and (col != 4 or set(counts.tolist()) == {64})
    shared = {}
    for c in range(len(weights)):
        members = sources[color_off[c]:color_off[c + 1]].tolist()
        assert len(set(members)) == len(members) >= 2
        for i, x in enumerate(members):
            for y in members[i + 1:]:
                shared[min(x, y), max(x, y)] = shared.get((min(x, y), max(x, y)), 0) + int(weights[c])
    assert len(shared) > 1000 and max(shared.values()) <= 16
    e = np.zeros(len(shared), dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"] = np.array(sorted(shared)).T - 1
    e["shared"] = [shared[k] for k in sorted(shared)]
    v = rr.column_values(e, counts, col)
    assert (v <= 1).all() and len(set(v.tolist())) > 10
    for x in set(v.tolist()):
        assert rr.strtof("%.6g" % x) == x, x                                               # six digits say it all


def test_layouts_and_symbols():
    assert engine.CLUSTER_ROW_DTYPE.itemsize == 48 and engine.MEMBER_ROW_DTYPE.itemsize == 24

    class ClusterRow(ctypes.Structure):
        _fields_ = [("root", ctypes.c_uint32), ("size", ctypes.c_uint32), ("edges", ctypes.c_uint64), ("nan_edges", ctypes.c_uint64), ("sum_q", ctypes.c_uint64),
                    ("min", ctypes.c_float), ("max", ctypes.c_float), ("medoid", ctypes.c_uint32), ("covered", ctypes.c_uint32)]

    class MemberRow(ctypes.Structure):
        _fields_ = [("label", ctypes.c_uint32), ("degree", ctypes.c_uint32), ("strength", ctypes.c_uint64), ("via", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    assert ctypes.sizeof(ClusterRow) == 48 and ctypes.sizeof(MemberRow) == 24             # (the C layout of the header's fields, no padding)
    for dt, st in ((engine.CLUSTER_ROW_DTYPE, ClusterRow), (engine.MEMBER_ROW_DTYPE, MemberRow)):
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"\}\s*ksp_cluster_row;\s*/\* 48 bytes \*/", text) and re.search(r"\}\s*ksp_member_row;\s*/\* 24 bytes \*/", text)
    assert re.search(r"#define KSP_REPORT_CHUNK_EDGES (\d+)u", text).group(1) == str(engine.REPORT_CHUNK_EDGES)
    for name in ("ksp_edges_cluster_report", "ksp_cluster_report_valued", "kspider_cluster_report", "kspider_pairwise_and_cluster_report"):
        assert name in engine.ABI_SYMBOLS and re.search(r"\bint " + name + r"\(", text)
