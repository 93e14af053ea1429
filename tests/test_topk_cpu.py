"""Top-k neighbours without a GPU: the restatement of tests/topk_restate.py on graphs written out by hand with
their expected answers, the refusals the C ABI makes before it touches a device, the constants of the header, and the
properties of every input of tests/topk_inputs.py that tests/test_topk_gpu.py relies on — the entry counts that put a hub into
each class, the ties across the k-th place."""
import os
import re

import numpy as np
import pytest

import derep_inputs as di
import repr_restate as rr
import topk_inputs as ti
import topk_restate as tr
from kspider_amd import engine

NONE = tr.NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUNDRED = np.full(6, 100, dtype=np.uint32)


def _rows(index, count):
    return [index[v, :int(count[v])].tolist() for v in range(len(count))]


# ---- the restatement on graphs with the answers written out ---------------------------------------------------------------------

@pytest.mark.parametrize("col", [3, 4, 5])
def test_star(col):
    e = di.edges([0, 2, 0, 4], [1, 0, 3, 0], [10, 40, 40, 20])         # values 0.1, 0.4, 0.4, 0.2 in every column
    index, count = tr.topk(e, HUNDRED[:5], col, 3)
    assert _rows(index, count) == [[1, 2, 3], [0], [1], [2], [3]]
    assert index[0].tolist() == [1, 2, 3] and index[1].tolist() == [0, NONE, NONE] and count.tolist() == [3, 1, 1, 1, 1]
    index, count = tr.topk(e, HUNDRED[:5], col, 5)
    assert index[0].tolist() == [1, 2, 3, 0, NONE] and count[0] == 4


def test_clique():
    a, b = np.triu_indices(4, 1)                                        # records 0-1, 0-2, 0-3, 1-2, 1-3, 2-3
    e = di.edges(a, b, [5, 50, 20, 30, 10, 40])
    index, count = tr.topk(e, HUNDRED[:4], 5, 2)
    assert _rows(index, count) == [[1, 2], [3, 4], [1, 5], [5, 2]]


def test_a_repeated_pair_in_both_orientations_is_listed_again():
    e = di.edges([0, 1, 0], [1, 0, 1], [10, 30, 30])
    for k, want in ((1, [1]), (2, [1, 2]), (3, [1, 2, 0]), (4, [1, 2, 0])):
        index, count = tr.topk(e, HUNDRED[:2], 4, k)
        assert _rows(index, count) == [want, want], k


def test_self_pairs_and_ends_out_of_range_are_no_entries():
    e = di.edges([2, 2, 0, 1, 9, 1], [2, 2, 1, 7, 1, 0xFFFFFFFF], [90, 90, 10, 99, 99, 99])
    index, count = tr.topk(e, HUNDRED[:3], 5, 2)
    assert _rows(index, count) == [[2], [2], []] and (index[2] == NONE).all()
    assert tr.entries(e, 3).tolist() == [1, 1, 0]


@pytest.mark.parametrize("col", [4, 5])
def test_a_nan_is_below_every_number_and_inf_above(col):
    cnt = np.array([100, 0, 100, 100], dtype=np.uint32)
    e = di.edges([0, 0, 1, 3], [1, 2, 0, 0], [0, 5, 3, 0])              # NaN (0 / 0), 0.05, +inf (3 / 0), 0
    v = rr.column_values(e, cnt, col)
    assert np.isnan(v[0]) and np.isinf(v[2]) and v[3] == 0
    index, count = tr.topk(e, cnt, col, 4)
    assert index[0].tolist() == [2, 1, 3, 0] and index[1].tolist() == [2, 0, NONE, NONE]
    assert tr.topk(e, cnt, col, 1)[0][:, 0].tolist() == [2, 2, 1, 3]


def test_equal_values_are_broken_by_index():
    e = di.edges([3, 0, 0, 2, 0], [0, 1, 2, 0, 4], [7, 7, 9, 7, 7])
    index, count = tr.topk(e, HUNDRED[:5], 3, 3)
    assert index[0].tolist() == [2, 0, 1] and count[0] == 3
    back = e[::-1].copy()                                               # the same records in the other order: the other ones win
    assert tr.topk(back, HUNDRED[:5], 3, 3)[0][0].tolist() == [2, 0, 1]  # (record 2 is the 9 again; then the two lowest indices)
    assert back["source_2"][[0, 1]].tolist() == [4, 0]


def test_ranked_and_the_file():
    index, count = tr.ranked(3, [0, 1, 0], [1, 2, 2], [5, 5, 0xFFFFFFFF], 2)
    assert _rows(index, count) == [[2, 0], [0, 1], [2, 1]]
    text = "h\n1\t2\t9\t0.5\t0.5\t0.5\n3\t1\t9\tnan\tnan\tnan\n2\t3\t9\t 0.50 \t0.5\t0.5\n3\t3\t9\t1\t1\t1\n"
    got = tr.topk_tsv(text, ["a", "b", "c"], 3, 2, "min_cont")
    assert got == b"source\thit\tneighbour\tmin_cont\na\t1\tb\t0.5\na\t2\tc\tnan\nb\t1\ta\t0.5\nb\t2\tc\t0.50\nc\t1\tb\t0.50\nc\t2\ta\tnan\n"
    assert tr.per_source(got)["c"] == [("b", "0.50"), ("a", "nan")]


# ---- the C ABI: constants, and what is refused before a device is touched -------------------------------------------------------

def test_constants_of_the_header():
    text = open(os.path.join(ROOT, "include", "kspider_amd.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (KSP_TOPK_[A-Z_]+) +(\d+)u", text)}
    assert defs == dict(KSP_TOPK_CHUNK_EDGES=engine.TOPK_CHUNK_EDGES, KSP_TOPK_WAVE_ENTRIES=engine.TOPK_WAVE_ENTRIES,
                        KSP_TOPK_LDS_ENTRIES=engine.TOPK_LDS_ENTRIES, KSP_TOPK_MAX_K=engine.TOPK_MAX_K)
    assert (ti.CHUNK, ti.WAVE, ti.LDS, ti.MAX_K) == (engine.TOPK_CHUNK_EDGES, engine.TOPK_WAVE_ENTRIES, engine.TOPK_LDS_ENTRIES, engine.TOPK_MAX_K)
    assert 2 * ti.MAX_K <= ti.LDS and 2 * 8 * ti.LDS <= 160 * 1024


def test_refusals_before_any_device():
    """The checks of the arguments come first, whatever the device: 99 is none anywhere."""
    idx, cnt = np.zeros(8, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    L = engine.lib()
    p, c = idx.ctypes.data, cnt.ctypes.data
    for args, code in (((99, 4, None, 0, None, 5, 0, p, c), engine.KSP_E_ARG),                  # k = 0
                       ((99, 4, None, 0, None, 5, engine.TOPK_MAX_K + 1, p, c), engine.KSP_E_ARG),
                       ((99, 4, None, 0, None, 6, 2, p, c), engine.KSP_E_ARG),                  # no containment column
                       ((99, 4, None, 0, None, 5, 2, p, None), engine.KSP_E_ARG),               # NULL h_count
                       ((99, 4, None, 3, None, 5, 2, p, c), engine.KSP_E_ARG),                  # NULL records with n_edges > 0
                       ((99, 4, p, 0xFFFFFFFF, c, 5, 2, p, c), engine.KSP_E_LIMIT),             # (never read: refused by the count alone)
                       ((99, 4, None, 0, None, 5, 2, p, c), engine.KSP_E_HIP)):
        assert L.ksp_edges_topk(*args) == code, args
    assert L.ksp_last_error().decode().startswith("ksp_edges_topk: no such device")
    assert (idx == 0).all() and (cnt == 0).all()
    with pytest.raises(engine.KspError) as ei:
        engine.topk_ranked(3, [0, 1], [1, 3], [1, 1], 2, device=99)      # an end >= n_nodes
    assert ei.value.code == engine.KSP_E_ARG and "out of range" in str(ei.value)
    for call in (lambda: engine.topk("nowhere/ix", "max_cont", 0), lambda: engine.topk("nowhere/ix", "jaccard", 3),
                 lambda: engine.pairwise_and_topk("nowhere/ix", 1, "ani", 3), lambda: engine.pairwise_and_topk("nowhere/ix", 1, None, engine.TOPK_MAX_K + 1)):
        with pytest.raises(engine.KspError) as ei:
            call()
        assert ei.value.code == engine.KSP_E_ARG
    assert engine.topk_classes().keys() == {"wave", "workgroup", "stream", "refills"}


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------

K_LIMITS = 10        # the k of the class-limit cases


@pytest.mark.parametrize("size", ti.CLASS_LIMIT_HUBS)
def test_class_limit_hubs(size):
    e, cnt, n_nodes, (hub,) = ti.hubs([size])
    n = tr.entries(e, n_nodes)
    assert n[hub] == size and n_nodes - 1 >= ti.SMALL and len(e) == size + 2 * ti.SMALL
    rest = np.delete(n, hub)
    assert rest.max() < ti.WAVE and (rest[:ti.SMALL - 1] > 0).sum() > 250           # everything else is selected by a wave
    want = {ti.WAVE - 1: "wave", ti.WAVE: "wave", ti.WAVE + 1: "workgroup", ti.LDS - 1: "workgroup", ti.LDS: "workgroup", ti.LDS + 1: "stream",
            3 * ti.LDS + 5: "stream"}[size]
    assert ti.class_of(size) == want
    if size == 3 * ti.LDS + 5:
        assert -(-size // (ti.LDS - K_LIMITS)) == 4                                  # refills of LDS - k keys each
    for col in (3, 4, 5):                                                            # a tie across the k-th place of the hub
        index, count = tr.topk(e, cnt, col, K_LIMITS + 1)
        v = rr.column_values(e[index[hub]], cnt, col)
        assert v[K_LIMITS - 1] == v[K_LIMITS] and index[hub, K_LIMITS - 1] < index[hub, K_LIMITS], (size, col)


def test_segments_and_their_ks():
    e, cnt, n_nodes, nodes = ti.hubs(ti.SEGMENTS)
    n = tr.entries(e, n_nodes)
    assert [ti.class_of(int(n[v])) for v in nodes] == ["wave", "workgroup", "stream"] and n[nodes].tolist() == list(ti.SEGMENTS)
    assert ti.ks_around(37) == [1, 36, 37, 38] and ti.ks_around(200) == [1, 199, 200, 201] and ti.ks_around(ti.LDS + 100) == [1, ti.MAX_K]
    assert all(1 <= k <= ti.MAX_K for s in ti.SEGMENTS for k in ti.ks_around(s))


@pytest.mark.parametrize("n,k", ti.TIES)
def test_more_than_k_entries_share_the_best_value(n, k):
    e, cnt, n_nodes, hub, best = ti.ties(n, k)
    assert len(best) == k + 9 and tr.entries(e, n_nodes)[hub] == n
    for col in (3, 4, 5):
        v = rr.column_values(e, cnt, col)
        of_hub = (e["source_1"] == hub) | (e["source_2"] == hub)
        assert len(set(v[best].tolist())) == 1 and (v[of_hub & ~np.isin(np.arange(len(e)), best)] < v[best[0]]).all()
        index, count = tr.topk(e, cnt, col, k)
        assert index[hub].tolist() == best[:k].tolist()                             # the lowest indices win


def test_specials_hold_what_their_test_names():
    e, cnt, meta = ti.specials()
    n = len(cnt)
    inside = (e["source_1"] < n) & (e["source_2"] < n)
    assert (~inside).sum() >= 4 and (e["source_1"][inside] == e["source_2"][inside]).sum() >= 10 and (cnt == 0).sum() == 24
    pairs = set(zip(e["source_1"].tolist(), e["source_2"].tolist()))
    assert sum((b, a) in pairs for a, b in pairs if a < b) >= 100                    # pairs that stand in both orientations
    for col in (3, 4, 5):
        v = rr.column_values(e[inside], cnt, col)
        assert np.isnan(v).sum() >= 10 and np.isinf(v).sum() >= 10 and (v == 0).sum() >= 100, col
    assert (e["shared"] == 0).sum() >= len(e) // 20
    o = ti.orders(e)
    assert (np.diff(o["ascending"]["source_1"].astype(np.int64)) >= 0).all() and (o["reversed"][::-1] == o["ascending"]).all()
    assert sorted(o["random"].tolist()) == sorted(e.tolist()) and (o["random"] != o["ascending"]).any()
    big = tr.entries(e, n)
    assert big.max() > 16                                                            # (segments of more than a few entries)


def test_chunk_sizes_random_records_and_the_ranked_case():
    C = ti.CHUNK
    assert ti.CHUNK_SIZES == (1, 63, 64, 65, C - 1, C, C + 1, 3 * C - 7)
    e, cnt = ti.random_case(3 * C - 7, 40)
    n = tr.entries(e, ti.N_RANDOM)
    assert n.max() <= ti.WAVE and len(set(rr.column_values(e, cnt, 5).tolist())) < len(e) // 2
    n_nodes, a, b, rank, (h1, h2) = ti.ranked_case()
    n = tr.select(n_nodes, a, b, rank, 1)[2]
    assert ti.class_of(int(n[h1])) == "workgroup" and ti.class_of(int(n[h2])) == "stream"
    assert len(set(rank.tolist())) == 12 and rank.min() == 0 and rank.max() == 0xFFFFFFFF
    e, cnt, meta = di.hostile(11, 20000, 2 * C + 1)
    assert meta["n_self"] > 0 and meta["n_outside"] > 0 and len(cnt) == 20000
