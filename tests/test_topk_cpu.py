"""Top-k neighbours without a GPU: the restatement of tests/topk_restate.py on graphs written out by hand with
their expected answers, the refusals the C ABI makes before it touches a device, the constants of the header, and the
properties of every input of tests/topk_inputs.py that tests/test_topk_gpu.py and tests/test_topk_paths_gpu.py rely on — the entry
counts that put a hub into each class, the ties across the k-th place, the runs, refill layouts, special values and inexact
counts of the second file."""
import os
import re

import numpy as np
import pytest

import derep_inputs as di
import exact_values as xv
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


# ---- the inputs of tests/test_topk_paths_gpu.py ---------------------------------------------------------------------------------

@pytest.mark.parametrize("lead_in", [0, ti.RUN_LEAD_IN])
@pytest.mark.parametrize("layout", ti.RUN_LAYOUTS)
def test_sorted_runs(layout, lead_in):
    """The run lengths, what the runs do at 64 records (a ballot), 512 (a wave's range of a chunk) and CHUNK, and the classes."""
    e, cnt, n_nodes, runs = ti.sorted_runs(layout, lead_in)
    assert tuple(r["span"] for r in runs) == ti.RUN_LENGTHS == (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049)
    assert runs[0]["start"] == lead_in and len(e) == lead_in + sum(ti.RUN_LENGTHS) + ti.RUN_GAP * len(ti.RUN_GAPS)
    for r, nxt in zip(runs, runs[1:]):                                       # a run starts where the last ended, or behind a gap of non-entries
        assert nxt["start"] == r["start"] + r["span"] + (ti.RUN_GAP if r["hub"] in ti.RUN_GAPS else 0)
    n = tr.entries(e, n_nodes)
    assert [int(n[r["hub"]]) for r in runs] == [r["entries"] for r in runs]
    assert sum(len(r["broken"]) == 2 for r in runs) == 3 and sum(len(r["broken"]) for r in runs) == 6
    assert [ti.class_of(r["entries"]) for r in runs] == ["wave"] * 4 + ["workgroup"] * 10
    s1, s2 = e["source_1"].astype(np.int64), e["source_2"].astype(np.int64)
    lanes = {(("self" if s1[p] == s2[p] else "outside"), int(p) % 64) for r in runs for p in r["broken"]}
    assert all(s1[p] == s2[p] or max(s1[p], s2[p]) >= n_nodes for r in runs for p in r["broken"])
    assert ("self", 0) in lanes and ("outside", 63) in lanes
    gaps = (s1 == s2) | (np.maximum(s1, s2) >= n_nodes)
    assert gaps.sum() == ti.RUN_GAP * len(ti.RUN_GAPS) + 6 and (s1[gaps] == s2[gaps]).sum() == 2 * ti.RUN_GAP + 3
    ends = {"source_1": ("source_1",), "source_2": ("source_2",), "pair": ("source_1", "source_2")}[layout]
    for end in ("source_1", "source_2"):
        node, start, stop = ti.sub_runs(e, n_nodes, end)
        length = stop - start
        if end not in ends:
            assert length.max() == 1                                        # the other end changes with every record
            continue
        of_runs = length[start >= lead_in].tolist()
        assert max(of_runs) == 2049 and all(r["span"] in of_runs for r in runs if not r["broken"])
        for B in (64, ti.WAVE_RANGE, ti.CHUNK):
            inside = ((stop - 1) // B > start // B) & (start % B != 0) & (stop % B != 0)
            assert inside.any(), (end, B, "no run crosses it")
            assert ((stop % B == 0) & (length >= 2)).any() and ((start % B == 0) & (length >= 2) & (start > 0)).any(), (end, B, "no run meets it")
        assert (length[(start % 64 == 0)] >= 64).any()                       # a ballot of one run, first lane to last
    # all values of a run are equal: its order is the index alone
    for col in (3, 5):
        v = rr.column_values(e[~gaps], cnt, col)
        at = np.nonzero(~gaps)[0]
        for r in runs:
            own = v[(at >= r["start"]) & (at < r["start"] + r["span"])]
            assert len(own) == r["entries"] and len(set(own.tolist())) == 1


def test_adjacent_hubs():
    e, cnt, n_nodes, nodes = ti.adjacent_hubs()
    L = ti.LDS
    assert nodes == list(range(9)) and ti.ADJACENT_HUBS == (4096, 65, 1000, 129, 2048, 66, 2 * L + 7, L + 1, L + 300)
    n = tr.entries(e, n_nodes)
    assert n[nodes].tolist() == list(ti.ADJACENT_HUBS)
    assert [ti.class_of(int(x)) for x in n[nodes]] == ["workgroup"] * 6 + ["stream"] * 3
    padded = [1 << int(x - 1).bit_length() for x in ti.ADJACENT_HUBS[:6]]
    assert padded == [4096, 128, 1024, 256, 2048, 128]
    assert all(a != b for a, b in zip(padded, padded[1:])) and all(a != b for a, b in zip(padded[0::2], padded[2::2])) \
        and all(a != b for a, b in zip(padded[1::2], padded[3::2]))          # on one workgroup and on two (nodes 0, 2, 4 and 1, 3, 5)
    assert n[6] > n[7] < n[8]                                                # a streamed node behind a longer one
    assert n[9:].max() <= ti.WAVE and 250 < int((n[9:ti.SMALL] > 0).sum())
    for k in (1, 70, ti.MAX_K):
        assert [-(-int(x) // (L - k)) for x in n[6:9]] == {1: [3, 2, 2], 70: [3, 2, 2], ti.MAX_K: [3, 2, 2]}[k]
    assert 66 < 70 < 129 and 1000 < ti.MAX_K < 2048
    # the old default: the same arrays as before the parameter
    old, new = ti.hubs([70, 200]), ti.hubs([70, 200], hub_nodes=ti.HUB_NODES[:2])
    assert (old[0] == new[0]).all() and (old[1] == new[1]).all() and old[2:] == new[2:]


@pytest.mark.parametrize("k", ti.REFILL_KS)
@pytest.mark.parametrize("layout", ti.REFILL_LAYOUTS)
def test_refill_cases(layout, k):
    L, C = ti.LDS, ti.CHUNK
    n_nodes, a, b, rank, hub = ti.refill_case(layout, k)
    n = len(a)
    assert n == L + 2 * (L - k) + 1 and ((a == hub) ^ (b == hub)).all() and -(-n // (L - k)) == 4 and L - k >= 3072 > C
    entries = tr.select(n_nodes, a, b, rank, 1)[2]
    assert entries[hub] == n and 0 < entries[1:].min() and entries[1:].max() <= ti.WAVE
    index, count = tr.ranked(n_nodes, a, b, rank, k)
    best = index[hub].astype(np.int64)
    r = rank.astype(np.int64)
    if layout == "head_first":
        assert best.max() < C and (r[C:] < r[best].min()).all()              # every later record is worse than every one of the best k
    elif layout == "rising":
        assert best.tolist() == list(range(n - 1, n - 1 - k, -1))            # the last k: every refill brings better keys only
        assert (np.diff(r) > 0).all()
    elif layout == "equal":
        assert best.tolist() == list(range(k)) and len(set(r.tolist())) == 1
    else:
        assert (r > 0).sum() == k - 1 and (r[best[:k - 1]] > 0).all() and best[k - 1] == np.nonzero(r == 0)[0][0]
        assert k == 1 or np.nonzero(r > 0)[0].max() > n - (L - k)              # a real key arrives with the last refill as well


def test_special_hubs():
    """Per hub and column: +inf first where the hub has one, then numbers, then — within the first k — NaN entries in index order."""
    e, cnt, n_nodes, nodes = ti.special_hubs()
    n = tr.entries(e, n_nodes)
    assert n[nodes].tolist() == list(ti.SPECIAL_HUBS) * 2 == [40, 500, ti.LDS + 500] * 2
    assert [ti.class_of(int(x)) for x in n[nodes]] == ["wave", "workgroup", "stream"] * 2 and n[len(nodes):].max() == 1
    assert cnt[nodes].tolist() == [0, 0, 0, 3500, 3500, 3500]
    seen_inf = 0
    for col in (3, 4, 5):
        v = rr.column_values(e, cnt, col)
        for h, k in zip(nodes, ti.SPECIAL_KS * 2):
            of_hub = (e["source_1"] == h) | (e["source_2"] == h)
            numbers = int((~np.isnan(v[of_hub])).sum())
            assert numbers < k <= ti.MAX_K and n[h] > k                      # k reaches the NaN entries and not the end of the list
            if col == 4:
                assert np.isnan(v[of_hub]).sum() >= (2 * int(n[h])) // 3     # two thirds and more
            index, count = tr.topk(e, cnt, col, k, n_nodes)
            listed = v[index[h]]
            if np.isinf(v[of_hub]).any():
                seen_inf += 1
                n_inf = int(np.isinf(v[of_hub]).sum())
                assert np.isinf(listed[:n_inf]).all() and np.isfinite(listed[n_inf:numbers]).all()
            assert not np.isnan(listed[:numbers]).any() and np.isnan(listed[numbers:]).all() and k - numbers >= 1
            assert (np.diff(index[h, numbers:].astype(np.int64)) > 0).all()
            assert (v[of_hub] == 0).any() or (col == 4 and cnt[h] == 0)
    assert seen_inf == 15                                                    # every hub and column but column 3 of the hubs that count k-mers


def _classes(n):
    return tuple(sum(ti.class_of(int(x)) == c for x in n) for c in ("wave", "workgroup", "stream"))


def test_tiled_classes_and_ties():
    h = xv.hostile_edges(1)
    assert len(h.kmer_counts) == 599 and len(h.edges) == 6161
    for copies in ti.TILED_COPIES:
        e, cnt, n_nodes = ti.tiled(copies)
        n = tr.entries(e, n_nodes)
        assert len(e) == 6161 * copies and _classes(n) == ti.TILED_CLASSES[copies], copies
        if copies == 1:
            assert n.max() == 49 == ti.TILED_KS[1][0]
    assert ti.TILED_CLASSES == {1: (599, 0, 0), 8: (169, 430, 0), 100: (0, 592, 7)}
    # ties between entries of one node whose `shared` differ and whose column float is equal: nothing but the index decides them
    e = h.edges
    for col in (3, 4, 5):
        bits = xv.bits_of(rr.column_values(e, h.kmer_counts, col))
        groups = {}
        for end in ("source_1", "source_2"):
            for node, b, s in zip(e[end].tolist(), bits.tolist(), e["shared"].tolist()):
                groups.setdefault((node, b), set()).add(s)
        assert sum(len(s) > 1 for (_, b), s in groups.items() if b != xv.NAN) >= 32, col


@pytest.mark.parametrize("col", [3, 4, 5])
def test_a_wrong_column_changes_the_inexact_top_k(col):
    """How many nodes' restated lists change under each deliberately wrong column of exact_values.WRONG, at the k values of
    tests/test_topk_paths_gpu.py: one copy at k = 49 (every entry of every node: the full ranking), a hundred copies at k = 10 and
    KSP_TOPK_MAX_K (the latter from one selection: the first 10 of 1 024).  Measured (columns 3 / 4 / 5):

        variant                  1 copy, k = 49    100 copies, k = 1 024    100 copies, k = 10
        shared_32_bits           279 / 280 / 280   279 / 280 / 280          275 / 268 / 268
        toward_zero              19 / 15 / 19      23 / 17 / 11             11 / 3 / 3
        reciprocal               11 / 14 / 13      14 / 12 / 10             2 / 4 / 2
        double_division          17 / 13 / 14      18 / 9 / 9               6 / 2 / 3
        shared_through_double    1 / 1 / 1         1 / 1 / 1                1 / 0 / 0
        fmin_fmax                2 / - / 2         2 / - / 2                0 / - / 0
        double_average           - / 0 / -         - / 0 / -                - / 0 / -

    fmin_fmax is the right computation in column 4 and double_average in columns 3 and 5 (-).  double_average is the right
    computation in column 4 as well: it gives the same float bit for bit for every value a record can have
    (tests/test_exact_values_cpu.py::test_the_double_average_is_the_same_function), so there is nothing for an order to tell apart,
    at k = 10 or at the full ranking.  Every other variant has a floor of 1 at the full ranking and at KSP_TOPK_MAX_K over a
    hundred copies; at k = 10 the floor holds for the four variants that change more than one node."""
    for copies, k in ((1, 49), (100, ti.MAX_K)):
        e, cnt, n_nodes = ti.tiled(copies)
        select = lambda values: tr.select(n_nodes, e["source_1"], e["source_2"], values, k)[0]
        right = select(rr.column_values(e, cnt, col))
        for name, wrong in xv.WRONG.items():
            same_by_definition = (name == "fmin_fmax" and col == 4) or (name == "double_average" and col != 4)
            if copies == 100 and (same_by_definition or name == "double_average"):
                continue
            got = select(wrong(e, cnt, col))
            changed = int((got != right).any(axis=1).sum())
            changed_10 = int((got[:, :10] != right[:, :10]).any(axis=1).sum())
            if same_by_definition or name == "double_average":
                assert changed == 0, (name, copies)
                continue
            assert changed >= 1, (name, copies, col)
            if copies == 100 and name in ("shared_32_bits", "toward_zero", "reciprocal", "double_division"):
                assert changed_10 >= 1, (name, col)
    if col == 4:
        h = xv.hostile_edges(1)
        a, b = rr.column_values(h.edges, h.kmer_counts, 4), xv.WRONG["double_average"](h.edges, h.kmer_counts, 4)
        assert (xv.bits_of(a) == xv.bits_of(b)).all()                        # the same column: nothing to tell apart


def test_small_cases():
    assert ti.SMALL_NODES == (2, 63, 64, 65, 257)
    for n_nodes in ti.SMALL_NODES:
        e, cnt = ti.small_case(n_nodes, True)
        assert len(e) == 1 and len(cnt) == n_nodes and tr.entries(e, n_nodes).tolist() == [1] + [0] * (n_nodes - 2) + [1]
        e, cnt = ti.small_case(n_nodes, False)
        n = tr.entries(e, n_nodes)
        assert len(e) == 9 and n[n_nodes - 1] >= 1 and n.sum() >= 2 and n.max() <= ti.WAVE
