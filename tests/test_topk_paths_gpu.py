"""The paths of kspider_amd/csrc/topk.hip that tests/test_topk_gpu.py reaches only by accident, each on a list built for it
(tests/topk_inputs.py; tests/test_topk_cpu.py checks without a GPU that every list has the property named here):

  1. sorted runs     consecutive records that name one node, as the join writes them: runs of 1 .. 2 049 records that fill a
                     ballot, cross it, cross a wave's 512 records and a chunk, in either end and in both at once, with
                     non-entries beside and inside them — the run-combining atomic of the count and scatter passes
  2. node loops      nine adjacent hubs, six of the workgroup class with alternating padded sizes and three streamed ones, on one
                     and on two workgroups: every select workgroup takes several nodes and reuses its LDS buffer
  3. refills         one streamed node whose later refills pass no key, replace the whole head, tie with it, or never fill it
  4. specials        NaN, +inf and 0 in a node of every class, k above the number of numeric entries
  5. inexact counts  exact_values.hostile_edges 1, 8 and 100 times over, and the drop-in call on exact_values.hostile_index
  6. small shapes    2 .. 257 nodes, the last node with the only record

Every case runs in both KSP_TOPK_SELECT modes against tests/topk_restate.py; `index` and `count` are compared for exact equality,
both output arrays have sentinels behind them, d_edges is compared after every call and engine.topk_classes() with the classes
the restatement's entry counts imply (tests/topk_device.py).  There is no tolerance anywhere."""
import glob
import os
import shutil

import numpy as np
import pytest

import exact_values as xv
import repr_restate as rr
import topk_inputs as ti
import topk_restate as tr
from kspider_amd import engine
from topk_device import _check, _check_ranked

pytestmark = pytest.mark.gpu

C = engine.TOPK_CHUNK_EDGES
L = engine.TOPK_LDS_ENTRIES
MAX_K = engine.TOPK_MAX_K
NONE = tr.NONE


# ---- 1. sorted runs --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("workgroups", [None, "2"])
@pytest.mark.parametrize("lead_in", [0, ti.RUN_LEAD_IN])
@pytest.mark.parametrize("layout", ti.RUN_LAYOUTS)
def test_sorted_runs(monkeypatch, layout, lead_in, workgroups):
    """All values of a run are equal, so each hub lists the first k record indices of its run, the non-entries left out: a
    position inside a run that two records share, or one that nobody takes, changes the list."""
    if workgroups:
        monkeypatch.setenv("KSP_TOPK_MAX_WORKGROUPS", workgroups)            # 5 chunks on 2 workgroups: every workgroup loops
    e, cnt, n_nodes, runs = ti.sorted_runs(layout, lead_in)
    for col in (3, 5):
        for k in (1, 10, MAX_K):
            (index, count), _ = _check(monkeypatch, n_nodes, e, cnt, col, k)
            for r in runs:
                own = np.setdiff1d(np.arange(r["start"], r["start"] + r["span"]), r["broken"])[:k]
                for node in (r["hub"],) + ((len(runs) + r["hub"],) if layout == "pair" else ()):
                    assert count[node] == len(own) and index[node, :len(own)].tolist() == own.tolist(), (layout, r["hub"], k)


# ---- 2. several nodes per looping workgroup --------------------------------------------------------------------------------------

@pytest.mark.parametrize("workgroups", ["1", "2"])
def test_several_nodes_per_select_workgroup(monkeypatch, workgroups):
    """k = 70 lies above the segments of 65 and 66 entries and below the others; KSP_TOPK_MAX_K above the one of 1 000 as well."""
    monkeypatch.setenv("KSP_TOPK_MAX_WORKGROUPS", workgroups)
    e, cnt, n_nodes, nodes = ti.adjacent_hubs()
    for k in (1, 70, MAX_K):
        (index, count), classes = _check(monkeypatch, n_nodes, e, cnt, 5, k)
        assert count[nodes].tolist() == [min(k, n) for n in ti.ADJACENT_HUBS]
        assert classes["workgroup"] == 6 and classes["stream"] == 3 and classes["wave"] > 250
        assert classes["refills"] == sum(-(-n // (L - k)) for n in ti.ADJACENT_HUBS[6:])


# ---- 3. refills that pass nothing, and refills that replace everything -----------------------------------------------------------

@pytest.mark.parametrize("k", ti.REFILL_KS)
@pytest.mark.parametrize("layout", ti.REFILL_LAYOUTS)
def test_refills(monkeypatch, layout, k):
    """One node of four refills through ksp_topk_ranked.  "head_first" is what it says only because of the single workgroup: the
    scatter then walks the chunks in order, the node's entries of chunk 0 take the first 2 048 slots of its segment, and these
    lie inside the first refill (KSP_TOPK_LDS_ENTRIES - k >= 3 072); every later refill then passes no key.  The trace counts
    refills, not sorts: this test proves the result, not the path taken."""
    monkeypatch.setenv("KSP_TOPK_MAX_WORKGROUPS", "1")
    n_nodes, a, b, rank, hub = ti.refill_case(layout, k)
    (index, count), classes = _check_ranked(monkeypatch, n_nodes, a, b, rank, k)
    assert count[hub] == k and classes == dict(wave=n_nodes - 1, workgroup=0, stream=1, refills=4)


# ---- 4. NaN, +inf and zero in every class ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("col", [3, 4, 5])
def test_nan_inf_and_zero_in_every_class(monkeypatch, col):
    e, cnt, n_nodes, nodes = ti.special_hubs()
    v = rr.column_values(e, cnt, col)
    for k in ti.SPECIAL_KS:
        (index, count), classes = _check(monkeypatch, n_nodes, e, cnt, col, k)
        assert classes["workgroup"] == 2 and classes["stream"] == 2 and classes["refills"] == 2 * -(-ti.SPECIAL_HUBS[2] // (L - k))
        for h, k_of in zip(nodes, ti.SPECIAL_KS + ti.SPECIAL_KS):
            if k_of == k:                                                    # the k that reaches this hub's NaN entries
                listed = v[index[h, :count[h]]]
                nan = np.isnan(listed)
                assert nan.any() and not nan[0] and (np.diff(nan.astype(int)) >= 0).all(), (col, h, k)
                assert (np.diff(index[h, :count[h]][nan].astype(np.int64)) > 0).all()       # the NaN entries in index order


# ---- 5. inexact counts -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("col", [3, 4, 5])
@pytest.mark.parametrize("copies", ti.TILED_COPIES)
def test_inexact_counts(monkeypatch, copies, col):
    e, cnt, n_nodes = ti.tiled(copies)
    for k in ti.TILED_KS[copies]:
        _, classes = _check(monkeypatch, n_nodes, e, cnt, col, k)
        assert (classes["wave"], classes["workgroup"], classes["stream"]) == ti.TILED_CLASSES[copies]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_drop_in_call_on_the_hostile_index(oracle_lib, tmp_path, monkeypatch, devices):
    """engine.pairwise_and_topk where every count and every shared count is an inexact float above 2^24."""
    if devices:
        monkeypatch.setenv("KSPIDER_DEVICES", devices)
    ix = xv.hostile_index(1)
    (tmp_path / "index").mkdir()
    prefix = str(tmp_path / "index" / "ix")
    oracle_lib.write_index(prefix, ix["color_off"], ix["sources"], ix["color_w"], ix["group_ids"], ix["kmer_counts"])
    names = [f"genome_{i + 1}" for i in range(ix["n_names"])]
    with open(prefix + ".namesMap", "w") as f:
        f.write(f"{len(names)}\n" + "".join(f"{i + 1} {name}\n" for i, name in enumerate(names)))
    shutil.copytree(tmp_path / "index", tmp_path / "full")
    full = str(tmp_path / "full" / "ix")
    oracle_lib.ref_pairwise(full, 1)
    tsv, seq = _read(full + "_kSpider_pairwise.tsv"), _read(full + "_kSpider_seqToKmersNo.tsv")
    counts = np.zeros(ix["n_names"], dtype=np.uint32)
    counts[ix["group_ids"] - 1] = ix["kmer_counts"]
    for dist, col in (("min_cont", 3), ("avg_cont", 4), ("max_cont", 5)):
        for k in (3, 39):                                                    # 39: every row of every source
            engine.pairwise_and_topk(prefix, 2, dist, k)
            assert _read(prefix + "_kSpider_pairwise.tsv") == tsv and _read(prefix + "_kSpider_seqToKmersNo.tsv") == seq
            out = prefix + f"_kSpider_topk_{dist}.tsv"
            want = tr.topk_tsv_floats(tsv.decode(), names, counts, col, k, dist)
            assert _read(out) == want and want.count(b"\n") > k * ix["n_names"] // 2, (dist, k, devices)
            os.remove(out)
    assert not glob.glob(str(tmp_path / "index" / "*.partial"))


# ---- 6. small shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("n_nodes", ti.SMALL_NODES)
def test_small_shapes(monkeypatch, n_nodes, single):
    e, cnt = ti.small_case(n_nodes, single)
    for k in (1, 4):
        (index, count), classes = _check(monkeypatch, n_nodes, e, cnt, 5, k)
        assert count[n_nodes - 1] >= 1 and classes["wave"] == int((count > 0).sum()) >= 2
        if single:
            assert count.sum() == 2 and index[0, 0] == index[n_nodes - 1, 0] == 0
