"""The cut-off ladder without a GPU: the restatement (tests/sweep_restate.py) against the cluster files the
REFERENCE wrote for the golden sets, the nesting the device relies on — "kept at c" is "level above the rank of c" — and the
refusals that are decided before any device call."""
import os
import re

import numpy as np
import pytest

import cut_restate as cr
import sweep_restate as sr
from kspider_amd import engine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "clusters")
LADDERS = {"max_cont": (5, [0.0, 0.3, 1.0]), "min_cont": (3, [0.07, 0.5])}


def _as_sets(path):
    return sorted(tuple(sorted(l.rstrip("\n").split(","))) for l in open(path) if l.strip())


def _golden(tag):
    """(names by node, rows of the pairwise TSV as lists of text) of a golden set."""
    prefix = os.path.join(GOLD, tag, "sigs")
    names = {}
    with open(prefix + ".namesMap") as f:
        next(f)
        for row in f:
            i, name = row.split()[:2]
            names[int(i) - 1] = name
    rows = [l.rstrip("\n").split("\t") for l in list(open(prefix + "_kSpider_pairwise.tsv"))[1:] if l.strip()]
    return [names[v] for v in range(len(names))], rows


@pytest.mark.parametrize("tag", ["setA", "setB"])
def test_restatement_equals_the_reference_clusters(tag):
    names, rows = _golden(tag)
    a = np.array([int(r[0]) - 1 for r in rows])
    b = np.array([int(r[1]) - 1 for r in rows])
    for dist, (col, cutoffs) in LADDERS.items():
        texts = [r[col] for r in rows]
        mk = sr.masks(texts, cutoffs)
        for c, m in zip(cutoffs, mk):
            lab = sr.union_find(len(names), a[m], b[m])
            comps = {}
            for v, r in enumerate(lab.tolist()):
                comps.setdefault(r, []).append(names[v])
            got = sorted(tuple(sorted(c_)) for c_ in comps.values())
            assert got == _as_sets(os.path.join(GOLD, tag, f"ref_{dist}_{c}.clusters")), (tag, dist, c)


def test_kept_at_a_cutoff_is_level_above_its_rank():
    rng = np.random.default_rng(11)
    vals = np.concatenate([rng.random(400).astype(np.float32), np.float32([0.0, 1.0, 0.07, 0.3, 0.5, np.nan, 0.0699999, 0.299999])])
    texts = [engine.format_float(float(v)) for v in vals]
    for trial in range(6):
        base = rng.choice([0.0, 0.07, 0.1, 0.3, 0.30000001, 0.5, 0.9, 1.0, 2.0, -0.5], size=6, replace=False).tolist()
        cutoffs = base + [base[1], base[4]]                     # duplicates
        rng.shuffle(cutoffs)
        mk, lv = sr.masks(texts, cutoffs), sr.levels(texts, cutoffs)
        rank = sr.strictness_ranks(texts, cutoffs)
        assert sorted(rank.tolist()) == list(range(len(cutoffs)))
        for i in range(len(cutoffs)):
            assert (mk[i] == (lv > rank[i])).all(), (cutoffs, i)
        assert lv[texts.index("nan")] == len(cutoffs)           # a NaN passes every cut-off


def test_restatement_helpers_agree_with_the_cut_restatement():
    e = np.zeros(4, dtype=engine.EDGE_DTYPE)
    e["source_1"], e["source_2"], e["shared"] = [0, 0, 2, 1], [1, 2, 3, 2], [8, 7, 0, 3]
    cnt = np.array([10, 10, 10, 0])
    for col in (3, 4, 5):
        texts = sr.column_texts(e, cnt, col)
        for c in (0.0, 0.3, 0.75, 0.8, 1.0):
            assert (sr.masks(texts, [c])[0] == cr.edge_mask(e, cnt, col, c)).all()
            lab, kept = sr.ladder(4, e, texts, [c])
            assert (lab[0] == sr.components(4, e, cnt, col, c)).all() and kept[0] == cr.edge_mask(e, cnt, col, c).sum()
    lab = sr.per_rank_components(4, [0, 1, 2], [1, 2, 3], [1, 2, 0], 2)
    assert lab.tolist() == [[0, 0, 0, 3], [0, 1, 1, 3]]


def test_constants_are_mirrored_and_exported():
    text = open(os.path.join(ROOT, "include", "kspider_amd.h")).read()
    assert int(re.search(r"#define KSP_SWEEP_CHUNK_EDGES (\d+)u", text).group(1)) == engine.SWEEP_CHUNK_EDGES
    assert int(re.search(r"#define KSP_SWEEP_MAX_CUTOFFS (\d+)u", text).group(1)) == engine.SWEEP_MAX_CUTOFFS == 255
    import kspider_amd
    assert kspider_amd.cluster_sweep is engine.cluster_sweep and kspider_amd.pairwise_and_cluster_sweep is engine.pairwise_and_cluster_sweep


def test_argument_checks_need_no_device(tmp_path):
    """Refusals that are decided before any device call; a refused call writes no file."""
    prefix = str(tmp_path / "nope")
    too_many = [i / 256 for i in range(256)]
    for cutoffs in ([], None, too_many, [0.5, float("nan")]):
        for call in (lambda c: engine.cluster_sweep(prefix, "max_cont", c), lambda c: engine.pairwise_and_cluster_sweep(prefix, 1, "max_cont", c),
                     lambda c: engine.components_edges_sweep(0, 0, 0, 0, 5, c)):
            with pytest.raises(engine.KspError) as ei:
                call(cutoffs)
            assert ei.value.code == engine.KSP_E_ARG, cutoffs
    with pytest.raises(engine.KspError) as ei:
        engine.cluster_sweep(prefix, "jaccard", [0.5])
    assert ei.value.code == engine.KSP_E_ARG
    for dist in ("jaccard", "ani"):
        with pytest.raises(engine.KspError) as ei:
            engine.pairwise_and_cluster_sweep(prefix, 1, dist, [0.5])
        assert ei.value.code == engine.KSP_E_ARG and dist in str(ei.value)
    for kw in (dict(dist_col=2), dict(dist_col=6)):
        with pytest.raises(engine.KspError) as ei:
            engine.components_edges_sweep(0, 0, 0, 0, cutoffs=[0.5], **kw)
        assert ei.value.code == engine.KSP_E_ARG, kw
    with pytest.raises(engine.KspError) as ei:
        engine.components_edges_sweep(4, 0, 5, 0, 5, [0.5])            # NULL pointers with edges
    assert ei.value.code == engine.KSP_E_ARG
    z = np.zeros(1, dtype=np.uint32)
    for n_levels in (0, 256):
        with pytest.raises(engine.KspError) as ei:
            engine.components_sweep(4, z, z, np.zeros(1, dtype=np.uint8), n_levels)
        assert ei.value.code == engine.KSP_E_ARG, n_levels
    with pytest.raises(engine.KspError) as ei:
        engine.components_sweep(4, z, z, np.array([3], dtype=np.uint8), 2)         # a level above n_levels
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.components_sweep(4, z, np.array([4], dtype=np.uint32), np.array([1], dtype=np.uint8), 2)   # a node out of range
    assert ei.value.code == engine.KSP_E_ARG
    L = engine.lib()
    assert L.ksp_components_sweep(0, 4, None, None, None, 3, 2, z.ctypes.data) == engine.KSP_E_ARG      # NULL arrays with edges
    assert L.ksp_components_sweep(0, 4, None, None, None, 0, 2, None) == engine.KSP_E_ARG               # NULL labels with nodes
    assert L.ksp_components_edges_sweep(0, 4, None, 0, None, 5, np.zeros(1).ctypes.data, 1, None, None) == engine.KSP_E_ARG
    assert L.kspider_cluster_sweep(None, b"max_cont", np.zeros(1).ctypes.data, 1) == engine.KSP_E_ARG
    assert L.kspider_pairwise_and_cluster_sweep(None, 1, b"max_cont", np.zeros(1).ctypes.data, 1) == engine.KSP_E_ARG
    assert not list(tmp_path.iterdir())
