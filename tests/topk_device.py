"""What tests/test_topk_gpu.py and tests/test_topk_paths_gpu.py share: one call of ksp_edges_topk or ksp_topk_ranked with sentinels
behind both output arrays and d_edges compared afterwards, the exact comparison with a restated result, the classes that the
restatement's entry counts imply, and both KSP_TOPK_SELECT modes against tests/topk_restate.py."""
import numpy as np

import topk_restate as tr
from kspider_amd import engine

W = engine.TOPK_WAVE_ENTRIES
L = engine.TOPK_LDS_ENTRIES
NONE = tr.NONE
TAIL = 7                        # sentinel entries behind both output arrays
FILL = 0xDEADBEEF
MODES = ("kernels", "library")
NO_CLASSES = dict(wave=0, workgroup=0, stream=0, refills=0)


def _device(n_nodes, e, cnt, col, k):
    """ksp_edges_topk over e; returns ((index, count), what the select kernels did)."""
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    ed = engine.DeviceBuffer.from_numpy(e) if len(e) else None
    cd = engine.DeviceBuffer.from_numpy(cnt)
    try:
        got = engine.edges_topk(n_nodes, ed.ptr.value if ed else 0, len(e), cd.ptr.value, col, k, tail=TAIL, fill=FILL)
        if len(e):
            assert (ed.to_numpy(engine.EDGE_DTYPE, len(e)) == e).all(), "d_edges was written"
        return got, engine.topk_classes()
    finally:
        for buf in (ed, cd):
            if buf:
                buf.free()


def _same(got, want, what):
    index, count = got
    assert (count == want[1]).all(), (what, "count", int((count != want[1]).sum()))
    assert (index == want[0]).all(), (what, "index", int((index != want[0]).any(axis=1).sum()))
    behind = np.arange(index.shape[1])[None, :] >= count[:, None]
    assert (index[behind] == NONE).all() and (index[~behind] != NONE).all(), what


def _expected_classes(n_entries, k):
    n = np.asarray(n_entries)
    stream = n[n > L]
    return dict(wave=int(((n > 0) & (n <= W)).sum()), workgroup=int(((n > W) & (n <= L)).sum()), stream=len(stream),
                refills=int((-(-stream // (L - k))).sum()))


def _check(monkeypatch, n_nodes, e, cnt, col, k, want=None):
    """Both modes against the restatement; returns (the restatement's result, the classes of the kernels mode)."""
    want = tr.topk(e, cnt, col, k, n_nodes) if want is None else want
    seen = {}
    for mode in MODES:
        monkeypatch.setenv("KSP_TOPK_SELECT", mode)
        got, seen[mode] = _device(n_nodes, e, cnt, col, k)
        _same(got, want, (mode, n_nodes, len(e), col, k))
    assert seen["library"] == NO_CLASSES
    assert seen["kernels"] == _expected_classes(tr.entries(e, n_nodes), k), (seen["kernels"], k)
    return want, seen["kernels"]


def _check_ranked(monkeypatch, n_nodes, a, b, rank, k):
    """ksp_topk_ranked in both modes against the restatement; returns (the restatement's result, the classes of the kernels mode)."""
    want = tr.ranked(n_nodes, a, b, rank, k)
    seen = {}
    for mode in MODES:
        monkeypatch.setenv("KSP_TOPK_SELECT", mode)
        _same(engine.topk_ranked(n_nodes, a, b, rank, k, tail=TAIL, fill=FILL), want, (mode, n_nodes, len(a), k))
        seen[mode] = engine.topk_classes()
    assert seen["library"] == NO_CLASSES
    assert seen["kernels"] == _expected_classes(tr.select(n_nodes, a, b, rank, 1)[2], k), (seen["kernels"], k)
    return want, seen["kernels"]
