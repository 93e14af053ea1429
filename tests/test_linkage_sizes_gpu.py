"""The device single linkage of `kSpider export --newick` at the sizes where its behaviour changes:
k_prim_single keeps D[] in LDS up to 19 456 nodes and in global memory above, and the entry points stop at 65 536
nodes, where n^2 = 2^32 elements no longer fit a 32-bit count.  Every comparison is bit for bit: the distance matrix
against the exact sequential sums (oracle.row_pdist, pinned to export_restate.row_pdist by test_export_cpu.py), Prim's
rows against a host replay, the linkage matrix against their relabel."""
import math
import time

import numpy as np
import pytest

import export_restate as er
from kspider_amd import engine

pytestmark = pytest.mark.gpu

LDS_NODES = 19456      # kPrimLdsNodes in export.hip
MAX_NODES = 65536      # kMaxNodes
# duplicated rows (with their columns): whenever Prim first reaches either row of a pair, both tie at the minimum and
# the smaller index must win.  1 / 1025: one Prim lane holds both (i % 1024); 3 / 67: the same lane number in two
# waves; 19 456: the last node, only at 19 457 nodes (D[] in global memory); 19 453 / 19 454: the last, partly filled
# 64-row tile of k_row_dist at every size here.
DUP_PAIRS = [(1, 1025), (3, 67), (10, 19456), (19453, 19454)]


def _u64(a):
    return a.view(np.uint64)


def _on_device(fns, M, n):
    """[f(device pointer, n) for f in fns] on the leading n x n block of M."""
    buf = engine.DeviceBuffer.from_numpy(np.ascontiguousarray(M[:n, :n]))
    try:
        return [f(buf.ptr.value, n) for f in fns]
    finally:
        buf.free()


def _sparse_six_digit(rng, n, per_row):
    """A symmetric n x n matrix with about per_row nonzero cells per row, each made as the export makes it:
    read_csv(repr(1 - float('%.6g' % c))), and a zero diagonal; the rows of DUP_PAIRS duplicated."""
    m = n * per_row // 2
    i = rng.integers(0, n, size=m)
    j = rng.integers(0, n, size=m)
    keep = i != j
    i, j = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    texts = ["%.6g" % c for c in rng.random(len(i))]
    cells = {t: er.xstrtod(repr(1 - float(t))) for t in set(texts)}
    M = np.zeros((n, n))
    M[i, j] = [cells[t] for t in texts]     # (a pair drawn twice keeps one of its cells)
    M[j, i] = M[i, j]
    for a, b in DUP_PAIRS:
        M[b] = M[a]
        M[:, b] = M[:, a]
    return M


@pytest.fixture(scope="module")
def matrix_19457():
    M = _sparse_six_digit(np.random.default_rng(19457), LDS_NODES + 1, 24)
    assert (M == M.T).all() and not M.diagonal().any()
    for a, b in DUP_PAIRS:
        assert (M[a] == M[b]).all()
    assert 16 <= np.count_nonzero(M, axis=1).mean() <= 40
    return M


@pytest.mark.parametrize("n", [LDS_NODES - 1, LDS_NODES, LDS_NODES + 1])
def test_linkage_at_the_lds_switch(matrix_19457, n, oracle_lib, monkeypatch):
    """n = 19 455 and 19 456 keep D[] in LDS, 19 457 puts it in global memory; 19 456 also runs with KSP_PRIM_LDS=0.
    On the leading n x n block of one matrix: the distance matrix equals the exact sequential sums in all n^2 entries,
    Prim's rows (with the nearest merged node) equal the replay on that matrix, the linkage equals their relabel."""
    M = matrix_19457
    t0 = time.perf_counter()
    S, P, Z = _on_device((engine.row_distances, engine.single_linkage_prim, engine.single_linkage_rows), M, n)
    t1 = time.perf_counter()
    ref = oracle_lib.row_pdist(M[:n, :n])
    t2 = time.perf_counter()
    assert S.shape == (n, n)
    bad = np.flatnonzero(_u64(S) != _u64(ref))
    assert not len(bad), f"{len(bad)} distances differ, the first at {divmod(int(bad[0]), n)}"
    del S
    first = {int(y): k for k, y in enumerate(P[:, 1])}   # on the device's own walk: each pair's tie to the smaller index
    lost = [(a, b) for a, b in DUP_PAIRS if b < n and not first[a] < first[b]]
    assert not lost, f"ties taken by the larger index: {lost}"
    assert (_u64(ref) == _u64(ref.T)).all() and (_u64(ref.diagonal()) == 0).all()   # symmetric, diagonal +0
    prim = er.prim_rows(ref, nearest=True)
    del ref
    t3 = time.perf_counter()
    step = {int(y): k for k, y in enumerate(prim[:, 1])}
    assert all(step[a] < step[b] for a, b in DUP_PAIRS if b < n)   # (the matrix does exercise those ties)
    bad = np.flatnonzero((_u64(P) != _u64(prim)).any(axis=1))
    assert not len(bad), f"Prim step {bad[0]}: device {P[bad[0]]}, reference {prim[bad[0]]}"
    assert (_u64(Z) == _u64(er.relabel(prim[:, :3], n))).all()
    if n == LDS_NODES:   # the largest size that may keep D[] in LDS, with D[] in global memory
        monkeypatch.setenv("KSP_PRIM_LDS", "0")
        P0, Z0 = _on_device((engine.single_linkage_prim, engine.single_linkage_rows), M, n)
        assert (_u64(P0) == _u64(P)).all() and (_u64(Z0) == _u64(Z)).all()
    print(f"\nn = {n}: device {t1 - t0:.1f} s, reference distances {t2 - t1:.1f} s, Prim replay {t3 - t2:.1f} s")


@pytest.mark.parametrize("n,lds", [(LDS_NODES + 1, True), (LDS_NODES, True), (LDS_NODES, False)])
def test_linkage_of_the_zero_matrix(n, lds, monkeypatch):
    """All ties: every distance is 0, so only step 0 lowers D[] and every step takes the first unmerged index: Prim's
    rows are (k, k + 1, 0, 0)."""
    if not lds:
        monkeypatch.setenv("KSP_PRIM_LDS", "0")
    P, Z = _on_device((engine.single_linkage_prim, engine.single_linkage_rows), np.zeros((n, n)), n)
    k = np.arange(n - 1, dtype=np.float64)
    want = np.stack([k, k + 1, np.zeros(n - 1), np.zeros(n - 1)], axis=1)
    bad = np.flatnonzero((_u64(P) != _u64(want)).any(axis=1))
    assert not len(bad), f"Prim step {bad[0]}: {P[bad[0]]}"
    assert (_u64(Z) == _u64(er.relabel(want[:, :3], n))).all()


def _band(n, seed):
    """M[i, i + 1] = w[i] and M[i, i + 3] = v[i] (and their mirror images), w and v in 1..7: every squared row distance
    is an integer far below 2^53, exact in any order of summation, and its sqrt the correctly rounded root."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 8, size=n - 1), rng.integers(1, 8, size=n - 3)


def _band_entries(w, v, r0, r1, n):
    """(row - r0, column, value) of the band entries of the rows r0 <= r < r1."""
    r = np.arange(r0, r1)
    parts = []
    for off, vals, ok in ((1, w, r + 1 < n), (-1, w, r >= 1), (3, v, r + 3 < n), (-3, v, r >= 3)):
        rr = r[ok]
        parts.append((rr - r0, rr + off, vals[np.minimum(rr, rr + off)]))
    return [np.concatenate(x) for x in zip(*parts)]


def _band_prim(w, v, n):
    """export_restate.prim_rows(distances, nearest=True) of the band matrix, without the matrix: dist^2(x, j) =
    |x|^2 + |j|^2 - 2 <x, j>, and <x, j> != 0 only for |x - j| in {2, 4, 6} (both offsets are odd), whose distances
    are summed exactly from the two rows.  O(n) per step."""
    wf, vf = w.astype(np.float64), v.astype(np.float64)
    norm2 = np.zeros(n)
    norm2[:-1] += wf * wf
    norm2[1:] += wf * wf
    norm2[:-3] += vf * vf
    norm2[3:] += vf * vf

    def row(i):
        return {c: int(val) for c, val, ok in ((i + 1, w[min(i, n - 2)], i + 1 < n), (i - 1, w[i - 1], i >= 1),
                                                (i + 3, v[min(i, n - 4)], i + 3 < n), (i - 3, v[i - 3], i >= 3)) if ok}

    Dm = np.full(n, np.inf)
    pen = np.zeros(n)                  # +inf once merged: such a node is never lowered and never the minimum
    near = np.zeros(n, dtype=np.int64)
    d = np.empty(n)
    lower = np.empty(n, dtype=bool)
    out = np.empty((n - 1, 4))
    x = 0
    for k in range(n - 1):
        pen[x] = Dm[x] = np.inf
        np.add(norm2, norm2[x], out=d)
        np.sqrt(d, out=d)
        rx = row(x)
        for j in (x - 6, x - 4, x - 2, x + 2, x + 4, x + 6):
            if 0 <= j < n:
                rj = row(j)
                d[j] = math.sqrt(sum((rx.get(c, 0) - rj.get(c, 0)) ** 2 for c in rx.keys() | rj.keys()))
        d += pen
        np.greater(Dm, d, out=lower)   # scipy: if D[i] > d
        np.copyto(Dm, d, where=lower)
        np.copyto(near, x, where=lower)
        y = int(np.argmin(Dm))         # the first index of the minimum
        out[k] = (x, y, Dm[y], near[y])
        x = y
    return out


def test_linkage_at_the_node_limit():
    """n = 65 536: n^2 = 2^32 distances (a 32-bit element count would be 0), the largest grid of k_row_dist, D[] in
    global memory, 65 535 Prim steps, and many exact ties from the small integer weights.  The matrix is filled on the
    device a block of rows at a time (never whole on the host); Prim is replayed on the host from the band alone.  The
    distance matrix itself (34 GB) is not read back."""
    n = MAX_NODES
    w, v = _band(n, 65536)
    t0 = time.perf_counter()
    buf = engine.DeviceBuffer(n * n * 8)
    try:
        R = 1024
        block = np.zeros((R, n))
        for r0 in range(0, n, R):
            lr, c, val = _band_entries(w, v, r0, r0 + R, n)
            block[lr, c] = val
            rc = engine.lib().ksp_memcpy_h2d(buf.ptr.value + r0 * n * 8, block.ctypes.data, block.nbytes)
            assert rc == engine.KSP_OK, engine.lib().ksp_last_error()
            block[lr, c] = 0.0
        del block
        t1 = time.perf_counter()
        P = engine.single_linkage_prim(buf.ptr.value, n)
        t2 = time.perf_counter()
        Z = engine.single_linkage_rows(buf.ptr.value, n)
        t3 = time.perf_counter()
    finally:
        buf.free()
    want = _band_prim(w, v, n)
    t4 = time.perf_counter()
    bad = np.flatnonzero((_u64(P) != _u64(want)).any(axis=1))
    assert not len(bad), f"Prim step {bad[0]}: device {P[bad[0]]}, replay {want[bad[0]]}"
    assert (_u64(Z) == _u64(er.relabel(want[:, :3], n))).all()
    print(f"\nn = {n}: upload {t1 - t0:.1f} s, single_linkage_prim {t2 - t1:.1f} s, single_linkage_rows {t3 - t2:.1f} s, "
          f"host replay {t4 - t3:.1f} s")
