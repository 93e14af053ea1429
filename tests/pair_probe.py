"""Exact full-size check of an edge set (a Freivalds check on the pair matrix), for the tests.

The pair matrix of a sketch set is S = sum_k w_k (1_H 1_H^T - diag), H the holders of key k (w_k = 1 unless weighted):
S[a, b] = shared(a, b).  For random u, v:
  * key side, from the inputs only:   u^T S v = sum_k w_k ((sum_H u)(sum_H v) - sum_H u v);
  * edge side, from the output only:  u^T S v = sum_edges shared (u_a v_b + u_b v_a);
both modulo 2^64.  With two independent probes, every row sum, the total, and edges that are sorted, unique, a < b < N
and shared > 0, a wrong edge set passes with negligible probability — including errors that keep the total and every row
sum (a 4-cycle of +-1), which sampled rows and pairs almost never see.  Fixed seeds make any failure reproduce.

The key side never reads engine output and the edge side never reads keys.  The grouping by key (one threaded sort in
oracle.key_index: the caller's keys plus 12 bytes per entry, 6 GB on top of C3's 4 GB of keys) and the key-side sums
(oracle.key_probe / key_rows, no gathered copies) run once per sketch set; KeyIndex caches its key sides.
"""
import numpy as np

import oracle

MASK = (1 << 64) - 1
_CHUNK = 1 << 22


class KeyIndex:
    """The keys of a sketch set held by two sources or more, grouped: keys[k] ascending, its holders
    sources[key_off[k]:key_off[k + 1]] ascending.  Keys held once do not enter S and are left out."""

    def __init__(self, keys, offsets, threads=None):
        offsets = np.asarray(offsets, dtype=np.uint64)
        self.n_sources = offsets.size - 1
        self.sizes = np.diff(offsets.astype(np.int64))
        self.keys, self.key_off, self.sources = oracle.key_index(keys, offsets, threads)
        self.counts = np.diff(self.key_off.astype(np.int64))   # m_k >= 2
        self._expected = {}

    @property
    def postings(self):
        """(key_off, sources): the input of engine.pairwise_postings_host, from the same grouping."""
        return self.key_off, self.sources

    def holders_of(self, q):
        """Number of holders of every key in q (a key absent from the index is held once)."""
        q = np.asarray(q, dtype=np.uint64)
        j = np.minimum(np.searchsorted(self.keys, q), max(0, self.keys.size - 1))
        hit = self.keys[j] == q if self.keys.size else np.zeros(q.size, dtype=bool)
        return np.where(hit, self.counts[j] if self.keys.size else 0, 1)

    def expected(self, w=None, probes=2, seed=0):
        """(rows, total, [(u, v, u^T S v)] * probes) of S with per-key weights w; computed once per (w, probes, seed)."""
        tag = (None if w is None else id(w), probes, seed)
        if tag not in self._expected:
            if w is not None:
                assert len(w) == self.keys.size
            rows, total = key_rows(self, w)
            uvs = _probe_vectors(self.n_sources, probes, seed)
            fps = oracle.key_probe(self.key_off, self.sources, w, self.n_sources,
                                   np.stack([u for u, _ in uvs]) if probes else np.zeros((0, self.n_sources), np.uint64),
                                   np.stack([v for _, v in uvs]) if probes else np.zeros((0, self.n_sources), np.uint64))
            self._expected[tag] = (w, rows, total, [(u, v, int(f)) for (u, v), f in zip(uvs, fps)])
        return self._expected[tag][1:]


def _probe_vectors(n, probes, seed):
    rng = np.random.default_rng([seed, n])
    return [(rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False),
             rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)) for _ in range(probes)]


def key_index(keys, offsets, threads=None) -> KeyIndex:
    return KeyIndex(keys, offsets, threads)


def key_fingerprint(index: KeyIndex, u, v, w=None) -> int:
    """u^T S v mod 2^64 from the keys: sum_k w_k ((sum_H u)(sum_H v) - sum_H u v)."""
    u = np.asarray(u, dtype=np.uint64).reshape(1, -1)
    v = np.asarray(v, dtype=np.uint64).reshape(1, -1)
    return int(oracle.key_probe(index.key_off, index.sources, w, index.n_sources, u, v)[0])


def key_rows(index: KeyIndex, w=None):
    """(row sums sum_{k held by a} w_k (m_k - 1) of all N sources as uint64, total sum_k w_k C(m_k, 2)), in integers."""
    return oracle.key_rows(index.key_off, index.sources, w, index.n_sources)


def edge_fingerprint(edges, u, v) -> int:
    """u^T S v mod 2^64 from the edges: sum shared (u_a v_b + u_b v_a)."""
    u = np.asarray(u, dtype=np.uint64)
    v = np.asarray(v, dtype=np.uint64)
    acc = 0
    for i in range(0, len(edges), _CHUNK):
        e = edges[i:i + _CHUNK]
        a, b, s = e["source_1"], e["source_2"], e["shared"].astype(np.uint64)
        t = u[a] * v[b]            # (uint64 arrays wrap modulo 2^64)
        t += u[b] * v[a]
        t *= s
        acc = (acc + int(t.sum(dtype=np.uint64))) & MASK
    return acc


def edge_rows(edges, n):
    """Row sums of the edge set: sum_b shared(a, b) over both ends, as uint64[n]."""
    rows = np.zeros(n, dtype=np.uint64)
    s = edges["shared"].astype(np.uint64)
    np.add.at(rows, edges["source_1"], s)
    np.add.at(rows, edges["source_2"], s)
    return rows


def _first(bad):
    return int(np.flatnonzero(bad)[0])


def check_edge_set(edges, index: KeyIndex, n_sources=None, w=None, probes=2, seed=20241008):
    """Assert that `edges` (EDGE_DTYPE) is exactly the edge set of S; the message names the failing check."""
    n = index.n_sources if n_sources is None else int(n_sources)
    assert n == index.n_sources, f"n_sources {n} != {index.n_sources} of the index"
    rows_want, total_want, fps = index.expected(w, probes, seed)
    a, b, s = edges["source_1"], edges["source_2"], edges["shared"]
    if len(edges):
        bad = a >= b
        assert not bad.any(), f"order: edge {_first(bad)} has source_1 {a[_first(bad)]} >= source_2 {b[_first(bad)]}"
        assert int(b.max()) < n, f"range: edge {int(np.argmax(b))} has source_2 {int(b.max())} >= N = {n}"
        key = (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
        bad = key[1:] <= key[:-1]
        assert not bad.any(), (f"sorted/unique: edge {_first(bad) + 1} ({a[_first(bad) + 1]}, {b[_first(bad) + 1]}) "
                               f"follows ({a[_first(bad)]}, {b[_first(bad)]})")
        bad = s == 0
        assert not bad.any(), f"shared > 0: edge {_first(bad)} ({a[_first(bad)]}, {b[_first(bad)]}) has shared 0"
        if w is None:
            bad = s > np.minimum(index.sizes[a], index.sizes[b]).astype(np.uint64)
            assert not bad.any(), (f"shared <= min(n_a, n_b): edge {_first(bad)} ({a[_first(bad)]}, {b[_first(bad)]}) "
                                   f"has shared {s[_first(bad)]}")
    total = int(s.sum(dtype=np.uint64)) if len(edges) else 0
    assert total == total_want, f"total: sum of shared {total} != sum_k w_k C(m_k, 2) = {total_want}"
    rows = edge_rows(edges, n)
    bad = rows != rows_want
    assert not bad.any(), (f"rows: {int(bad.sum())} of {n} row sums differ, first source {_first(bad)}: "
                           f"edges {rows[_first(bad)]} != keys {rows_want[_first(bad)]}")
    for j, (u, v, want) in enumerate(fps):
        got = edge_fingerprint(edges, u, v)
        assert got == want, f"probe {j} (seed {seed}): u^T S v from the edges {got:#x} != from the keys {want:#x}"


_LAST = {}


def config(cfg, n_sources=None):
    """(SketchSet, KeyIndex) of a BASELINE config, generated and grouped once; one config is kept at a time (C3's keys
    and index hold ~10 GB of host memory), so tests of one config share it when they run one after another."""
    from kspider_amd import synth
    tag = (cfg, n_sources)
    if tag not in _LAST:
        _LAST.clear()
        sk = synth.generate(cfg, n_sources=n_sources)
        _LAST[tag] = (sk, KeyIndex(sk.keys, sk.offsets))
    return _LAST[tag]


def sort_edges(ev):
    """Edges in (source_1, source_2) order (an argsort of one uint64 key: faster than a structured sort)."""
    key = (ev["source_1"].astype(np.uint64) << np.uint64(32)) | ev["source_2"].astype(np.uint64)
    return ev[np.argsort(key, kind="stable")]
