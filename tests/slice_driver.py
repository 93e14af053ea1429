"""The sliced stage 1 driven call by call on one GPU, as run_multi (multi.hip) and kspider_amd/dist.py drive it between
devices: build every slice up to its labels, MIN-combine the labels (for slices of an inverted index also SUM-combine
the counter bounds), finish every slice in that source order, export, stack the slices as the exchange would, assemble,
join."""
import numpy as np

from kspider_amd import engine


def _sorted(ev):
    key = (ev["source_1"].astype(np.uint64) << np.uint64(32)) | ev["source_2"].astype(np.uint64)
    return ev[np.argsort(key, kind="stable")]


def _run(n_sources, nparts, build, sum_bounds=False):
    """build(e, p): the slice build of part p on engine e.  sum_bounds: the slices hold a share of every source's keys
    (an inverted index), so their per-source counter bounds are added up and set on every slice before it is finished.
    Returns (edges, sizes: flat nparts x 4 slice_sizes(), stats after the assemble and the join)."""
    e = engine.Engine(0)
    nb = None
    # what the ranks' MIN all-reduce does: element-wise minimum of the slices' source labels
    lab = engine.DeviceBuffer(max(4, n_sources * 4))
    labels = np.full(n_sources, 0xFFFFFFFF, dtype=np.uint32)
    bounds = np.zeros(n_sources, dtype=np.uint64)
    for p in range(nparts):
        build(e, p)
        e.slice_labels(lab.ptr.value)
        nb = e.stats()["n_blocks"]   # (blocks of the build: may hold spare ones for cluster-aligned boundaries)
        labels = np.minimum(labels, lab.to_numpy(np.uint32, n_sources))
        if sum_bounds:   # (the ranks' SUM all-reduce)
            e.slice_bounds(lab.ptr.value)
            bounds += lab.to_numpy(np.uint32, n_sources)
    lab = engine.DeviceBuffer.from_numpy(labels) if n_sources else lab
    bnd = engine.DeviceBuffer.from_numpy(np.minimum(bounds, 0xFFFFFFFF).astype(np.uint32)) if sum_bounds and n_sources else None
    sizes, parts = [], []
    for p in range(nparts):
        build(e, p)
        if bnd:
            e.slice_set_bounds(bnd.ptr.value)
        e.slice_finish(lab.ptr.value)
        sz = e.slice_sizes()
        L, nbig = int(sz[0]), int(sz[2])
        bufs = dict(brk=engine.DeviceBuffer(max(4, L * 4)), info=engine.DeviceBuffer(max(4, L * 4)),
                    bw=engine.DeviceBuffer(max(4, L * 4)), raw=engine.DeviceBuffer((nb + 1) * 4),
                    pos=engine.DeviceBuffer((nb + 1) * 4), big=engine.DeviceBuffer(max(16, nbig * 16)))
        e.slice_export(bufs["brk"].ptr.value, bufs["info"].ptr.value, bufs["bw"].ptr.value, bufs["raw"].ptr.value,
                       bufs["pos"].ptr.value, bufs["big"].ptr.value)
        host = {k: b.to_numpy(np.uint8, b.nbytes) for k, b in bufs.items()}
        for b in bufs.values():
            b.free()
        sizes.append(sz)
        parts.append(host)
    sizes = np.concatenate(sizes)
    lstride = max(1, int(sizes[0::4].max()))
    bigstride = max(1, int(sizes[2::4].max()))

    def stack(key, row_bytes):
        out = np.zeros((nparts, row_bytes), dtype=np.uint8)
        for p, h in enumerate(parts):
            n = min(row_bytes, h[key].size)
            out[p, :n] = h[key][:n]
        return engine.DeviceBuffer.from_numpy(out)

    brk_all, info_all, bw_all = stack("brk", lstride * 4), stack("info", lstride * 4), stack("bw", lstride * 4)
    raw_all, pos_all = stack("raw", (nb + 1) * 4), stack("pos", (nb + 1) * 4)
    big_all = stack("big", bigstride * 16)
    e.assemble(sizes, brk_all.ptr.value, info_all.ptr.value, bw_all.ptr.value, lstride, raw_all.ptr.value,
               pos_all.ptr.value, big_all.ptr.value, bigstride)
    T = e.num_tiles
    cap = max(16, e.edge_bound(0, T) + 1)
    de = engine.DeviceBuffer(cap * 16)
    cnt = e.join(0, T, de.ptr.value, cap)
    edges = _sorted(de.to_numpy(engine.EDGE_DTYPE, cnt))
    st = e.stats()
    if bnd:
        bnd.free()
    for b in (de, lab, brk_all, info_all, bw_all, raw_all, pos_all, big_all):
        b.free()
    e.close()
    return edges, sizes, st


def sliced_edges(sk, nparts, weights=None, key_bits=0):
    """Key-range slices of sketches (`sk`: anything with .keys, .offsets, .n_sources)."""
    dk = engine.DeviceBuffer.from_numpy(sk.keys) if sk.keys.size else engine.DeviceBuffer(8)
    dw = engine.DeviceBuffer.from_numpy(weights) if weights is not None else None

    def build(e, p):
        e.build_slice(dk.ptr.value, sk.offsets, p, nparts, d_weights_ptr=dw.ptr.value if dw else 0, key_bits=key_bits)

    try:
        return _run(sk.n_sources, nparts, build)
    finally:
        dk.free()
        if dw:
            dw.free()


def sliced_postings_edges(key_off, sources, key_weights, n_sources, cuts, sum_bounds=True):
    """Slices of an inverted index: slice s holds the keys [cuts[s], cuts[s + 1]) with all their holders.
    sum_bounds False: the caller that leaves slice_bounds / slice_set_bounds out."""
    key_off = np.ascontiguousarray(key_off, dtype=np.uint64)
    sources = np.ascontiguousarray(sources, dtype=np.uint32)
    ds = engine.DeviceBuffer.from_numpy(sources) if sources.size else engine.DeviceBuffer(4)
    dw = None
    if key_weights is not None:
        kw = np.ascontiguousarray(key_weights, dtype=np.uint32)
        dw = engine.DeviceBuffer.from_numpy(kw) if kw.size else engine.DeviceBuffer(4)

    def build(e, p):
        k0, k1 = int(cuts[p]), int(cuts[p + 1])
        off = key_off[k0:k1 + 1] - key_off[k0]
        e.build_postings_slice(off, ds.ptr.value + 4 * int(key_off[k0]), (dw.ptr.value + 4 * k0) if dw else 0, n_sources)

    try:
        return _run(n_sources, len(cuts) - 1, build, sum_bounds=sum_bounds)
    finally:
        ds.free()
        if dw:
            dw.free()


class Sketches:
    """(keys, offsets) with the attributes the drivers read."""

    def __init__(self, keys, offsets):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n_sources = self.offsets.size - 1
