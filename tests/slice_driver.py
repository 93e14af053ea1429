"""The sliced stage 1 driven call by call on one GPU, as run_multi (multi.hip) and kspider_amd/dist.py drive it between
devices: build every slice up to its labels, MIN-combine the labels (for slices of an inverted index also SUM-combine
the counter bounds), finish every slice in that source order, export, stack the slices as the exchange would, assemble,
join.

`_run` (and sliced_edges / sliced_postings_edges above it) makes an engine of its own and runs the whole protocol; given
an `engine_` it works on the caller's (and leaves it open), and given a `stop` it leaves the protocol there."""
import numpy as np

from kspider_amd import engine

# where a protocol can be left (`stop`), in protocol order
STOPS = ("build",        # after the first build_slice
         "labels",       # after slice_labels of the last slice (the first pass is over, but for that slice's bounds)
         "set_bounds",   # second pass, last slice: built again (and, with summed bounds, slice_set_bounds called)
         "finish",       # ... after its slice_finish
         "export",       # ... after its slice_sizes / slice_export
         "assemble")     # after assemble: joinable, the driver's own join left out


def _sorted(ev):
    key = (ev["source_1"].astype(np.uint64) << np.uint64(32)) | ev["source_2"].astype(np.uint64)
    return ev[np.argsort(key, kind="stable")]


class Protocol:
    """The steps of _run on engine `e`, one method each, for callers that go through them by themselves.
    build(e, p): the slice build of part p on engine e.  sum_bounds: the slices hold a share of every source's keys (an
    inverted index), so their per-source counter bounds are added up and set on every slice before it is finished.
    hook(where, p): called between the protocol's calls, for tests that put calls of their own there; where is "built"
    (first pass, part p built), "rebuilt" (second pass, part p built again), "finished" or "exported"."""

    def __init__(self, e, n_sources, nparts, build, sum_bounds=False, hook=None):
        self.e, self.n_sources, self.nparts, self.build, self.sum_bounds = e, n_sources, nparts, build, sum_bounds
        self.hook = hook or (lambda where, p: None)
        self.nb = None
        self.lab = engine.DeviceBuffer(max(4, n_sources * 4))    # combined labels once first_pass() is through
        self.bnd = None                                          # summed bounds (sum_bounds)
        self.sizes, self.parts = [], []
        self.stacked = None

    def first_pass(self, stop=None):
        """Every slice up to its labels; what the ranks' MIN all-reduce does: the element-wise minimum of the slices'
        source labels.  True: stopped at `stop`."""
        e, n_sources, lab = self.e, self.n_sources, self.lab
        labels = np.full(n_sources, 0xFFFFFFFF, dtype=np.uint32)
        bounds = np.zeros(n_sources, dtype=np.uint64)
        for p in range(self.nparts):
            self.build(e, p)
            if stop == "build":
                return True
            self.hook("built", p)
            e.slice_labels(lab.ptr.value)
            if stop == "labels" and p == self.nparts - 1:
                return True
            self.nb = e.stats()["n_blocks"]   # (blocks of the build: may hold spare ones for cluster-aligned boundaries)
            labels = np.minimum(labels, lab.to_numpy(np.uint32, n_sources))
            if self.sum_bounds:   # (the ranks' SUM all-reduce)
                e.slice_bounds(lab.ptr.value)
                bounds += lab.to_numpy(np.uint32, n_sources)
        if n_sources:
            self.lab = engine.DeviceBuffer.from_numpy(labels)
            lab.free()
        if self.sum_bounds and n_sources:
            self.bnd = engine.DeviceBuffer.from_numpy(np.minimum(bounds, 0xFFFFFFFF).astype(np.uint32))
        return False

    def second_pass(self, stop=None):
        """Every slice built again, finished in the combined source order and exported to the host.  True: stopped."""
        e, nb = self.e, self.nb
        for p in range(self.nparts):
            last = p == self.nparts - 1
            self.build(e, p)
            self.hook("rebuilt", p)
            if self.bnd:
                e.slice_set_bounds(self.bnd.ptr.value)
            if stop == "set_bounds" and last:
                return True
            e.slice_finish(self.lab.ptr.value)
            if stop == "finish" and last:
                return True
            self.hook("finished", p)
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
            self.sizes.append(sz)
            self.parts.append(host)
            self.hook("exported", p)
            if stop == "export" and last:
                return True
        return False

    def stack(self):
        """The exported slices side by side on the device, as the exchange between the ranks leaves them."""
        nparts, nb, parts = self.nparts, self.nb, self.parts
        self.sizes = sizes = np.concatenate(self.sizes)
        self.lstride = lstride = max(1, int(sizes[0::4].max()))
        self.bigstride = bigstride = max(1, int(sizes[2::4].max()))

        def stack(key, row_bytes):
            out = np.zeros((nparts, row_bytes), dtype=np.uint8)
            for p, h in enumerate(parts):
                n = min(row_bytes, h[key].size)
                out[p, :n] = h[key][:n]
            return engine.DeviceBuffer.from_numpy(out)

        self.stacked = [stack("brk", lstride * 4), stack("info", lstride * 4), stack("bw", lstride * 4),
                        stack("raw", (nb + 1) * 4), stack("pos", (nb + 1) * 4), stack("big", bigstride * 16)]

    def assemble(self, e=None):
        """(e: another engine than the protocol's, on which a slice of the same input has been finished)"""
        brk_all, info_all, bw_all, raw_all, pos_all, big_all = self.stacked
        (e or self.e).assemble(self.sizes, brk_all.ptr.value, info_all.ptr.value, bw_all.ptr.value, self.lstride,
                               raw_all.ptr.value, pos_all.ptr.value, big_all.ptr.value, self.bigstride)

    def join(self):
        e = self.e
        T = e.num_tiles
        cap = max(16, e.edge_bound(0, T) + 1)
        de = engine.DeviceBuffer(cap * 16)
        cnt = e.join(0, T, de.ptr.value, cap)
        edges = _sorted(de.to_numpy(engine.EDGE_DTYPE, cnt))
        de.free()
        return edges

    def free(self):
        for b in [self.bnd, self.lab] + (self.stacked or []):
            if b:
                b.free()
        self.bnd = self.stacked = None


def _run(n_sources, nparts, build, sum_bounds=False, engine_=None, stop=None):
    """build(e, p): the slice build of part p on engine e.  sum_bounds: the slices hold a share of every source's keys
    (an inverted index), so their per-source counter bounds are added up and set on every slice before it is finished.
    engine_: the engine to work on (left open; default: one of the driver's own, closed at the end).  stop: one of STOPS.
    Returns (edges, sizes: flat nparts x 4 slice_sizes(), stats after the assemble and the join); stopped: (None, the
    sizes so far or None, the stats at the stop)."""
    assert stop is None or stop in STOPS, stop
    e = engine_ if engine_ is not None else engine.Engine(0)
    pr = Protocol(e, n_sources, nparts, build, sum_bounds)
    try:
        if pr.first_pass(stop) or pr.second_pass(stop):
            return None, (np.concatenate(pr.sizes) if pr.sizes else None), e.stats()
        pr.stack()
        pr.assemble()
        if stop == "assemble":
            return None, pr.sizes, e.stats()
        edges = pr.join()
        return edges, pr.sizes, e.stats()
    finally:
        pr.free()
        if engine_ is None:
            e.close()


def sketch_slice_build(dk_ptr, offsets, nparts, dw_ptr=0, key_bits=0):
    """build(e, p) of key-range slices of sketches whose keys (and weights) are on the device already."""
    def build(e, p):
        e.build_slice(dk_ptr, offsets, p, nparts, d_weights_ptr=dw_ptr, key_bits=key_bits)
    return build


def postings_slice_build(key_off, ds_ptr, dw_ptr, n_sources, cuts):
    """build(e, p) of slices of an inverted index on the device: slice p holds the keys [cuts[p], cuts[p + 1])."""
    def build(e, p):
        k0, k1 = int(cuts[p]), int(cuts[p + 1])
        off = key_off[k0:k1 + 1] - key_off[k0]
        e.build_postings_slice(off, ds_ptr + 4 * int(key_off[k0]), (dw_ptr + 4 * k0) if dw_ptr else 0, n_sources)
    return build


def sliced_edges(sk, nparts, weights=None, key_bits=0, engine_=None, stop=None):
    """Key-range slices of sketches (`sk`: anything with .keys, .offsets, .n_sources)."""
    dk = engine.DeviceBuffer.from_numpy(sk.keys) if sk.keys.size else engine.DeviceBuffer(8)
    dw = engine.DeviceBuffer.from_numpy(weights) if weights is not None else None
    build = sketch_slice_build(dk.ptr.value, sk.offsets, nparts, dw.ptr.value if dw else 0, key_bits)
    try:
        return _run(sk.n_sources, nparts, build, engine_=engine_, stop=stop)
    finally:
        dk.free()
        if dw:
            dw.free()


def sliced_postings_edges(key_off, sources, key_weights, n_sources, cuts, sum_bounds=True, engine_=None, stop=None):
    """Slices of an inverted index: slice s holds the keys [cuts[s], cuts[s + 1]) with all their holders.
    sum_bounds False: the caller that leaves slice_bounds / slice_set_bounds out."""
    key_off = np.ascontiguousarray(key_off, dtype=np.uint64)
    sources = np.ascontiguousarray(sources, dtype=np.uint32)
    ds = engine.DeviceBuffer.from_numpy(sources) if sources.size else engine.DeviceBuffer(4)
    dw = None
    if key_weights is not None:
        kw = np.ascontiguousarray(key_weights, dtype=np.uint32)
        dw = engine.DeviceBuffer.from_numpy(kw) if kw.size else engine.DeviceBuffer(4)
    build = postings_slice_build(key_off, ds.ptr.value, dw.ptr.value if dw else 0, n_sources, cuts)
    try:
        return _run(n_sources, len(cuts) - 1, build, sum_bounds=sum_bounds, engine_=engine_, stop=stop)
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
