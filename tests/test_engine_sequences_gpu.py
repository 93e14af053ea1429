"""One engine over many calls: seeded sequences of builds, joins, refused calls and mode switches on a single Engine,
every result against the oracle; the sticky fall-backs of one input against the next; the engine's entries on a stream
of their own.

The engine keeps a lot from one call to the next (grown buffers that are never cleared, zeroing and staging flags, the
offsets of the last build, fall-backs that hold for the rest of its life).  The other suites mostly build once per
engine; here the pool of inputs is walked big -> small -> big, so stale buffers hold the data of a bigger build.

Sections E to G put the slice protocol (build_slice ... assemble, tests/slice_driver.py) into such sequences: whole builds
behind a slice left at any phase, refused builds inside a protocol, slice calls out of order, slices as operations of
the seeded sequences, and seeded walks over the state table of tests/engine_states.py."""
import ctypes
import functools

import numpy as np
import pytest

from kspider_amd import engine, synth

import engine_states as ES
from slice_driver import STOPS, Protocol, postings_slice_build, sketch_slice_build
from slice_driver import _run as slice_run
from test_fuzz_gpu import MODES
from test_slices_edges_gpu import SLICE_MODES

pytestmark = pytest.mark.gpu

ENV_KNOBS = ("KSP_REORDER", "KSP_NO_SCHED", "KSP_COLLECT", "KSP_JOIN", "KSP_TAG32", "KSP_HASH_GROUP", "KSP_KEY_GROUPS",
             "KSP_PART_MIN", "KSP_PARTITION", "KSP_ALIGN", "KSP_SEG", "KSP_MS", "KSP_FUSED", "KSP_DEBUG_FK_GB",
             "KSP_DEBUG_PART_SORTED", "KSP_DEBUG_LABEL_SPREAD", "KSP_DEBUG_LATE_SCHED", "KSP_FULL_SORT")
CAP = 1 << 23          # edges of a device buffer: above the edge bound of every pool input (n3000: 4.5 M source pairs)
WEIGHTED_MODES = ({}, {"KSP_REORDER": "0"}, {"KSP_NO_SCHED": "1"}, {"KSP_KEY_GROUPS": "0"})   # (test_fuzz_gpu's weighted modes)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---- inputs and their oracle ---------------------------------------------------------------------------------------

def _canon(edges):
    """Edges in (source_1, source_2) order (device joins return them in any order)."""
    k = (edges["source_1"].astype(np.uint64) << np.uint64(32)) | edges["source_2"].astype(np.uint64)
    return edges[np.argsort(k, kind="stable")]


def _postings(keys, offsets):
    """Keys held by two sources or more -> (key values, key_off uint64, holders uint32 ascending per key)."""
    n = offsets.size - 1
    src = np.repeat(np.arange(n, dtype=np.uint32), np.diff(offsets).astype(np.int64))
    order = np.argsort(keys, kind="stable")
    k, s = keys[order], src[order]
    if k.size == 0:
        return k, np.zeros(1, dtype=np.uint64), s
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    counts = np.diff(np.concatenate([starts, [k.size]]))
    keep = counts >= 2
    sel = np.repeat(keep, counts)
    key_off = np.zeros(int(keep.sum()) + 1, dtype=np.uint64)
    key_off[1:] = np.cumsum(counts[keep])
    return k[starts[keep]], key_off, s[sel]


def _weighted_ref(oracle, key_off, holders, key_w):
    _, _, _, ref = oracle.accumulate_mem(key_off.astype(np.uint32), holders, key_w)
    return _canon(ref)


class Input:
    """One pool entry: sketches (keys, offsets[, per-entry weights]) or postings (key_off, holders[, key weights])."""

    def __init__(self, name, oracle, keys=None, offsets=None, weights=None, postings=None, n_sources=None):
        self.name = name
        if postings is not None:
            self.kind = "post"
            self.key_off, self.holders, self.key_w = postings
            self.n_sources = n_sources
            self.n_entries = int(self.key_off[-1])
            self.weighted = self.key_w is not None
            if self.weighted:
                self.ref = _weighted_ref(oracle, self.key_off, self.holders, self.key_w)
            else:
                self.ref = _weighted_ref(oracle, self.key_off, self.holders, np.ones(self.key_off.size - 1, dtype=np.uint32))
            self.d_srcbuf = engine.DeviceBuffer.from_numpy(self.holders if self.holders.size else np.zeros(1, np.uint32))
            self.d_wbuf = engine.DeviceBuffer.from_numpy(self.key_w) if self.weighted else None
            self.width = 0
            return
        self.kind = "sk"
        self.keys, self.offsets, self.weights = keys, offsets, weights
        self.n_sources = offsets.size - 1
        self.n_entries = int(offsets[-1]) if offsets.size > 1 else 0
        self.weighted = weights is not None
        self.width = int(keys.max()).bit_length() if keys.size else 0
        if self.weighted:
            uk, key_off, holders = _postings(keys, offsets)
            # per-entry weights are the key's weight (a colour weight): the engine sums the weights of the shared keys
            w_of = dict(zip(keys.tolist(), weights.tolist()))
            kw = np.array([w_of[int(k)] for k in uk], dtype=np.uint32)
            self.ref = _weighted_ref(oracle, key_off, holders, kw)
        else:
            self.ref = oracle.brute_pairs(keys, offsets)
        self.d_keys = engine.DeviceBuffer.from_numpy(keys if keys.size else np.zeros(1, np.uint64))
        self.d_wbuf = engine.DeviceBuffer.from_numpy(weights) if self.weighted else None

    @property
    def d_weights(self):
        return self.d_wbuf.ptr.value if self.d_wbuf is not None else 0

    def build(self, e, key_bits=0, stream=0):
        if self.kind == "post":
            e.build_postings(self.key_off, self.d_srcbuf.ptr.value, self.d_weights, self.n_sources, stream=stream)
        else:
            e.build_blocks(self.d_keys.ptr.value, self.offsets, d_weights_ptr=self.d_weights, key_bits=key_bits, stream=stream)


def _key_weights_for(keys, rng):
    """Per-entry weights that agree for equal keys (a colour weight per key), in [1, 1000]."""
    uk, inv = np.unique(keys, return_inverse=True)
    return rng.integers(1, 1001, size=uk.size, dtype=np.uint32)[inv].astype(np.uint32)


def _twin(sk, seed):
    """The same offsets with other keys: new sorted-unique runs of the same lengths, drawn from a small universe so that
    they share a lot (a different edge set: an engine that kept the old keys or the old lists gives the old edges)."""
    rng = np.random.default_rng(seed)
    lens = np.diff(sk.offsets).astype(np.int64)
    universe = max(8, int(lens.max()) * 3) if lens.size else 8
    runs = [np.sort(rng.choice(universe, size=int(L), replace=False).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
            for L in lens]
    out = synth.from_runs(runs)
    assert (out.offsets == sk.offsets).all()
    return out


def top32_set():
    """5 000 distinct keys of 60 bits that agree in their top 32: the prefix sort overflows, the build is repeated with the
    full-width sort and the engine keeps the full sort from then on (full_sort)."""
    rng = np.random.default_rng(12)
    giant = (np.uint64(0xABCDEF01) << np.uint64(28)) | rng.integers(0, 1 << 28, size=5000, dtype=np.uint64)
    return synth.from_runs([giant[rng.integers(0, giant.size, size=300)] for _ in range(150)])


def skewed_set():
    """test_partition_gpu's skewed keys: the hand-written partition's page tables fill, the build falls back to the
    library partition and the engine keeps it (part_off)."""
    rng = np.random.default_rng(10)
    runs = []
    for s in range(700):
        low = rng.integers(0, 1 << 40, size=2500, dtype=np.uint64)
        high = rng.integers(0, 1 << 57, size=20, dtype=np.uint64)
        runs.append(np.concatenate([low, high, np.arange(s % 5, 4000, 5, dtype=np.uint64)]))
    return synth.from_runs(runs)


def holders_set():
    """Two keys held by all 2 100 sources, more than the key-by-key list build stages in LDS (2 048): the huge-key path.
    (Too few such keys for its own overflow, which would make the engine sort by block from then on: key_groups_off.)"""
    rng = np.random.default_rng(43)
    everywhere = rng.integers(0, 1 << 58, size=2, dtype=np.uint64)
    runs = [np.concatenate([rng.integers(0, 1 << 58, size=6, dtype=np.uint64), everywhere]) for _ in range(2100)]
    return synth.from_runs(runs)


def sparse_set():
    """Keys mostly shared by two sources: under KSP_FUSED=1 the bucket-resident build gives up (sparse sharing) and the
    engine builds pass by pass from then on (fused_off)."""
    rng = np.random.default_rng(55)
    return synth.from_runs([rng.integers(0, 1 << 21, size=500, dtype=np.uint64) for _ in range(1000)])


def _family_set(rng, n, universe, mean, fam_size):
    base = rng.integers(0, universe, size=fam_size, dtype=np.uint64)
    runs = []
    for _ in range(n):
        own = rng.integers(0, universe, size=int(rng.integers(0, 2 * mean + 1)), dtype=np.uint64)
        runs.append(np.concatenate([own, base[rng.random(base.size) < 0.3]]))
    return synth.from_runs(runs)


@functools.lru_cache(maxsize=None)
def _pool_cached():
    import oracle
    oracle.lib()
    rng = np.random.default_rng(7)
    pool = {}

    def add(name, sk, weights=None):
        pool[name] = Input(name, oracle, keys=sk.keys, offsets=sk.offsets, weights=weights)
        return sk

    add("empty", synth.from_runs([]))
    add("one", synth.from_runs([rng.integers(0, 1 << 40, size=50, dtype=np.uint64)]))
    add("n127", synth.generate("C2", n_sources=127, mean_size=300, cluster_cap=16, seed=101))
    add("n128", synth.generate("C2", n_sources=128, mean_size=1500, cluster_cap=20, seed=102))
    add("n129", synth.generate("C2", n_sources=129, mean_size=40, cluster_cap=8, seed=103))
    c700 = add("n700", synth.generate("C2", n_sources=700, mean_size=500, cluster_cap=50, seed=104))
    add("n3000", synth.generate("C2", n_sources=3000, mean_size=60, cluster_cap=60, seed=105))
    low = add("low20", _family_set(rng, 400, 1 << 20, 40, 3000))
    full = _family_set(rng, 300, 1 << 64, 30, 2000)
    runs = [full.keys[full.offsets[i]:full.offsets[i + 1]] for i in range(full.n_sources)]
    for i in range(0, 300, 7):            # the extreme keys 0 and 2^64 - 1, held by many sources
        runs[i] = np.concatenate([runs[i], np.array([0, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)])
    add("full64", synth.from_runs(runs))
    w = synth.generate("C2", n_sources=500, mean_size=400, cluster_cap=40, seed=106)
    add("weighted", w, _key_weights_for(w.keys, rng))
    add("weighted_low20", low, _key_weights_for(low.keys, rng))
    add("twin700", _twin(c700, 108))
    for name, f in (("top32", top32_set), ("skewed", skewed_set), ("holders", holders_set), ("sparse", sparse_set)):
        add(name, f())
    _, ko, hs = _postings(c700.keys, c700.offsets)
    perm = np.random.default_rng(5).permutation(ko.size - 1)         # keys in scrambled order
    groups = [hs[ko[i]:ko[i + 1]] for i in perm]
    ko2 = np.zeros(len(groups) + 1, dtype=np.uint64)
    ko2[1:] = np.cumsum([g.size for g in groups])
    hs2 = np.concatenate(groups).astype(np.uint32)
    pool["post700"] = Input("post700", oracle, postings=(ko2, hs2, None), n_sources=c700.n_sources)
    pool["post700w"] = Input("post700w", oracle, postings=(ko2, hs2, rng.integers(1, 1001, size=ko2.size - 1, dtype=np.uint32)),
                             n_sources=c700.n_sources)
    return pool


@pytest.fixture(scope="module")
def pool():
    return _pool_cached()


@pytest.fixture(scope="module")
def edges_buf():
    return engine.DeviceBuffer(CAP * 16)


def _got(buf, cnt):
    return _canon(buf.to_numpy(engine.EDGE_DTYPE, cnt))


def _same(got, ref):
    return len(got) == len(ref) and bool((got == ref).all())


def _full_join(e, inp, buf, stream=0):
    cnt = e.join(0, e.num_tiles, buf.ptr.value, CAP, stream=stream)
    return _got(buf, cnt)


# ---- A: seeded call sequences on one engine ------------------------------------------------------------------------

# big -> small -> big: the walk visits these in random order, but every third pick jumps between the two ends
BIG = ["n3000", "n128", "skewed", "holders", "n700", "weighted", "top32", "sparse", "post700", "post700w", "twin700"]
SMALL = ["empty", "one", "n127", "n129", "low20", "full64", "weighted_low20"]


class Runner:
    def __init__(self, seed, pool, buf, monkeypatch):
        self.seed, self.pool, self.buf, self.mp = seed, pool, buf, monkeypatch
        self.rng = np.random.default_rng(9000 + seed)
        self.e = engine.Engine(0)
        self.log = []
        self.cur = None            # input of the last good build
        self.pending = None        # (input, buffer) of a launched, uncollected join
        self.buf2 = engine.DeviceBuffer(CAP * 16)
        self.mode = {}

    def fail(self, msg):
        lines = "\n".join(f"  {i:2d}: {op}" for i, op in enumerate(self.log))
        return f"seed {self.seed}, operation {len(self.log) - 1}: {msg}\noperation log:\n{lines}"

    def check(self, cond, msg):
        assert cond, self.fail(msg)

    def pick(self, i):
        if i % 3 == 2 and self.cur is not None:     # jump to the other end of the size range
            side = SMALL if self.cur.name in BIG else BIG
        else:
            side = BIG if self.rng.random() < 0.5 else SMALL
        if self.mode not in WEIGHTED_MODES:         # (weights and postings under the modes the fuzz suite runs them in)
            side = [n for n in side if not self.pool[n].weighted and self.pool[n].kind == "sk"]
        return self.pool[side[int(self.rng.integers(len(side)))]]

    def check_stats(self, inp):
        st = self.e.stats()
        self.check(st["n_sources"] == inp.n_sources and st["n_entries"] == inp.n_entries, f"stats {st}")
        self.check(st["weighted"] == int(inp.weighted), f"weighted {st['weighted']}")
        if inp.n_sources:
            self.check(st["n_blocks"] >= -(-inp.n_sources // 128), f"n_blocks {st['n_blocks']}")
        return st

    def expect_edges(self, got, inp, what):
        self.check(_same(got, inp.ref), f"{what} on {inp.name}: {len(got)} edges, oracle {len(inp.ref)}")

    def collect_pending(self):
        inp, buf = self.pending
        cnt = self.e.join_wait()
        self.pending = None
        self.expect_edges(_got(buf, cnt), inp, "join_launch / join_wait")

    def build(self, inp, key_bits=0):
        self.log.append(f"build {inp.name} key_bits={key_bits}")
        inp.build(self.e, key_bits=key_bits)
        self.cur = inp
        self.check_stats(inp)

    def op(self, i):
        rng = self.rng
        r = rng.random()
        e = self.e
        if self.cur is None or r < 0.30:
            inp = self.pick(i)
            kb = 0
            if inp.kind == "sk" and inp.width:
                kb = int(rng.choice([0, inp.width, min(64, inp.width + 1), 64]))
            if self.pending is not None:          # a build queued behind the launched join, then the join collected
                self.build(inp, kb)
                self.log.append("join_wait")
                self.collect_pending()
            else:
                self.build(inp, kb)
        elif r < 0.40:
            self.log.append(f"join {self.cur.name}")
            if self.pending is not None:
                self.log.append("join_wait")
                self.collect_pending()
            got = _full_join(e, self.cur, self.buf)
            self.expect_edges(got, self.cur, "join")
            self.check(e.stats()["last_edges"] == len(self.cur.ref), "last_edges")
        elif r < 0.50:
            if self.pending is not None:
                self.log.append("join_wait")
                self.collect_pending()
            T = e.num_tiles
            cuts = sorted(set([0, T] + [int(x) for x in rng.integers(0, T + 1, size=int(rng.integers(1, 5)))]))
            self.log.append(f"join in pieces {cuts} of {self.cur.name}")
            parts = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                cnt = e.join(a, b, self.buf.ptr.value, CAP)
                parts.append(self.buf.to_numpy(engine.EDGE_DTYPE, cnt))
            got = _canon(np.concatenate(parts)) if parts else np.zeros(0, engine.EDGE_DTYPE)
            self.expect_edges(got, self.cur, "union of the pieces")
        elif r < 0.62:
            if self.pending is not None:
                self.log.append("join_wait")
                self.collect_pending()
            self.log.append(f"join_launch {self.cur.name}")
            e.join_launch(0, e.num_tiles, self.buf2.ptr.value, CAP)
            self.pending = (self.cur, self.buf2)
        elif r < 0.72:
            inp = self.pick(i)
            while inp.kind != "sk":
                inp = self.pick(i)
            self.log.append(f"step_launch {inp.name}")
            prev = self.pending
            buf = self.buf if prev is None or prev[1] is self.buf2 else self.buf2
            t0, t1, bound, launched, prev_cnt = e.step_launch(inp.d_keys.ptr.value, inp.offsets, 0, 1, buf.ptr.value, CAP,
                                                              d_weights_ptr=inp.d_weights)
            if prev is not None:
                self.expect_edges(_got(prev[1], prev_cnt), prev[0], "step_launch's collected join")
            self.check(launched and t0 == 0 and t1 == e.num_tiles and bound <= CAP, f"step {t0, t1, bound, launched}")
            self.cur = inp
            self.pending = (inp, buf)
            self.check_stats(inp)
        elif r < 0.78:
            if self.pending is not None:
                self.log.append("join_wait")
                self.collect_pending()
            self.log.append(f"join_to_host {self.cur.name}")
            n = len(self.cur.ref)
            host = np.zeros(max(1, n), dtype=engine.EDGE_DTYPE)
            cnt = e.join_to_host(0, e.num_tiles, host.ctypes.data, n)
            self.expect_edges(_canon(host[:cnt]), self.cur, "join_to_host")
        elif r < 0.86:
            env = MODES[int(rng.integers(len(MODES)))]
            self.log.append(f"mode {env}")
            self.mode = env
            for k in ENV_KNOBS:
                self.mp.delenv(k, raising=False)
            for k, v in env.items():
                self.mp.setenv(k, v)
        else:
            self.refused()

    def refused(self):
        """A call the engine must refuse, then the last good build (and a pending join) checked."""
        rng, e, cur = self.rng, self.e, self.cur
        kinds = ["monotone", "first", "limit", "key_bits", "part", "post_src", "join_cap", "host_cap", "step_cap", "launch_cap"]
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind in ("post_src", "join_cap", "host_cap", "step_cap", "launch_cap") and self.pending is not None:
            self.log.append("join_wait")
            self.collect_pending()
        self.log.append(f"refused {kind}")
        dk = self.pool["n700"].d_keys.ptr.value
        want = engine.KSP_E_ARG
        with pytest.raises(engine.KspError) as ei:
            if kind == "monotone":
                e.build_blocks(dk, np.array([0, 5, 3, 9], dtype=np.uint64))
            elif kind == "first":
                e.build_blocks(dk, np.array([2, 5, 9], dtype=np.uint64))
            elif kind == "limit":
                want = engine.KSP_E_LIMIT
                e.build_blocks(dk, np.array([0, 1 << 29, 1 << 30], dtype=np.uint64))
            elif kind == "key_bits":
                e.build_blocks(dk, np.array([0, 3, 9], dtype=np.uint64), key_bits=int(rng.choice([65, 200, -1])))
            elif kind == "part":
                e.build_slice(dk, np.array([0, 3, 9], dtype=np.uint64), 2, 2)
            elif kind == "post_src":
                bad = engine.DeviceBuffer.from_numpy(np.array([0, 1, 2, 7], dtype=np.uint32))
                try:
                    e.build_postings(np.array([0, 2, 4], dtype=np.uint64), bad.ptr.value, 0, 5)
                finally:
                    bad.free()
            elif kind in ("join_cap", "host_cap", "launch_cap", "step_cap"):
                want = engine.KSP_E_OVERFLOW
                if len(cur.ref) == 0 and kind != "step_cap":
                    raise engine.KspError(want, "(nothing to overflow: skipped)")
                if kind == "join_cap":
                    e.join(0, e.num_tiles, self.buf.ptr.value, len(cur.ref) - 1)
                elif kind == "host_cap":
                    host = np.zeros(len(cur.ref), dtype=engine.EDGE_DTYPE)
                    e.join_to_host(0, e.num_tiles, host.ctypes.data, len(cur.ref) - 1)
                elif kind == "launch_cap":
                    e.join_launch(0, e.num_tiles, self.buf.ptr.value, len(cur.ref) - 1)
                    e.join_wait()
                else:
                    if cur.kind != "sk":
                        raise engine.KspError(want, "(postings: no step_launch)")
                    t0, t1, bound, launched, _ = e.step_launch(cur.d_keys.ptr.value, cur.offsets, 0, 1, self.buf.ptr.value, 0,
                                                               d_weights_ptr=cur.d_weights)
                    self.check(not launched, "step_launch launched into a buffer below the bound")
                    raise engine.KspError(want, "(not launched)")
        self.check(ei.value.code == want, f"refused {kind}: code {ei.value.code}, want {want}")
        if kind == "post_src":
            self.cur = None        # (a postings build refuses this only after it has run: nothing to keep)
            return
        if self.pending is not None:   # the refused build left the launched join collectable ...
            self.log.append("join_wait")
            self.collect_pending()
        self.log.append(f"join {cur.name} (after the refusal)")
        self.expect_edges(_full_join(e, cur, self.buf), cur, "join after a refused call")   # ... and the last build joinable

    def close(self):
        if self.pending is not None:
            self.log.append("join_wait")
            self.collect_pending()
        self.e.close()
        self.buf2.free()


@pytest.mark.parametrize("seed", range(10))
def test_call_sequences_on_one_engine(pool, edges_buf, monkeypatch, seed):
    r = Runner(seed, pool, edges_buf, monkeypatch)
    for i in range(30):
        r.op(i)
    r.close()


def test_slice_calls_without_a_slice_build_are_refused(pool, edges_buf):
    """slice_labels / slice_bounds / slice_set_bounds / slice_finish on a fresh engine and after a whole build: KSP_E_ARG,
    and the whole build stays joinable."""
    inp = pool["n700"]
    buf = engine.DeviceBuffer(max(4, inp.n_sources * 4))
    e = engine.Engine(0)
    try:
        for built in (False, True):
            if built:
                inp.build(e)
            for call in (e.slice_labels, e.slice_bounds, e.slice_set_bounds, e.slice_finish):
                with pytest.raises(engine.KspError) as ei:
                    call(buf.ptr.value)
                assert ei.value.code == engine.KSP_E_ARG and "build_slice has not been run" in str(ei.value), call
        assert _same(_full_join(e, inp, edges_buf), inp.ref)
    finally:
        buf.free()
        e.close()


# ---- refused calls, one by one (C1 / C2 of the engine's contract) --------------------------------------------------

@pytest.mark.parametrize("kind", ["monotone", "first", "limit", "key_bits", "part"])
def test_refused_build_keeps_the_last_build_and_the_pending_join(pool, edges_buf, kind):
    """Every argument of a build is checked before the engine changes: after the refusal the pending join is still
    collected with its own count, and the last build is still joinable."""
    inp = pool["n700"]
    e = engine.Engine(0)
    inp.build(e)
    pend = engine.DeviceBuffer(CAP * 16)
    e.join_launch(0, e.num_tiles, pend.ptr.value, CAP)
    dk = inp.d_keys.ptr.value
    with pytest.raises(engine.KspError) as ei:
        if kind == "monotone":
            e.build_blocks(dk, np.array([0, 5, 3, 9], dtype=np.uint64))
        elif kind == "first":
            e.build_blocks(dk, np.array([2, 5, 9], dtype=np.uint64))
        elif kind == "limit":
            e.build_blocks(dk, np.array([0, 1 << 30], dtype=np.uint64))
        elif kind == "key_bits":
            e.build_blocks(dk, inp.offsets, key_bits=65)
        else:
            e.build_slice(dk, inp.offsets, 1, 1)
    assert ei.value.code == (engine.KSP_E_LIMIT if kind == "limit" else engine.KSP_E_ARG)
    cnt = e.join_wait()
    assert _same(_got(pend, cnt), inp.ref)
    assert _same(_full_join(e, inp, edges_buf), inp.ref)
    st = e.stats()
    assert st["n_sources"] == inp.n_sources and st["n_entries"] == inp.n_entries and st["last_edges"] == len(inp.ref)
    pend.free()
    e.close()


def test_refused_postings_build_keeps_the_last_build(pool, edges_buf):
    inp = pool["n129"]
    e = engine.Engine(0)
    inp.build(e)
    dsrc = engine.DeviceBuffer.from_numpy(np.array([0, 1, 2, 3], dtype=np.uint32))
    with pytest.raises(engine.KspError) as ei:
        e.build_postings(np.array([0, 1, 4], dtype=np.uint64), dsrc.ptr.value, 0, 8)   # a key with one holder
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        e.build_postings(np.array([0, 2, 1 << 30], dtype=np.uint64), dsrc.ptr.value, 0, 8)
    assert ei.value.code == engine.KSP_E_LIMIT
    assert _same(_full_join(e, inp, edges_buf), inp.ref)
    dsrc.free()
    e.close()


@pytest.mark.parametrize("second", ["join_launch", "join", "join_to_host"])
def test_second_join_while_one_is_pending_is_refused(pool, edges_buf, second):
    """One launched join per engine: a second one is refused (KSP_E_ARG) and the first keeps its count."""
    inp = pool["n700"]
    e = engine.Engine(0)
    inp.build(e)
    pend = engine.DeviceBuffer(CAP * 16)
    e.join_launch(0, e.num_tiles, pend.ptr.value, CAP)
    with pytest.raises(engine.KspError) as ei:
        if second == "join_launch":
            e.join_launch(0, e.num_tiles, edges_buf.ptr.value, CAP)
        elif second == "join":
            e.join(0, e.num_tiles, edges_buf.ptr.value, CAP)
        else:
            host = np.zeros(len(inp.ref), dtype=engine.EDGE_DTYPE)
            e.join_to_host(0, e.num_tiles, host.ctypes.data, host.size)
    assert ei.value.code == engine.KSP_E_ARG
    cnt = e.join_wait()
    assert cnt == len(inp.ref) and _same(_got(pend, cnt), inp.ref)
    assert e.stats()["last_edges"] == len(inp.ref)
    assert _same(_full_join(e, inp, edges_buf), inp.ref)      # and once collected, the next join goes ahead
    pend.free()
    e.close()


@pytest.mark.parametrize("late", [False, True])
def test_step_launch_on_the_full_sort_retry(pool, monkeypatch, late):
    """Keys sharing their top 32 bits make the first attempt of a build overflow its prefix sort; the second attempt
    sorts on all bits (sort_bits = the key width).  With step_launch's early work list the first attempt has staged its
    block tables already: the second must stage its own.  KSP_DEBUG_LATE_SCHED=1: the work list after the build."""
    if late:
        monkeypatch.setenv("KSP_DEBUG_LATE_SCHED", "1")
    x, y = pool["top32"], pool["n700"]
    e = engine.Engine(0)
    bufs = [engine.DeviceBuffer(CAP * 16), engine.DeviceBuffer(CAP * 16)]
    seq = [x, y, x, x, y]
    prev = None
    for i, inp in enumerate(seq):
        buf = bufs[i % 2]
        t0, t1, bound, launched, cnt = e.step_launch(inp.d_keys.ptr.value, inp.offsets, 0, 1, buf.ptr.value, CAP)
        assert launched
        st = e.stats()
        if i == 0:
            assert st["sort_bits"] == st["key_bits"] == x.width == 60, st      # attempt 2 ran: the full-width sort
        if prev is not None:
            assert _same(_got(bufs[(i - 1) % 2], cnt), prev.ref), (i, prev.name)
        prev = inp
    cnt = e.join_wait()
    assert _same(_got(bufs[(len(seq) - 1) % 2], cnt), prev.ref)
    for b in bufs:
        b.free()
    e.close()


# ---- B: sticky fall-backs and the order of inputs ------------------------------------------------------------------

def _run(pool, buf, names):
    """Build and join the named inputs in turn on one engine: [(edges equal the oracle's, stats)]."""
    e = engine.Engine(0)
    out = []
    for name in names:
        inp = pool[name]
        inp.build(e)
        st = e.stats()
        out.append((_same(_full_join(e, inp, buf), inp.ref), st))
    e.close()
    return out


def _path(st):
    return {k: st[k] for k in ("partition_kind", "partition_fallback", "sort_bits", "key_bits", "stage1_kind")}


STICKY = {   # fall-back input X -> (environment, what X's own build shows)
    "top32": {},
    "skewed": {"KSP_PART_MIN": "1"},
    "holders": {},
    "sparse": {"KSP_FUSED": "1"},
}


@pytest.mark.parametrize("x", sorted(STICKY))
def test_fallback_input_then_an_ordinary_one(pool, edges_buf, monkeypatch, x):
    """Y fresh, X then Y, Y X Y: every build gives the oracle's edges; the stats show the fall-back X left behind."""
    for k, v in STICKY[x].items():
        monkeypatch.setenv(k, v)
    y = "n700"
    fresh = _run(pool, edges_buf, [y])
    xy = _run(pool, edges_buf, [x, y])
    yxy = _run(pool, edges_buf, [y, x, y])
    runs = {"Y": fresh, "XY": xy, "YXY": yxy}
    for tag, res in runs.items():
        print(f"PATH {x} {tag}: " + " | ".join(str(_path(st)) for _, st in res))
        assert all(ok for ok, _ in res), (x, tag, [_path(st) for _, st in res])
    y0, x1, y1 = fresh[0][1], xy[0][1], xy[1][1]
    assert _path(yxy[0][1]) == _path(y0)              # (the first Y of Y X Y is a fresh Y)
    assert _path(yxy[2][1]) == _path(y1)              # Y after X: the same path, whatever came before X
    assert y0["partition_fallback"] == 0 and y1["partition_fallback"] == 0   # it describes the last build only
    if x == "top32":
        assert x1["sort_bits"] == x1["key_bits"] == 60                       # full-width sort (second attempt)
        assert 0 < y0["sort_bits"] <= 16                                     # Y alone: partitioned
        assert y1["sort_bits"] == y1["key_bits"] and y1["partition_kind"] == 1   # after X: full sort, library sort
    elif x == "skewed":
        assert x1["partition_kind"] == 1 and x1["partition_fallback"] == 1   # page tables full -> library partition
        assert y0["partition_kind"] in (2, 3)
        assert y1["partition_kind"] == 1                                     # the engine keeps the library partition
    elif x == "holders":
        assert _path(y1) == _path(y0)                                        # nothing sticks
    elif x == "sparse":
        assert y0["stage1_kind"] == 1                                        # Y alone: bucket-resident
        assert x1["stage1_kind"] == 0                                        # the bucket-resident build gave up
        assert y1["stage1_kind"] == 0                                        # ... and stays off on this engine


@pytest.mark.parametrize("env", [{"KSP_SEG": "1", "KSP_PART_MIN": "1"}, {"KSP_SEG": "0", "KSP_PART_MIN": "1"},
                                 {"KSP_FUSED": "1"}, {}])
def test_same_offsets_other_keys(pool, edges_buf, monkeypatch, env):
    """A set and its twin (the same offsets, other keys) in turn: the engine keeps the offsets (and the segment
    partition's tables) but must read the new keys."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, b = pool["n700"], pool["twin700"]
    assert (a.offsets == b.offsets).all() and len(a.ref) != len(b.ref)
    e = engine.Engine(0)
    for inp in (a, b, a, b, b, a):
        inp.build(e)
        assert _same(_full_join(e, inp, edges_buf), inp.ref), (env, inp.name)
    e.close()


# ---- D: streams ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def streams():
    """Two non-blocking HIP streams, made by the HIP runtime the library itself runs on."""
    engine.lib()
    hip = ctypes.CDLL("libamdhip64.so.7")
    out = []
    for _ in range(2):
        s = ctypes.c_void_p()
        assert hip.hipSetDevice(0) == 0 and hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0   # hipStreamNonBlocking
        out.append(s.value)
    yield out
    for s in out:
        hip.hipStreamDestroy(ctypes.c_void_p(s))


def test_every_entry_on_a_stream_of_its_own(pool, edges_buf, streams):
    s = streams[0]
    e = engine.Engine(0)
    for name in ("n700", "weighted", "n129", "n3000"):
        inp = pool[name]
        inp.build(e, stream=s)
        assert _same(_full_join(e, inp, edges_buf, stream=s), inp.ref), name
        e.join_launch(0, e.num_tiles, edges_buf.ptr.value, CAP, stream=s)
        assert _same(_got(edges_buf, e.join_wait()), inp.ref), name
        host = np.zeros(max(1, len(inp.ref)), dtype=engine.EDGE_DTYPE)
        cnt = e.join_to_host(0, e.num_tiles, host.ctypes.data, len(inp.ref), stream=s)
        assert _same(_canon(host[:cnt]), inp.ref), name
    p = pool["post700w"]
    p.build(e, stream=s)
    assert _same(_full_join(e, p, edges_buf, stream=s), p.ref)
    # a step_launch chain on the stream, weighted steps included
    bufs = [engine.DeviceBuffer(CAP * 16), engine.DeviceBuffer(CAP * 16)]
    seq = [pool[n] for n in ("n700", "weighted", "n128", "weighted_low20", "n700")]
    prev = None
    for i, inp in enumerate(seq):
        t0, t1, bound, launched, cnt = e.step_launch(inp.d_keys.ptr.value, inp.offsets, 0, 1, bufs[i % 2].ptr.value, CAP,
                                                     stream=s, d_weights_ptr=inp.d_weights, key_bits=inp.width)
        assert launched
        assert e.stats()["weighted"] == int(inp.weighted)
        if prev is not None:
            assert _same(_got(bufs[(i - 1) % 2], cnt), prev.ref), prev.name
        prev = inp
    assert _same(_got(bufs[(len(seq) - 1) % 2], e.join_wait()), prev.ref)
    for b in bufs:
        b.free()
    e.close()


def test_two_engines_interleaved_on_two_streams(pool, streams):
    s1, s2 = streams
    e1, e2 = engine.Engine(0), engine.Engine(0)
    b1, b2 = engine.DeviceBuffer(CAP * 16), engine.DeviceBuffer(CAP * 16)
    plan = [("n700", "weighted"), ("n3000", "n129"), ("twin700", "n700"), ("low20", "full64")]
    for a, b in plan:
        pa, pb = pool[a], pool[b]
        pa.build(e1, stream=s1)
        pb.build(e2, stream=s2)
        e1.join_launch(0, e1.num_tiles, b1.ptr.value, CAP, stream=s1)
        e2.join_launch(0, e2.num_tiles, b2.ptr.value, CAP, stream=s2)
        c2 = e2.join_wait()
        c1 = e1.join_wait()
        assert _same(_got(b1, c1), pa.ref), a
        assert _same(_got(b2, c2), pb.ref), b
    for x in (b1, b2):
        x.free()
    e1.close()
    e2.close()


def test_build_on_another_stream_than_a_pending_join_is_refused(pool, edges_buf, streams):
    """Nothing orders two streams: a build on stream B while a join is pending on stream A could overwrite the lists the
    join reads.  The engine refuses it (nothing changes); once the join is collected, the build goes ahead."""
    s1, s2 = streams
    a, b = pool["n700"], pool["n3000"]
    e = engine.Engine(0)
    a.build(e, stream=s1)
    pend = engine.DeviceBuffer(CAP * 16)
    e.join_launch(0, e.num_tiles, pend.ptr.value, CAP, stream=s1)
    with pytest.raises(engine.KspError) as ei:
        b.build(e, stream=s2)
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        e.step_launch(b.d_keys.ptr.value, b.offsets, 0, 1, edges_buf.ptr.value, CAP, stream=s2)
    assert ei.value.code == engine.KSP_E_ARG
    assert _same(_got(pend, e.join_wait()), a.ref)
    b.build(e, stream=s2)
    assert _same(_full_join(e, b, edges_buf, stream=s2), b.ref)
    pend.free()
    e.close()


# ---- E: sliced builds inside call sequences --------------------------------------------------------------------------
# (what tests/test_slices*_gpu.py leave out: they run the slice protocol in its documented order on a fresh engine)

SLICE_CALLS = ("slice_labels", "slice_bounds", "slice_set_bounds", "slice_finish")
REFUSED_BUILDS = ("monotone", "first", "limit", "key_bits", "part")


def _key_count_cuts(inp, nparts):
    n_keys = inp.key_off.size - 1
    return [n_keys * s // nparts for s in range(nparts + 1)]


def _slice_build(inp, nparts):
    """build(e, p) of the slice driver for a pool input: sketches by key range, postings by key count."""
    if inp.kind == "post":
        return postings_slice_build(inp.key_off, inp.d_srcbuf.ptr.value, inp.d_weights, inp.n_sources, _key_count_cuts(inp, nparts))
    return sketch_slice_build(inp.d_keys.ptr.value, inp.offsets, nparts, inp.d_weights)


def _protocol(e, inp, nparts, sum_bounds=None, hook=None):
    sum_bounds = inp.kind == "post" if sum_bounds is None else sum_bounds
    return Protocol(e, inp.n_sources, nparts, _slice_build(inp, nparts), sum_bounds=sum_bounds, hook=hook)


def _sliced(e, inp, nparts, sum_bounds=None, stop=None):
    """The slice driver on engine e: the edges (None when stopped)."""
    sum_bounds = inp.kind == "post" if sum_bounds is None else sum_bounds
    return slice_run(inp.n_sources, nparts, _slice_build(inp, nparts), sum_bounds=sum_bounds, engine_=e, stop=stop)[0]


def _refusal(call, stem=None, code=None):
    """call() raises KspError `code` (KSP_E_ARG) whose message holds `stem`."""
    with pytest.raises(engine.KspError) as ei:
        call()
    assert ei.value.code == (engine.KSP_E_ARG if code is None else code), (ei.value.code, str(ei.value))
    if stem is not None:
        assert stem in str(ei.value), str(ei.value)


def _no_slice_at_labels(e, scratch):
    for name in SLICE_CALLS:
        _refusal(lambda: getattr(e, name)(scratch.ptr.value), "build_slice has not been run")


def _no_finished_slice(e, scratch):
    p = scratch.ptr.value
    _refusal(e.slice_sizes)
    _refusal(lambda: e.slice_export(p, p, p, p, p, p))
    _refusal(lambda: e.assemble(np.zeros(4, dtype=np.uint64), p, p, p, 1, p, p, p, 1))


def _not_joinable(e, buf):
    T = e.num_tiles
    host = np.zeros(4, dtype=engine.EDGE_DTYPE)
    _refusal(lambda: e.join(0, T, buf.ptr.value, CAP), "build_blocks has not been run")
    _refusal(lambda: e.join_launch(0, T, buf.ptr.value, CAP), "build_blocks has not been run")
    _refusal(lambda: e.join_to_host(0, T, host.ctypes.data, host.size), "build_blocks has not been run")
    _refusal(lambda: e.balanced_cuts(2), "has not been run")
    assert e.edge_bound(0, T) == 0 and e.lists_path() == 0


def _refused_build(e, kind, dk):
    """One build that the engine refuses on its arguments (the kinds of Runner.refused that change nothing)."""
    small = np.array([0, 3, 9], dtype=np.uint64)
    if kind == "monotone":
        _refusal(lambda: e.build_blocks(dk, np.array([0, 5, 3, 9], dtype=np.uint64)))
    elif kind == "first":
        _refusal(lambda: e.build_blocks(dk, np.array([2, 5, 9], dtype=np.uint64)))
    elif kind == "limit":
        _refusal(lambda: e.build_blocks(dk, np.array([0, 1 << 29, 1 << 30], dtype=np.uint64)), code=engine.KSP_E_LIMIT)
    elif kind == "key_bits":
        _refusal(lambda: e.build_blocks(dk, small, key_bits=65))
    else:
        _refusal(lambda: e.build_slice(dk, small, 2, 2))


@pytest.fixture(scope="module")
def scratch(pool):
    """4 bytes per source of the largest pool input: what the slice calls copy labels and bounds into."""
    return engine.DeviceBuffer(4 * max(inp.n_sources for inp in pool.values()) + 64)


@pytest.mark.parametrize("whole", ["build_blocks", "step_launch", "build_postings"])
@pytest.mark.parametrize("abandoned", ["build", "labels", "set_bounds"])
@pytest.mark.parametrize("start", ["build_slice", "build_postings_slice"])
def test_whole_build_forgets_an_unfinished_slice(pool, edges_buf, scratch, start, abandoned, whole):
    """A slice left after its build, after slice_labels or after slice_bounds + slice_set_bounds, then a whole build of a
    smaller input: the slice is forgotten (no slice call is accepted: slice_finish would run the second half of a slice
    build over a whole build's state), and the whole build is all the engine knows."""
    sl = pool["n700" if start == "build_slice" else "post700w"]
    inp = pool[{"build_blocks": "n129", "step_launch": "n127", "build_postings": "post700"}[whole]]
    e = engine.Engine(0)
    try:
        _slice_build(sl, 2)(e, 1)
        if abandoned != "build":
            e.slice_labels(scratch.ptr.value)
        if abandoned == "set_bounds":
            e.slice_bounds(scratch.ptr.value)
            e.slice_set_bounds(scratch.ptr.value)
        if whole == "step_launch":
            t0, t1, bound, launched, prev = e.step_launch(inp.d_keys.ptr.value, inp.offsets, 0, 1, edges_buf.ptr.value, CAP)
            assert launched and (t0, t1) == (0, e.num_tiles) and prev is None
        else:
            inp.build(e)
        _no_slice_at_labels(e, scratch)
        _no_finished_slice(e, scratch)
        st = e.stats()
        assert st["n_sources"] == inp.n_sources and st["n_entries"] == inp.n_entries and st["weighted"] == 0, st
        if whole == "step_launch":      # the refused calls left the launched join alone
            cnt = e.join_wait()
            assert cnt == len(inp.ref) and _same(_got(edges_buf, cnt), inp.ref)
        assert _same(_full_join(e, inp, edges_buf), inp.ref)
    finally:
        e.close()


@pytest.mark.parametrize("kind", REFUSED_BUILDS)
@pytest.mark.parametrize("name", ["weighted_low20", "post700"])
def test_refused_build_inside_a_slice_protocol_changes_nothing(pool, scratch, name, kind):
    """A refused build behind every slice build (so between build_slice and slice_labels, and between build_slice and
    slice_finish) and behind every slice_finish and export (between slice_finish and assemble): the protocol goes on."""
    inp = pool[name]
    dk = pool["n700"].d_keys.ptr.value
    e = engine.Engine(0)
    seen = []

    def hook(where, p):
        seen.append(where)
        _refused_build(e, kind, dk)

    pr = _protocol(e, inp, 3, hook=hook)
    try:
        assert not pr.first_pass() and not pr.second_pass()
        pr.stack()
        _refused_build(e, kind, dk)
        pr.assemble()
        assert _same(pr.join(), inp.ref)
        assert seen == ["built"] * 3 + ["rebuilt", "finished", "exported"] * 3
    finally:
        pr.free()
        e.close()


@pytest.mark.parametrize("first", ["n700", "twin700"])
@pytest.mark.parametrize("stage", ["finish", "assemble"])
def test_whole_build_after_a_finished_slice_and_after_an_assemble(pool, edges_buf, scratch, stage, first):
    """n700 and twin700 have the same offsets and other keys: after the slices of one, the whole build of the other gives
    its own edges (the engine keeps the offsets, not the slices' lists), and nothing of the slice protocol is accepted."""
    a = pool[first]
    b = pool["twin700" if first == "n700" else "n700"]
    e = engine.Engine(0)
    try:
        assert _sliced(e, a, 2, stop=stage) is None
        b.build(e)
        _no_slice_at_labels(e, scratch)
        _no_finished_slice(e, scratch)
        assert _same(_full_join(e, b, edges_buf), b.ref)
        assert _same(_sliced(e, a, 3), a.ref)      # ... and the slices again behind the whole build
    finally:
        e.close()


@pytest.mark.parametrize("name", ["n129", "post700w"])
def test_not_joinable_until_assembled(pool, edges_buf, scratch, name):
    """A slice build on a joinable engine: nothing joins until the assemble, and the join launched on the whole build
    before it (the same stream) is collected behind it with the whole build's count and edges."""
    big, inp = pool["n3000"], pool[name]
    e = engine.Engine(0)
    pend = engine.DeviceBuffer(CAP * 16)
    where = []

    def hook(at, p):
        if at in ("built", "finished"):
            _not_joinable(e, edges_buf)
        if not where:      # (after the first slice build)
            cnt = e.join_wait()
            assert cnt == len(big.ref) and _same(_got(pend, cnt), big.ref)
            assert e.stats()["last_edges"] == len(big.ref)
        where.append(at)

    pr = _protocol(e, inp, 2, hook=hook)
    try:
        big.build(e)
        e.join_launch(0, e.num_tiles, pend.ptr.value, CAP)
        assert not pr.first_pass() and not pr.second_pass()
        pr.stack()
        _not_joinable(e, edges_buf)
        pr.assemble()
        assert _same(pr.join(), inp.ref)
        assert e.balanced_cuts(2)[-1] == e.num_tiles
    finally:
        pr.free()
        pend.free()
        e.close()


@pytest.mark.parametrize("name", ["n127", "weighted_low20", "post700"])
def test_slice_calls_out_of_order(pool, edges_buf, scratch, name):
    """slice_finish twice; slice_sizes / slice_export of a slice that is built and not finished; assemble twice."""
    inp = pool[name]
    e = engine.Engine(0)

    def hook(at, p):
        if at in ("built", "rebuilt"):      # the slice before this one was finished: its sizes went with the build
            _refusal(e.slice_sizes, "build_slice has not been run")
            q = scratch.ptr.value
            _refusal(lambda: e.slice_export(q, q, q, q, q, q), "build_slice has not been run")
        if at == "finished":
            _refusal(lambda: e.slice_finish(pr.lab.ptr.value), "build_slice has not been run")

    pr = _protocol(e, inp, 3, hook=hook)
    try:
        assert not pr.first_pass() and not pr.second_pass()
        pr.stack()
        pr.assemble()
        first = e.stats()["n_block_keys"]
        assert _same(_full_join(e, inp, edges_buf), inp.ref)
        pr.assemble()
        assert e.stats()["n_block_keys"] == first
        assert _same(_full_join(e, inp, edges_buf), inp.ref)
    finally:
        pr.free()
        e.close()


# ---- F: slices inside the seeded sequences ---------------------------------------------------------------------------

SLICE_POOL = ["n129", "n127", "one", "empty", "n700", "n3000", "weighted_low20", "post700", "post700w"]


class SliceRunner(Runner):
    """Runner's operations and two more: a pool input built in slices on this engine, and a slice protocol left at a
    random point.  Slices run under the modes of test_random_sketches_in_slices_all_modes; weights and postings under
    the weighted ones."""

    def op(self, i):
        r = self.rng.random()
        if r < 0.16:
            self.sliced(i, None)
        elif r < 0.26:
            self.sliced(i, STOPS[int(self.rng.integers(len(STOPS) - 1))])      # (any stop before the assemble)
        else:
            super().op(i)

    def pick_sliced(self):
        rng = self.rng
        if self.mode not in SLICE_MODES:
            self.mode = SLICE_MODES[int(rng.integers(len(SLICE_MODES)))]
            self.log.append(f"mode {self.mode} (for slices)")
            for k in ENV_KNOBS:
                self.mp.delenv(k, raising=False)
            for k, v in self.mode.items():
                self.mp.setenv(k, v)
        names = SLICE_POOL
        if self.mode not in WEIGHTED_MODES:
            names = [n for n in names if not self.pool[n].weighted and self.pool[n].kind == "sk"]
        inp = self.pool[names[int(rng.integers(len(names)))]]
        sum_bounds = inp.kind == "post" and bool(rng.integers(2))
        return inp, int(rng.integers(1, 4)), sum_bounds

    def sliced(self, i, stop):
        inp, nparts, sum_bounds = self.pick_sliced()
        behind = self.pending is not None and bool(self.rng.integers(2))
        if self.pending is not None and not behind:
            self.log.append("join_wait")
            self.collect_pending()
        self.log.append(f"slices of {inp.name}: {nparts}, summed bounds {sum_bounds}, " + (f"left at {stop}" if stop else "assembled"))
        _sliced(self.e, inp, nparts, sum_bounds=sum_bounds, stop=stop or "assemble")
        if behind:      # the join launched before the slices ran in front of them on the stream
            self.log.append("join_wait")
            self.collect_pending()
        if stop:
            self.cur = None
            return
        self.cur = inp
        st = self.e.stats()
        self.check(st["n_sources"] == inp.n_sources and st["weighted"] == int(inp.weighted), f"stats {st}")
        if inp.kind == "sk":      # (a slice of postings reports its own entries)
            self.check(st["n_entries"] == inp.n_entries, f"stats {st}")
        self.expect_edges(_full_join(self.e, inp, self.buf), inp, "join of the assembled slices")


@pytest.mark.parametrize("seed", range(10))
def test_call_sequences_with_slices_on_one_engine(pool, edges_buf, monkeypatch, seed):
    r = SliceRunner(seed, pool, edges_buf, monkeypatch)
    for i in range(30):
        r.op(i)
    r.close()


# ---- G: seeded walks over the state table (tests/engine_states.py) -----------------------------------

@functools.lru_cache(maxsize=None)
def _walk_inputs():
    import oracle
    pool = _pool_cached()
    out = {n: pool[n] for n in ES.SKETCH_INPUTS}
    s = pool["n129"]
    _, ko, hs = _postings(s.keys, s.offsets)
    kw = np.random.default_rng(129).integers(1, 1001, size=ko.size - 1, dtype=np.uint32)
    out["post129"] = Input("post129", oracle, postings=(ko, hs, None), n_sources=s.n_sources)
    out["post129w"] = Input("post129w", oracle, postings=(ko, hs, kw), n_sources=s.n_sources)
    return out


@functools.lru_cache(maxsize=None)
def _slices_of(name, nparts):
    """The slices of a walk input as another rank would hand them over: made once on an engine of their own and kept on
    the device (combined labels, the bounds to set, the stacked exports)."""
    inp = _walk_inputs()[name]
    e = engine.Engine(0)
    pr = _protocol(e, inp, nparts)
    assert not pr.first_pass() and not pr.second_pass()
    pr.stack()
    if pr.bnd is None:      # sketches: a slice reports every source's whole bound
        pr.build(e, 0)
        pr.bnd = engine.DeviceBuffer(max(4, inp.n_sources * 4))
        e.slice_bounds(pr.bnd.ptr.value)
    e.close()
    pr.e = None
    pr.inp = inp
    return pr


class Walker:
    """One walk of engine_states.walk on one engine: a refused cell raises its code and message and leaves the stats
    alone; an accepted one is made with valid arguments; joins are compared with the oracle."""

    def __init__(self, seed, buf, scratch):
        self.seed, self.buf, self.scratch = seed, buf, scratch
        self.inputs = _walk_inputs()
        self.e = engine.Engine(0)
        self.buf2 = engine.DeviceBuffer(CAP * 16)
        self.pend_buf = None
        self.ctx = self.part = None
        self.bounds_set = False
        self.log = []

    def check(self, cond, msg):
        lines = "\n".join(f"  {i:3d}: {s}" for i, s in enumerate(self.log))
        assert cond, f"seed {self.seed}, step {len(self.log) - 1}: {msg}\nsteps:\n{lines}"

    def edges(self, got, name, what):
        ref = self.inputs[name].ref
        self.check(_same(got, ref), f"{what} of {name}: {len(got)} edges, oracle {len(ref)}")

    def args(self, call):
        """A refused call: arguments that pass the NULL checks, so the refusal is the state's."""
        e, q, T = self.e, self.scratch.ptr.value, self.e.num_tiles
        small = self.inputs["n127"]
        host = np.zeros(4, dtype=engine.EDGE_DTYPE)
        return {"slice_labels": lambda: e.slice_labels(q), "slice_bounds": lambda: e.slice_bounds(q),
                "slice_set_bounds": lambda: e.slice_set_bounds(q), "slice_finish": lambda: e.slice_finish(q),
                "slice_sizes": e.slice_sizes, "slice_export": lambda: e.slice_export(q, q, q, q, q, q),
                "assemble": lambda: e.assemble(np.zeros(4, dtype=np.uint64), q, q, q, 1, q, q, q, 1),
                "join": lambda: e.join(0, T, self.buf.ptr.value, CAP),
                "join_launch": lambda: e.join_launch(0, T, self.buf.ptr.value, CAP),
                "join_to_host": lambda: e.join_to_host(0, T, host.ctypes.data, host.size),
                "balanced_cuts": lambda: e.balanced_cuts(2)}[call]

    def step(self, s):
        e, call, cell = self.e, s.call, s.cell
        self.log.append(f"{s.state:9s} {'pending ' + s.pending if s.pending else '':16s} {call} "
                        f"{(s.inp, s.nparts, s.part) if s.inp else ''} -> {cell.kind}")
        if cell.kind == "refused":
            in_flight = getattr(e, "_join_in_flight", False)
            before = e.stats()
            with pytest.raises(engine.KspError) as ei:
                self.args(call)()
            e._join_in_flight = in_flight      # (the wrapper's own note of a launched join: the engine kept it)
            self.check(ei.value.code == getattr(engine, cell.code) and cell.stem in str(ei.value), f"refusal {ei.value}")
            after = e.stats()
            same = ("n_sources", "n_entries", "n_blocks", "weighted", "n_block_keys", "last_edges")
            self.check(all(before[k] == after[k] for k in same), f"a refused call changed the stats: {before} -> {after}")
            return
        inp = self.inputs[s.inp] if s.inp else None
        cur = self.inputs[s.cur] if s.cur else None
        T = e.num_tiles
        if call in ("build_blocks", "build_postings"):
            inp.build(e)
        elif call == "step_launch":
            buf = self.buf if self.pend_buf is self.buf2 else self.buf2
            t0, t1, bound, launched, prev = e.step_launch(inp.d_keys.ptr.value, inp.offsets, 0, 1, buf.ptr.value, CAP,
                                                          d_weights_ptr=inp.d_weights)
            self.check(launched and (t0, t1) == (0, e.num_tiles), f"step {t0, t1, bound, launched}")
            if s.pending:
                self.edges(_got(self.pend_buf, prev), s.pending, "step_launch's collected join")
            self.pend_buf = buf
        elif call in ES.SLICE_BUILDS:
            self.ctx, self.part, self.bounds_set = _slices_of(s.inp, s.nparts), s.part, False
            self.ctx.build(e, s.part)
        elif call == "slice_labels":
            e.slice_labels(self.scratch.ptr.value)
        elif call == "slice_bounds":
            e.slice_bounds(self.scratch.ptr.value)
        elif call == "slice_set_bounds":
            e.slice_set_bounds(self.ctx.bnd.ptr.value)
            self.bounds_set = True
        elif call == "slice_finish":
            if self.ctx.sum_bounds and not self.bounds_set:      # (every slice of an index under the same, summed bounds)
                e.slice_set_bounds(self.ctx.bnd.ptr.value)
            e.slice_finish(self.ctx.lab.ptr.value)
        elif call == "slice_sizes":
            sz = e.slice_sizes()
            want = self.ctx.sizes[4 * self.part:4 * self.part + 4]
            self.check((sz == want).all(), f"slice_sizes {sz.tolist()}, the same slice on another engine {want.tolist()}")
        elif call == "slice_export":
            sz = e.slice_sizes()
            L, nbig, nb = int(sz[0]), int(sz[2]), e.stats()["n_blocks"]
            bufs = [engine.DeviceBuffer(max(4, L * 4)) for _ in range(3)] + [engine.DeviceBuffer((nb + 1) * 4) for _ in range(2)]
            bufs.append(engine.DeviceBuffer(max(16, nbig * 16)))
            e.slice_export(*[b.ptr.value for b in bufs])
            raw = bufs[3].to_numpy(np.uint32, nb + 1)
            want = self.ctx.parts[self.part]["raw"].view(np.uint32)
            for b in bufs:
                b.free()
            if self.ctx.inp.n_entries:      # (nothing built: nothing is exported)
                self.check((raw == want).all(), "slice_export: other keys per block than the same slice on another engine")
        elif call == "assemble":
            self.ctx.assemble(e)
            st = e.stats()
            self.check(st["n_sources"] == self.ctx.inp.n_sources and st["weighted"] == int(self.ctx.inp.weighted), f"stats {st}")
        elif call == "join":
            self.edges(_full_join(e, cur, self.buf), s.cur, "join")
        elif call == "join_launch":
            e.join_launch(0, T, self.buf2.ptr.value, CAP)
            self.pend_buf = self.buf2
        elif call == "join_to_host":
            host = np.zeros(max(1, len(cur.ref)), dtype=engine.EDGE_DTYPE)
            cnt = e.join_to_host(0, T, host.ctypes.data, len(cur.ref))
            self.edges(_canon(host[:cnt]), s.cur, "join_to_host")
        elif call == "join_wait":
            cnt = e.join_wait()
            if s.pending:
                self.edges(_got(self.pend_buf, cnt), s.pending, "join_wait")
            else:
                self.check(cnt == 0, f"join_wait with nothing launched: {cnt}")
            self.pend_buf = None
        elif call == "balanced_cuts":
            cuts = e.balanced_cuts(3)
            self.check(cuts[0] == 0 and cuts[-1] == T and cuts == sorted(cuts), f"balanced_cuts {cuts}")
        elif call == "edge_bound":
            v = e.edge_bound(0, T)
            self.check(v == 0 if cell.zero else v >= len(cur.ref), f"edge_bound {v}")
        elif call == "lists_path":
            v = e.lists_path()
            self.check(v == 0 or not cell.zero, f"lists_path {v}")
        elif call == "stats":
            st = e.stats()
            if s.state == "whole":
                self.check(st["n_sources"] == cur.n_sources and st["n_entries"] == cur.n_entries, f"stats {st}")
        if call in ES.WHOLE_BUILDS:
            st = e.stats()
            self.check(st["n_sources"] == inp.n_sources and st["n_entries"] == inp.n_entries and
                       st["weighted"] == int(inp.weighted), f"stats {st}")

    def close(self):
        self.e.close()
        self.buf2.free()


def test_the_walk_inputs_are_what_the_model_says(pool):
    for name, inp in _walk_inputs().items():
        assert ES.SHARES[name] == (len(inp.ref) > 0), name
        assert (inp.kind == "post") == (name in ES.POSTINGS_INPUTS), name


@pytest.mark.parametrize("seed", ES.WALK_SEEDS)
def test_walk_over_the_state_table(pool, edges_buf, scratch, seed):
    w = Walker(seed, edges_buf, scratch)
    try:
        for s in ES.walk(seed):
            w.step(s)
    finally:
        w.close()
