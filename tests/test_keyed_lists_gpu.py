"""The keyed split of the block lists (k_msk_hist / k_msk_scan / k_msk_place: the lists straight from the per-key group
records, no compaction pass) at the sizes where it can go wrong: chunk and batch boundaries, masks in first and parked
groups, cooperative and huge keys, the limits of the path, both work-list orders, one engine across paths.

Every case compares the whole edge set with the oracle's accumulation, runs the same input again under KSP_MOVE=1 (the
compacting chain) and proves through Engine.lists_path() which path each build took.  With KSP_REORDER=0 a source's
block is its index / 128, and with KSP_HASH_GROUP=0 the ranks are the keys in ascending order: the inputs below place
their keys and groups by construction."""
import numpy as np
import pytest

from kspider_amd import engine, synth

pytestmark = pytest.mark.gpu

KNOBS = ("KSP_REORDER", "KSP_NO_SCHED", "KSP_COLLECT", "KSP_JOIN", "KSP_TAG32", "KSP_HASH_GROUP", "KSP_KEY_GROUPS",
         "KSP_PART_MIN", "KSP_PARTITION", "KSP_ALIGN", "KSP_SEG", "KSP_MS", "KSP_FUSED", "KSP_DEBUG_LATE_SCHED",
         "KSP_FULL_SORT", "KSP_DEBUG_COOP", "KSP_MOVE")
KEYED, COMPACTED, SORTED = engine.LISTS_KEYED, engine.LISTS_COMPACTED, engine.LISTS_SORTED
C = 1024          # MSK_KEYS: keys of a chunk of the keyed split
BATCH = 2048      # MS_CHUNK: records of a batch of k_msk_place
PLAIN = {"KSP_REORDER": "0", "KSP_HASH_GROUP": "0"}
CAP = 1 << 22     # edges of the step_launch buffers


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _setenv(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _sketches(n_sources, held):
    """Key i (ascending key values, spread over 50 bits) is held by the sources held[i]."""
    sizes = [len(h) for h in held]
    src = np.concatenate([np.asarray(h, dtype=np.int64) for h in held])
    key = np.repeat((np.arange(1, len(held) + 1, dtype=np.uint64) << np.uint64(40)) + np.uint64(7), sizes)
    for h in held:
        assert len(set(int(x) for x in h)) == len(h) and max(h) < n_sources
    order = np.lexsort((key, src))
    offsets = np.zeros(n_sources + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(src, minlength=n_sources))
    return key[order].astype(np.uint64), offsets


def _ref(oracle, keys, offsets, weights=None):
    """Edges through the oracle's accumulation over the inverted index (every entry of a key carries the key's weight)."""
    n = offsets.size - 1
    src = np.repeat(np.arange(n, dtype=np.uint32), np.diff(offsets).astype(np.int64))
    w = np.ones(keys.size, dtype=np.uint32) if weights is None else weights
    order = np.argsort(keys, kind="stable")
    k, s, w = keys[order], src[order], w[order]
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    counts = np.diff(np.concatenate([starts, [k.size]]))
    keep = counts >= 2
    key_off = np.zeros(int(keep.sum()) + 1, dtype=np.uint32)
    key_off[1:] = np.cumsum(counts[keep])
    _, _, _, ref = oracle.accumulate_mem(key_off, s[np.repeat(keep, counts)], w[starts[keep]])
    kk = (ref["source_1"].astype(np.uint64) << np.uint64(32)) | ref["source_2"].astype(np.uint64)
    return ref[np.argsort(kk, kind="stable")]


def _same(edges, ref, what):
    assert len(edges) == len(ref), (what, len(edges), len(ref))
    assert (edges["source_1"] == ref["source_1"]).all() and (edges["source_2"] == ref["source_2"]).all(), what
    assert (edges["shared"] == ref["shared"]).all(), (what, "counts differ")


def _sorted(buf, cnt):
    return np.sort(buf.to_numpy(engine.EDGE_DTYPE, cnt), order=["source_1", "source_2"])


def _build_join(e, keys, offsets, weights=None, step=False):
    """One build and a join of all tiles on engine e: (edges, lists path, stats, what the work list says)."""
    dk = engine.DeviceBuffer.from_numpy(keys)
    dw = engine.DeviceBuffer.from_numpy(weights) if weights is not None else None
    try:
        if step:
            de = engine.DeviceBuffer(CAP * 16)
            t0, t1, bound, launched, _ = e.step_launch(dk.ptr.value, offsets, 0, 1, de.ptr.value, CAP,
                                                       d_weights_ptr=dw.ptr.value if dw else 0)
            assert launched and t0 == 0 and t1 == e.num_tiles, (t0, t1, bound, launched)
            cnt = e.join_wait()
        else:
            e.build_blocks(dk.ptr.value, offsets, dw.ptr.value if dw else 0)
            T = e.num_tiles
            cap = e.edge_bound(0, T) + 1
            de = engine.DeviceBuffer(cap * 16)
            cnt = e.join(0, T, de.ptr.value, cap)
        edges = _sorted(de, cnt)
        de.free()
        T = e.num_tiles
        sched = {"cuts": e.balanced_cuts(3), "pairs": e.tile_pairs(0, T), "bound": e.edge_bound(0, T)}
        return edges, e.lists_path(), e.stats(), sched
    finally:
        dk.free()
        if dw:
            dw.free()


def _one(monkeypatch, env, keys, offsets, weights=None, step=False, profiling=False):
    _setenv(monkeypatch, env)
    e = engine.Engine(0)   # (KSP_MOVE is read when the engine is made)
    try:
        e.set_profiling(profiling)
        return _build_join(e, keys, offsets, weights, step)
    finally:
        e.close()


def _check(oracle, monkeypatch, env, keys, offsets, want, what, weights=None, step=False, profiling=False, ref=None):
    """The input under env (lists path `want`) and under env + KSP_MOVE=1, both against the oracle."""
    ref = _ref(oracle, keys, offsets, weights) if ref is None else ref
    edges, path, st, sched = _one(monkeypatch, env, keys, offsets, weights, step, profiling)
    assert path == want, (what, "lists path", path, st)
    _same(edges, ref, (what, env))
    forced = dict(env, KSP_MOVE="1")
    edges2, path2, st2, sched2 = _one(monkeypatch, forced, keys, offsets, weights, step, profiling)
    assert path2 == (want if want != KEYED else COMPACTED), (what, "forced lists path", path2, st2)
    _same(edges2, ref, (what, forced))
    if env.get("KSP_REORDER") == "0":   # (a given source order: the same lists, the same work list)
        for k in ("n_blocks", "n_block_keys", "n_kept_keys", "n_kept_entries", "n_active_tiles", "n_join_workgroups", "n_match_records"):
            assert st[k] == st2[k], (what, k, st[k], st2[k])
        assert sched == sched2, (what, sched, sched2)
    return st


def _blk(b, members):
    """Sources of block b with the given local ids."""
    return [b * 128 + int(x) for x in members]


def _filler(i, block=0, width=8):
    """Key i's default holders: `width` consecutive sources of one block (a mask group: more than 4 members)."""
    s0 = (i * 5) % (128 - width)
    return _blk(block, range(s0, s0 + width))


# ---- chunks: U kept keys around the chunk size ---------------------------------------------------------------------
@pytest.mark.parametrize("U", [1, C - 1, C, C + 1, 2 * C + 1])
def test_chunk_boundaries(oracle_lib, monkeypatch, U):
    """U keys in three blocks; the last key of a chunk, the first key of the next and the last key of all have groups in
    several blocks (first group not in the lowest block for one of them)."""
    held = [_filler(i, i % 3) for i in range(U)]
    multi = {U - 1: [0, 1, 2], C - 1: [2, 0, 1], C: [1, 2], 2 * C - 1: [0, 2], 2 * C: [2, 1, 0]}
    for i, blocks in multi.items():
        if 0 <= i < U:
            held[i] = sum((_blk(b, range(3 + q, 3 + q + 5 + q)) for q, b in enumerate(blocks)), [])
    keys, offsets = _sketches(384, held)
    st = _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, KEYED, f"U={U}")
    assert st["n_blocks"] == 3 and st["n_kept_keys"] == U, st


# ---- batches: a chunk with more records than one batch ---------------------------------------------------------------
def test_chunk_of_several_batches(oracle_lib, monkeypatch):
    """More than C keys, each held in three blocks: 3 x 1 024 records in the first chunk, two batches."""
    U = C + 76
    held = [_blk(0, range(i % 100, i % 100 + 4)) + _blk(1, range(i % 90, i % 90 + 5)) + _blk(2, range(i % 80, i % 80 + 4))
            for i in range(U)]
    assert 3 * C > BATCH
    keys, offsets = _sketches(384, held)
    _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, KEYED, "three blocks a key")


@pytest.mark.parametrize("nb,every", [(12, 200), (256, 10)])
def test_keys_in_every_block(oracle_lib, monkeypatch, nb, every):
    """`every` keys held by one source of every block (nb groups a key: every x nb records in one chunk, more than a
    batch), among keys of one group that keep the sharing dense."""
    n = nb * 128
    held = []
    for i in range(every):
        held.append([b * 128 + (i * 7 + b) % 128 for b in range(nb)])
        for j in range(nb // 8 + 1):
            held.append(_filler(i * 31 + j, (i + j) % nb, 40))
    assert every * nb > BATCH and len(held) < C
    keys, offsets = _sketches(n, held)
    st = _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, KEYED, f"nb={nb}")
    assert st["n_blocks"] == nb


# ---- masks: inline groups and mask groups, first and parked ---------------------------------------------------------
def test_masks_first_and_parked(oracle_lib, monkeypatch):
    """Groups of 1 .. 4 members (inline ids), 5 and 128 members (masks) as a key's first group and as parked ones; every
    group shares its key with a group of another block."""
    rng = np.random.default_rng(11)
    sizes = (1, 2, 3, 4, 5, 128)
    held = []
    for a in sizes:
        for b in sizes:
            for c in sizes:
                if (a + b + c) % 2 and (a, b, c) != (128, 128, 128):
                    continue
                h = []
                for blk, cnt in zip((0, 1, 2), (a, b, c)):
                    h += _blk(blk, rng.choice(128, size=cnt, replace=False))
                held.append(h)
    # the first holder decides the first group: reverse the roles of the blocks for every other key
    for i in range(0, len(held), 2):
        held[i] = [(2 - s // 128) * 128 + s % 128 for s in held[i]]
    keys, offsets = _sketches(384, held)
    _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, KEYED, "masks")


# ---- cooperative and huge keys: KG_COOP = 64, KG_MAXC = 2 048 holders ----------------------------------------------------
@pytest.mark.parametrize("holders", [(64, 65), (2048, 2049)])
def test_coop_and_huge_keys(oracle_lib, monkeypatch, holders):
    n = 17 * 128
    held = [_filler(i, i % 17) for i in range(40)]
    for q, h in enumerate(holders):
        if h <= 128:
            held.insert(5 + 9 * q, _blk(3, range(0, h // 2)) + _blk(5 + q, range(7, 7 + h // 4)) + _blk(9, range(20, 20 + h - h // 2 - h // 4)))
        else:
            held.insert(5 + 9 * q, list(range(q, q + h)))
    for h in held:
        assert len(h) in holders or len(h) == 8
    keys, offsets = _sketches(n, held)
    _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, KEYED, f"holders {holders}")


# ---- limits of the path ----------------------------------------------------------------------------------------------------
def _dense_input(n_sources=384, U=300, seed=5):
    rng = np.random.default_rng(seed)
    nb = n_sources // 128
    held = []
    for i in range(U):
        h = _filler(i, i % nb, 6 + i % 5)
        if i % 3 == 0:
            h += _blk((i + 1) % nb, rng.choice(128, size=1 + i % 7, replace=False))
        held.append(h)
    return _sketches(n_sources, held)


@pytest.mark.parametrize("n_sources,want", [(256 * 128, KEYED), (256 * 128 + 1, COMPACTED)])
def test_block_limit(oracle_lib, monkeypatch, n_sources, want):
    rng = np.random.default_rng(3)
    nb = (n_sources + 127) // 128
    held = [_filler(i, int(rng.integers(0, 256)), 12) for i in range(400)]
    held += [[n_sources - 1, 5, 128 * 200 + 1, 77, 128 * 255 + 126]]
    keys, offsets = _sketches(n_sources, held)
    st = _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, want, f"{nb} blocks")
    assert st["n_blocks"] == nb


@pytest.mark.parametrize("env,want", [({}, KEYED), ({"KSP_MS": "0"}, COMPACTED), ({"KSP_MS": "1024"}, COMPACTED),
                                      ({"KSP_KEY_GROUPS": "0"}, SORTED), ({"KSP_NO_SCHED": "1"}, KEYED),
                                      ({"KSP_JOIN": "matches"}, COMPACTED), ({"KSP_JOIN": "window"}, KEYED),
                                      ({"KSP_COLLECT": "0"}, KEYED), ({"KSP_COLLECT": "1"}, KEYED)])
def test_modes(oracle_lib, monkeypatch, env, want):
    keys, offsets = _dense_input()
    _check(oracle_lib, monkeypatch, dict(PLAIN, **env), keys, offsets, want, env)
    _check(oracle_lib, monkeypatch, env, keys, offsets, want, (env, "reordered"))


def test_weighted_takes_the_compacting_chain(oracle_lib, monkeypatch):
    keys, offsets = _dense_input()
    uk, inv = np.unique(keys, return_inverse=True)
    w = ((np.arange(uk.size, dtype=np.uint64) * 2654435761 % 1000 + 1).astype(np.uint32))[inv]
    _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, COMPACTED, "weighted", weights=w)


def _sparse_input(n_sources=384, U=500):
    """Keys of two holders in two blocks: fewer than four kept entries a group."""
    return _sketches(n_sources, [[(i * 3) % 128, 128 + (i * 5) % 256] for i in range(U)])


def test_sparse_sharing_takes_the_compacting_chain(oracle_lib, monkeypatch):
    keys, offsets = _sparse_input()
    st = _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, COMPACTED, "sparse")
    assert st["n_match_records"] > 0, st


def test_dense_mode(oracle_lib, monkeypatch):
    """Keys in more than six blocks each (K > 6 U): no work list, every tile is visited."""
    nb = 12
    held = [sum((_blk(b, range((i + b) % 100, (i + b) % 100 + 5)) for b in range(nb) if (i + b) % 4), []) for i in range(150)]
    keys, offsets = _sketches(nb * 128, held)
    st = _check(oracle_lib, monkeypatch, PLAIN, keys, offsets, KEYED, "dense mode")
    assert st["n_block_keys"] > 6 * st["n_kept_keys"], st


# ---- both work-list orders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["early", "late", "profiling"])
def test_work_list_orders(oracle_lib, monkeypatch, mode):
    """Engine.step_launch: the work list leaves in front of the placement pass (early), behind the build
    (KSP_DEBUG_LATE_SCHED=1), and with the phase events in the stream."""
    keys, offsets = _dense_input(5 * 128, 1500, seed=9)
    env = dict(PLAIN, KSP_DEBUG_LATE_SCHED="1") if mode == "late" else dict(PLAIN)
    ref = _ref(oracle_lib, keys, offsets)
    st = _check(oracle_lib, monkeypatch, env, keys, offsets, KEYED, mode, step=True, profiling=mode == "profiling", ref=ref)
    assert st["n_active_tiles"] > 0, st
    _check(oracle_lib, monkeypatch, {k: v for k, v in env.items() if k not in PLAIN}, keys, offsets, KEYED, (mode, "reordered"),
           step=True, profiling=mode == "profiling", ref=ref)


# ---- one engine across paths ------------------------------------------------------------------------------------------------
def test_keyed_weighted_keyed_on_one_engine(oracle_lib, monkeypatch):
    _setenv(monkeypatch, PLAIN)
    a = _dense_input(384, 700, seed=1)
    b = _dense_input(640, 300, seed=2)
    uk, inv = np.unique(b[0], return_inverse=True)
    wb = ((np.arange(uk.size, dtype=np.uint64) * 40503 % 97 + 1).astype(np.uint32))[inv]
    c = _dense_input(512, 1300, seed=3)
    e = engine.Engine(0)
    try:
        for name, (keys, offsets), w, want in (("a", a, None, KEYED), ("b weighted", b, wb, COMPACTED), ("c", c, None, KEYED),
                                               ("a again", a, None, KEYED)):
            for step in (False, True):
                edges, path, st, _ = _build_join(e, keys, offsets, w, step)
                assert path == want, (name, step, path, st)
                _same(edges, _ref(oracle_lib, keys, offsets, w), (name, step))
    finally:
        e.close()


def test_sparse_input_switches_the_engine_for_good(oracle_lib, monkeypatch):
    _setenv(monkeypatch, PLAIN)
    a = _dense_input(384, 700, seed=1)
    s = _sparse_input()
    e = engine.Engine(0)
    try:
        for name, (keys, offsets), want in (("a", a, KEYED), ("sparse", s, COMPACTED), ("a again", a, COMPACTED)):
            edges, path, st, _ = _build_join(e, keys, offsets)
            assert path == want, (name, path, st)
            _same(edges, _ref(oracle_lib, keys, offsets), name)
    finally:
        e.close()


# ---- alignment modes on a clustered input -----------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KSP_ALIGN": "0"}, {"KSP_REORDER": "0"}])
def test_alignment_modes(oracle_lib, monkeypatch, env):
    # (clusters in source order: with KSP_REORDER=0 the blocks still hold related sources and the sharing stays dense)
    sk = synth.generate("C2", n_sources=2000, mean_size=300, cluster_cap=40, seed=77, shuffle=False)
    _check(oracle_lib, monkeypatch, env, sk.keys, sk.offsets, KEYED, env)
