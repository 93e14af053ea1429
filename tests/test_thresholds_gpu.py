"""Inputs built to sit on the size constants that choose a kernel path, a table size or a counter width: every
threshold at N - 1, N and N + 1.  Each case compares the whole edge set with a reference (the oracle, or a closed form
for inputs built by construction) and proves which side of the threshold it took, from the build's stats or from a
restatement of the bucket function (tests/edge_inputs.py).  Random and config-shaped inputs almost never land here."""
import os
import shutil

import numpy as np
import pytest

import edge_inputs as E
from kspider_amd import engine

pytestmark = pytest.mark.gpu

KNOBS = ("KSP_REORDER", "KSP_NO_SCHED", "KSP_COLLECT", "KSP_JOIN", "KSP_TAG32", "KSP_HASH_GROUP", "KSP_KEY_GROUPS",
         "KSP_PART_MIN", "KSP_PARTITION", "KSP_ALIGN", "KSP_SEG", "KSP_MS", "KSP_FUSED", "KSP_DEBUG_FK_GB",
         "KSP_DEBUG_PART_SORTED", "KSP_DEBUG_LABEL_SPREAD", "KSP_DEBUG_LATE_SCHED", "KSP_FULL_SORT",
         "KSP_DEBUG_BUCKET_MEAN", "KSP_DEBUG_NO16CUT", "KSP_DEBUG_NO_MID", "KSP_DEBUG_SEG_PB2", "KSP_DEBUG_SHARES",
         "KSP_DEBUG_COOP")
JOIN_MODES = ({"KSP_COLLECT": "0"}, {"KSP_COLLECT": "1"}, {"KSP_JOIN": "window"}, {"KSP_JOIN": "matches"},
              {"KSP_JOIN": "matches", "KSP_COLLECT": "0"}, {"KSP_JOIN": "matches", "KSP_COLLECT": "1"})


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _run(monkeypatch, env, keys, offsets, weights=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return engine.pairwise_host(keys, offsets, weights)


def _same(edges, ref, what):
    assert len(edges) == len(ref), (what, len(edges), len(ref))
    assert (edges["source_1"] == ref["source_1"]).all() and (edges["source_2"] == ref["source_2"]).all(), what
    assert (edges["shared"] == ref["shared"]).all(), (what, "counts differ")


def _engine_run(keys, offsets):
    """One build and a join of all tiles on an Engine (the environment as set): (edges, stats, engine index of every
    source: block x 128 + slot)."""
    n = offsets.size - 1
    dk = engine.DeviceBuffer.from_numpy(keys)
    e = engine.Engine(0)
    try:
        e.build_blocks(dk.ptr.value, offsets)
        st = e.stats()
        slot = e.source_order(n)
        T = e.num_tiles
        cap = e.edge_bound(0, T) + 1
        de = engine.DeviceBuffer(cap * 16)
        cnt = e.join(0, T, de.ptr.value, cap)
        edges = np.sort(de.to_numpy(engine.EDGE_DTYPE, cnt), order=["source_1", "source_2"])
        de.free()
    finally:
        dk.free()
        e.close()
    return edges, st, slot


def _edges(rows):
    out = np.zeros(len(rows), dtype=engine.EDGE_DTYPE)
    for i, (a, b, c) in enumerate(sorted(rows)):
        out[i] = (a, b, c)
    return out


def _weighted_ref(oracle, keys, offsets, weights):
    """Edges of weighted sketches (every entry of a key carries the key's weight) through the oracle's accumulation."""
    n = offsets.size - 1
    src = np.repeat(np.arange(n, dtype=np.uint32), np.diff(offsets).astype(np.int64))
    order = np.argsort(keys, kind="stable")
    k, s, w = keys[order], src[order], weights[order]
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    counts = np.diff(np.concatenate([starts, [k.size]]))
    keep = counts >= 2
    key_off = np.zeros(int(keep.sum()) + 1, dtype=np.uint32)
    key_off[1:] = np.cumsum(counts[keep])
    _, _, _, ref = oracle.accumulate_mem(key_off, s[np.repeat(keep, counts)], w[starts[keep]])
    kk = (ref["source_1"].astype(np.uint64) << np.uint64(32)) | ref["source_2"].astype(np.uint64)
    return ref[np.argsort(kk, kind="stable")]


# ---- LDS table sizes (416 / 832 / 1664) and HB_CAP (3 072) of k_bucket_group ---------------------------------------
HAND_NB = 4


def _hand_env(n, extra):
    env = {"KSP_PART_MIN": "1", "KSP_DEBUG_BUCKET_MEAN": str((n + HAND_NB - 1) // HAND_NB)}
    env.update(extra)
    return env


def _hand_sizes(keys):
    n = keys.size
    nb = E.hand_nbuckets(n, (n + HAND_NB - 1) // HAND_NB)
    assert nb == HAND_NB
    return E.bucket_sizes(E.hand_buckets(keys, nb), nb)


def _lib_sizes(keys):
    pb, topbit = E.lib_pb(keys.size, E.key_bits(int(keys.max())))
    assert pb > 0, "the library partition must group buckets (>= 4 096 entries)"
    return pb, E.bucket_sizes(E.lib_buckets(keys, pb, topbit), 1 << pb)


def _check_bucket_case(oracle_lib, monkeypatch, size, kind, n_sources, label):
    """The bucket of `size` entries in every stage-1 mode: hand-written partition paged / segment / bucket-resident,
    library partition; the big_buckets stat against the restatement's count of buckets above HB_CAP."""
    # hand-written partition: 4 buckets (0 and 2 filler, 3 the one under test); filler buckets below HB_CAP
    fill = 2 * min(size, 3000)
    keys, offsets = E.bucket_input(size, fill, n_sources, kind)
    sizes = _hand_sizes(keys)
    assert sizes[HAND_NB - 1] == size and sizes.sum() == keys.size, (label, sizes)
    big = int((sizes > E.HB_CAP).sum())
    cap = E.seg_cap(keys.size, HAND_NB)
    assert sizes.max() <= cap, (label, "the segment partition must hold every bucket", sizes, cap)
    ref = oracle_lib.brute_pairs(keys, offsets)
    # (the bucket-resident path hands sparse sharing — fewer than 4 kept entries a group — on to the match-list join
    #  unless the window join is asked for: under "fused/window" its own records are what the join reads)
    for name, extra, pkind in (("paged", {"KSP_SEG": "0"}, 2), ("segment", {"KSP_SEG": "1"}, 3),
                               ("fused", {"KSP_FUSED": "1"}, None), ("fused/window", {"KSP_FUSED": "1", "KSP_JOIN": "window"}, None),
                               ("paged/no key groups", {"KSP_SEG": "0", "KSP_KEY_GROUPS": "0"}, 2)):
        edges, st = _run(monkeypatch, _hand_env(keys.size, extra), keys, offsets)
        _same(edges, ref, (label, name))
        what = (label, name, st)
        assert st["partition_fallback"] == 0, what
        assert st["sort_bits"] == 2, what   # (the grouping ran on 2^2 buckets, not the sort path)
        if pkind is not None:
            assert st["partition_kind"] == pkind, what
        if name == "fused/window" or (name == "fused" and kind != "pairs"):   # ("pairs": keys of two holders, sparse)
            # the bucket-resident path takes no oversize bucket: it hands the build on and k_bucket_group runs
            assert st["stage1_kind"] == (0 if big else 1), what
        assert st["big_buckets"] == big, what
    # library partition (the same bucket at the top of a larger key set: >= 4 096 entries)
    fill = max(2 * min(size, 3000), 4096 - size)
    keys, offsets = E.bucket_input(size, fill, n_sources, kind)
    pb, sizes = _lib_sizes(keys)
    assert sizes[-1] == size and sizes.sum() == keys.size, (label, sizes)
    ref = oracle_lib.brute_pairs(keys, offsets)
    edges, st = _run(monkeypatch, {"KSP_PARTITION": "rocprim"}, keys, offsets)
    _same(edges, ref, (label, "rocprim"))
    assert st["partition_kind"] == 1 and st["sort_bits"] == pb, (label, st)
    assert st["big_buckets"] == int((sizes > E.HB_CAP).sum()), (label, st)
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, ref, (label, "default"))
    # weighted: the library partition again, every entry of a key with the key's weight
    uk, inv = np.unique(keys, return_inverse=True)
    wk = (np.arange(uk.size, dtype=np.uint64) * 2654435761 % 1000 + 1).astype(np.uint32)
    w = wk[inv]
    wref = _weighted_ref(oracle_lib, keys, offsets, w)
    edges, st = _run(monkeypatch, {}, keys, offsets, w)
    _same(edges, wref, (label, "weighted"))
    assert st["weighted"] and st["sort_bits"] == pb and st["big_buckets"] == int((sizes > E.HB_CAP).sum()), (label, st)


@pytest.mark.parametrize("size", [415, 416, 417, 831, 832, 833, 1663, 1664, 1665])
def test_bucket_table_sizes(oracle_lib, monkeypatch, size):
    _check_bucket_case(oracle_lib, monkeypatch, size, "mixed", 150, f"table {size}")


@pytest.mark.parametrize("size", [3071, 3072, 3073])
def test_bucket_hb_cap(oracle_lib, monkeypatch, size):
    _check_bucket_case(oracle_lib, monkeypatch, size, "mixed", 200, f"HB_CAP {size}")


@pytest.mark.parametrize("kind,n_sources", [("pairs", 200), ("one", 3072)])
def test_bucket_hb_cap_shapes(oracle_lib, monkeypatch, kind, n_sources):
    """3 072 entries as 1 536 keys of two holders (more than FK_KEYB = 1 024 keys: a second mask round of k_fkeys, whose
    records the join reads under KSP_FUSED=1 KSP_JOIN=window, stage1_kind 1), or as a single key of 3 072 holders."""
    _check_bucket_case(oracle_lib, monkeypatch, 3072, kind, n_sources, f"HB_CAP {kind}")


# ---- HB_BIG_DISTINCT: distinct keys of an oversize bucket (k_bucket_big, or the sort path beyond) --------------------
@pytest.mark.parametrize("distinct", [3071, 3072, 3073])
def test_big_bucket_distinct_keys(oracle_lib, monkeypatch, distinct):
    size = 3200   # entries of the bucket: more than HB_CAP
    keys, offsets = E.bucket_input(size, 6000, 200, f"distinct:{distinct}")
    sizes = _hand_sizes(keys)
    assert sizes[-1] == size and sizes[:-1].max() <= E.HB_CAP, sizes
    top = keys[E.hand_buckets(keys, HAND_NB) == HAND_NB - 1]
    # (the all-ones key is in the bucket too, in a slot of its own: the table counts the others)
    assert np.unique(top[top != np.uint64(E.ALL_ONES)]).size == distinct and top.size == size
    ref = oracle_lib.brute_pairs(keys, offsets)
    for extra in ({"KSP_SEG": "0"}, {"KSP_SEG": "0", "KSP_KEY_GROUPS": "0"}):
        edges, st = _run(monkeypatch, _hand_env(keys.size, extra), keys, offsets)
        _same(edges, ref, (distinct, extra))
        if distinct <= 3072:   # k_bucket_big grouped it: the bucket path on 2^2 buckets
            assert st["sort_bits"] == 2 and st["big_buckets"] == 1 and st["partition_kind"] == 2, (distinct, st)
        else:                  # too many distinct keys for its table: the build was handed to the sort path
            assert st["sort_bits"] >= 32 and st["big_buckets"] == 0, (distinct, st)
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, ref, (distinct, "default"))


# ---- the segment partition's bucket capacity seg_cap (k_seg_scatter: at + c > cap) --------------------------------
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_segment_bucket_capacity(oracle_lib, monkeypatch, delta):
    n = 3000
    cap = E.seg_cap(n, HAND_NB)
    size = cap + delta
    keys, offsets = E.bucket_input(size, n - size, 150, "mixed")
    assert keys.size == n
    sizes = _hand_sizes(keys)
    assert sizes[-1] == size and sizes[:-1].max() <= cap, (sizes, cap)
    ref = oracle_lib.brute_pairs(keys, offsets)
    edges, st = _run(monkeypatch, _hand_env(n, {"KSP_SEG": "1"}), keys, offsets)
    _same(edges, ref, ("seg_cap", delta))
    if delta <= 0:
        assert st["partition_fallback"] == 0 and st["partition_kind"] == 3, st
    else:   # the bucket overflowed its range: handed to the paged partition
        assert st["partition_fallback"] == 5 and st["partition_kind"] == 2, st
    assert st["big_buckets"] == 0, st
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, ref, ("seg_cap default", delta))


# ---- per-block holder counts: INLINE_MAX (posting word vs mask), DENSE_MAX (dense grid), FK_SMALL -------------------
def _block_key_input(holders_a, holders_b, n_sources=256, seed=0):
    """Key 7 held by `holders_a` sources of block 0 and `holders_b` of block 1 (KSP_REORDER=0: block = source // 128),
    plus a background of random keys so the tiles have other work."""
    rng = np.random.default_rng(seed + 31 * holders_a + holders_b)
    runs = [set(int(x) for x in rng.integers(100, 5000, size=int(rng.integers(0, 30)))) for _ in range(n_sources)]
    for s in list(range(holders_a)) + list(range(128, 128 + holders_b)):
        runs[s].add(7)
    offsets = np.zeros(n_sources + 1, dtype=np.uint64)
    rs = [np.array(sorted(r), dtype=np.uint64) for r in runs]
    offsets[1:] = np.cumsum([r.size for r in rs])
    keys = np.concatenate(rs)
    # restatement: holders of key 7 per block
    src = np.repeat(np.arange(n_sources), np.diff(offsets).astype(np.int64))
    per_block = np.bincount(src[keys == 7] // 128, minlength=2)
    assert per_block[0] == holders_a and per_block[1] == holders_b
    return keys, offsets


@pytest.mark.parametrize("h", [3, 4, 5, 6])
def test_inline_max_holders(oracle_lib, monkeypatch, h):
    for ha, hb in ((h, 2), (2, h), (h, h), (h, 0)):
        keys, offsets = _block_key_input(ha, hb)
        ref = oracle_lib.brute_pairs(keys, offsets)
        for env in JOIN_MODES:
            edges, st = _run(monkeypatch, dict(env, KSP_REORDER="0"), keys, offsets)
            _same(edges, ref, (ha, hb, env))
            assert st["n_blocks"] == 2, st
        edges, _ = _run(monkeypatch, {}, keys, offsets)
        _same(edges, ref, (ha, hb, "default"))


@pytest.mark.parametrize("h", [47, 48, 49])
def test_dense_max_holders(oracle_lib, monkeypatch, h):
    for ha, hb in ((3, h), (h, 3), (h, h), (1, h)):
        keys, offsets = _block_key_input(ha, hb)
        ref = oracle_lib.brute_pairs(keys, offsets)
        for env in JOIN_MODES:
            edges, st = _run(monkeypatch, dict(env, KSP_REORDER="0"), keys, offsets)
            _same(edges, ref, (ha, hb, env))
            assert st["n_blocks"] == 2, st
        edges, _ = _run(monkeypatch, {}, keys, offsets)
        _same(edges, ref, (ha, hb, "default"))


@pytest.mark.parametrize("h", [7, 8, 9])
def test_fk_small_holders(oracle_lib, monkeypatch, h):
    """A key of h holders spread over three families of 128 sources (each family shares 16 keys of its own, so the
    source order keeps it in one block): a key in several blocks for k_fkeys, in registers up to FK_SMALL = 8."""
    fam, per = 3, 128
    runs = []
    for f in range(fam):   # (key values spread over the whole range: no bucket of the partition above HB_CAP)
        for i in range(per):
            runs.append({7 + (f * 16 + j + 1) * 40009 for j in range(16)} | {20013 + (f * per + i) * 5003})
    holders = [(q % fam) * per + q // fam for q in range(h)]
    for s in holders:
        runs[s].add(7)
    rs = [np.array(sorted(r), dtype=np.uint64) for r in runs]
    offsets = np.zeros(len(rs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in rs])
    keys = np.concatenate(rs)
    src = np.repeat(np.arange(len(rs)), np.diff(offsets).astype(np.int64))
    assert (keys == 7).sum() == h and np.unique(src[keys == 7] // per).size == min(h, fam)
    nbh = E.hand_nbuckets(keys.size, 2000)   # (the engine's default bucket mean)
    assert E.bucket_sizes(E.hand_buckets(keys, nbh), nbh).max() <= E.HB_CAP
    ref = oracle_lib.brute_pairs(keys, offsets)
    for env in ({"KSP_FUSED": "1", "KSP_PART_MIN": "1"}, {"KSP_FUSED": "1", "KSP_PART_MIN": "1", "KSP_SEG": "0"}):
        edges, st = _run(monkeypatch, env, keys, offsets)
        _same(edges, ref, (h, env))
        assert st["stage1_kind"] == 1 and st["big_buckets"] == 0 and st["n_blocks"] >= fam, (h, env, st)
        # the same build on an engine: where the source order put the key's holders (the several-block branch)
        edges, st, slot = _engine_run(keys, offsets)
        _same(edges, ref, (h, env, "engine"))
        assert st["stage1_kind"] == 1, st
        assert np.unique(slot[holders] // 128).size >= 2, (h, env, slot[holders])
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, ref, (h, "default"))


# ---- key-by-key list build: KG_COOP = 64 / KG_MAXC = 2 048 holders, CR_CHUNK = KG_CHUNK = 4 096 kept entries -------
@pytest.mark.parametrize("h", [63, 64, 65, 2047, 2048, 2049])
def test_key_group_holders(oracle_lib, monkeypatch, h):
    n_sources = h + 60
    b = E.Built(n_sources)
    b.hold(7, h)                                        # sources 0 .. h - 1
    for q in range(400):                                # background: keys of 2 .. 5 holders
        b.hold(100 + q, 2 + q % 4)
    keys, offsets = b.arrays()
    assert (keys == 7).sum() == h
    ref = oracle_lib.brute_pairs(keys, offsets)
    for env in ({}, {"KSP_KEY_GROUPS": "0"}, {"KSP_REORDER": "0"}):
        edges, st = _run(monkeypatch, env, keys, offsets)
        _same(edges, ref, (h, env))
        assert st["n_kept_keys"] == 401, st
    uk, inv = np.unique(keys, return_inverse=True)
    w = ((np.arange(uk.size) * 7919) % 500 + 1).astype(np.uint32)[inv]
    wref = _weighted_ref(oracle_lib, keys, offsets, w)
    edges, st = _run(monkeypatch, {}, keys, offsets, w)
    _same(edges, wref, (h, "weighted"))


@pytest.mark.parametrize("k", [4095, 4096, 4097])
def test_huge_key_list(monkeypatch, k):
    """k keys held by all of 2 049 sources (more than KG_MAXC = 2 048 holders each: listed for k_key_groups_huge, which
    takes KG_HUGE_CAP = 4 096 of them; one more sends the build to the fallback), about 8.4 M entries.  Every pair of
    sources shares all k keys (closed form)."""
    n = 2049
    keys = np.tile(np.arange(1, k + 1, dtype=np.uint64), n)
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(k)
    # the input at the threshold: keys with more than 2 048 holders
    assert int((np.bincount(keys.astype(np.int64)) > 2048).sum()) == k and keys.size < 10_000_000
    s1, s2 = np.triu_indices(n, 1)
    want = np.zeros(s1.size, dtype=engine.EDGE_DTYPE)
    want["source_1"], want["source_2"], want["shared"] = s1, s2, k
    for env in ({}, {"KSP_REORDER": "0"}):
        edges, st = _run(monkeypatch, env, keys, offsets)
        _same(edges, want, (k, env))
        assert st["n_kept_keys"] == k and st["n_kept_entries"] == keys.size, st


@pytest.mark.parametrize("kept", [4095, 4096, 4097, 8192])
def test_kept_entry_chunks(oracle_lib, monkeypatch, kept):
    """Kept-entry totals around the 4 096-entry chunks of crank[] and the key-by-key list build: one key of 102 holders,
    keys of 3, and one key of 2 or 4 for the remainder; singletons that the prune drops.  Kept entries go key by key in
    an order the test does not know; with these holder counts every key boundary is 0 or 2 (mod 3) for 4 097 and 8 192,
    never 4 096 = 1 (mod 3), so some key's holders straddle entry 4 096 whatever the order."""
    counts = [102]
    rest = kept - 102
    counts += [3] * (rest // 3 - (rest % 3 == 1))
    counts += {0: [], 1: [4], 2: [2]}[rest % 3]
    assert sum(counts) == kept
    b = E.Built(300)
    for q, h in enumerate(counts):
        b.hold(5000 + q, h)
    for j in range(700):
        b.hold(100000 + j, 1)
    keys, offsets = b.arrays()
    if kept > 4096:   # boundaries mod 3 reachable from these holder counts: 4 096 is not among them
        assert all(c % 3 == 0 for c in counts if c % 3 != kept % 3) and sum(c % 3 != 0 for c in counts) == 1
        assert 4096 % 3 not in {0, kept % 3}
    ref = oracle_lib.brute_pairs(keys, offsets)
    for env in ({}, {"KSP_FUSED": "1", "KSP_PART_MIN": "1"}, {"KSP_PART_MIN": "1"}, {"KSP_KEY_GROUPS": "0"}):
        edges, st = _run(monkeypatch, env, keys, offsets)
        _same(edges, ref, (kept, env))
        assert st["n_kept_entries"] == kept, (kept, env, st)


# ---- FK_NB_MAX = MS_MAXB = 1 024 blocks: the split's tables and the bucket-resident stage 1 ------------------------
@pytest.mark.parametrize("nb", [1023, 1024, 1025])
def test_block_table_limit(monkeypatch, nb):
    """nb blocks of 128 sources (KSP_ALIGN=0: plain cuts); sources in groups of 8 share 4 keys of their own."""
    n = 128 * nb
    src = np.arange(n, dtype=np.uint64)
    keys = ((src // 8)[:, None] * 4 + np.arange(4, dtype=np.uint64)[None, :] + 1).reshape(-1)
    offsets = np.arange(n + 1, dtype=np.uint64) * 4
    g = np.arange(0, n, 8, dtype=np.int64)
    xs, ys = np.triu_indices(8, 1)                     # (row-major: the pairs of a group in (source_1, source_2) order)
    want = np.zeros(g.size * xs.size, dtype=engine.EDGE_DTYPE)
    want["source_1"] = (g[:, None] + xs[None, :]).reshape(-1)
    want["source_2"] = (g[:, None] + ys[None, :]).reshape(-1)
    want["shared"] = 4
    for env, fused in (({"KSP_FUSED": "1", "KSP_MS": "1024"}, nb <= 1024), ({"KSP_FUSED": "1", "KSP_MS": "0"}, False),
                       ({"KSP_MS": "1024"}, False), ({"KSP_MS": "0"}, False)):
        edges, st = _run(monkeypatch, dict(env, KSP_ALIGN="0"), keys, offsets)
        _same(edges, want, (nb, env))
        assert st["n_blocks"] == nb and st["stage1_kind"] == int(fused), (nb, env, st)
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, want, (nb, "default"))


# ---- join windows (WIN = 256 keys) and match records (MSUB = 512, MCAP = 2 048) -----------------------------------
@pytest.mark.parametrize("k", [255, 256, 257, 512])
def test_window_keys(monkeypatch, k):
    keys, offsets = E.pair_input(k, 200, 5, 150)
    want = _edges([(5, 150, k)])
    for env in ({"KSP_JOIN": "window"}, {"KSP_JOIN": "window", "KSP_NO_SCHED": "1"}, {"KSP_NO_SCHED": "1"}):
        edges, st = _run(monkeypatch, dict(env, KSP_REORDER="0"), keys, offsets)
        _same(edges, want, (k, env))
        assert st["n_block_keys"] == 2 * k and st["n_blocks"] == 2, st
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, want, (k, "default"))


@pytest.mark.parametrize("k", [511, 512, 513, 2047, 2048, 2049])
def test_match_records(monkeypatch, k):
    keys, offsets = E.pair_input(k, 200, 5, 150)
    want = _edges([(5, 150, k)])
    for env in ({"KSP_JOIN": "matches"}, {"KSP_JOIN": "matches", "KSP_COLLECT": "0"}, {"KSP_JOIN": "matches", "KSP_COLLECT": "1"}):
        edges, st = _run(monkeypatch, dict(env, KSP_REORDER="0"), keys, offsets)
        _same(edges, want, (k, env))
        assert st["n_match_records"] == k, (k, env, st)
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, want, (k, "default"))


# ---- 16-bit / 32-bit counters ---------------------------------------------------------------------------------------
# The host marks a tile for the 32-bit pass (act32) and the device checks the same rule (join_workgroup: lim); a pair
# whose blocks both hold a source of >= 2^16 keys needs 32 bits.  No other tile of these inputs needs 32 bits, so the
# host's rule alone decides whether the 32-bit pass runs at all.
# (sparse sharing like this takes the match-list join by default, whose shares the host cuts at 65 535 records; the
#  window join counts a whole off-diagonal tile in one share: the host's act32 alone decides its width)
COUNTER_MODES = ({}, {"KSP_COLLECT": "0"}, {"KSP_COLLECT": "1"}, {"KSP_JOIN": "matches"}, {"KSP_DEBUG_NO16CUT": "1"},
                 {"KSP_JOIN": "matches", "KSP_DEBUG_NO16CUT": "1"}, {"KSP_JOIN": "window"},
                 {"KSP_JOIN": "window", "KSP_COLLECT": "0"}, {"KSP_JOIN": "window", "KSP_COLLECT": "1"},
                 {"KSP_JOIN": "window", "KSP_DEBUG_NO16CUT": "1"}, {"KSP_JOIN": "window", "KSP_NO_SCHED": "1"})


@pytest.mark.parametrize("k", [65535, 65536, 65537])
@pytest.mark.parametrize("where", ["two blocks", "one block"])
def test_counter_width_unweighted(monkeypatch, k, where):
    b = 128 if where == "two blocks" else 1
    keys, offsets = E.pair_input(k, 129, 0, b)
    want = _edges([(0, b, k)])
    for env in COUNTER_MODES:
        edges, st = _run(monkeypatch, dict(env, KSP_REORDER="0"), keys, offsets)
        _same(edges, want, (k, where, env))
        assert st["n_blocks"] == 2, st
        if env.get("KSP_JOIN") == "matches" and where == "two blocks":
            assert st["n_match_records"] == k, st
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, want, (k, where, "default"))


def test_counter_width_two_full_shares(monkeypatch):
    """Match join, a pair sharing 2 x 65 535 keys: two 16-bit shares of 65 535 records meet in the tile's 32-bit tail
    buffer."""
    k = 2 * 65535
    keys, offsets = E.pair_input(k, 129, 0, 128)
    want = _edges([(0, 128, k)])
    for env in ({"KSP_JOIN": "matches"}, {"KSP_JOIN": "matches", "KSP_COLLECT": "0"}, {"KSP_JOIN": "matches", "KSP_COLLECT": "1"}):
        edges, st = _run(monkeypatch, dict(env, KSP_REORDER="0"), keys, offsets)
        _same(edges, want, env)
        assert st["n_match_records"] == k, st
    edges, _ = _run(monkeypatch, {}, keys, offsets)
    _same(edges, want, "default")


@pytest.mark.parametrize("total", [65535, 65536, 65537])
def test_counter_width_weighted(oracle_lib, monkeypatch, total):
    """Two sources in different blocks, three shared keys whose colour weights sum to `total`: the block weight-sum
    maximum (lim) sits on the 16-bit edge."""
    keys, offsets = E.pair_input(3, 129, 0, 128)
    w3 = [total // 3, total // 3, total - 2 * (total // 3)]
    w = np.array(w3 + w3, dtype=np.uint32)
    assert int(w[:3].astype(np.int64).sum()) == total
    want = _edges([(0, 128, total)])
    assert (_weighted_ref(oracle_lib, keys, offsets, w) == want).all()
    for env in ({"KSP_REORDER": "0"}, {"KSP_REORDER": "0", "KSP_NO_SCHED": "1"}, {"KSP_REORDER": "0", "KSP_KEY_GROUPS": "0"}):
        edges, st = _run(monkeypatch, env, keys, offsets, w)
        _same(edges, want, (total, env))
        assert st["weighted"] and st["n_blocks"] == 2, st
    edges, _ = _run(monkeypatch, {}, keys, offsets, w)   # (default mode: the source order on)
    _same(edges, want, (total, "default"))


def _three_weights(total):
    return [total // 3, total // 3, total - 2 * (total // 3)]


@pytest.mark.parametrize("total", [2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2, 2**32 - 1])
def test_weight_sums_at_the_top_of_the_contract(oracle_lib, monkeypatch, total):
    """The input of test_counter_width_weighted with weight sums up to 2^32 - 1, the largest the contract of the weighted calls
    admits (include/kspider_amd.h: every source's weights sum to less than 2^32): the sum fills a 32-bit pair counter, the
    per-source bound and the blocks' maxima, which only ever choose the counter width.  Through the weighted sketches and through
    the inverted index the drop-in path feeds the engine."""
    keys, offsets = E.pair_input(3, 129, 0, 128)
    w3 = _three_weights(total)
    w = np.array(w3 + w3, dtype=np.uint32)
    assert int(w[:3].astype(np.int64).sum()) == total < 2**32
    want = _edges([(0, 128, total)])
    assert (_weighted_ref(oracle_lib, keys, offsets, w) == want).all()
    key_off = np.array([0, 2, 4, 6], dtype=np.uint64)
    holders = np.array([0, 128] * 3, dtype=np.uint32)
    for env in ({"KSP_REORDER": "0"}, {"KSP_REORDER": "0", "KSP_NO_SCHED": "1"}, {"KSP_REORDER": "0", "KSP_KEY_GROUPS": "0"}, {}):
        edges, st = _run(monkeypatch, env, keys, offsets, w)
        _same(edges, want, (total, env, "sketches"))
        assert st["weighted"] and (st["n_blocks"] == 2 or not env), st
        edges, st = engine.pairwise_postings_host(key_off, holders, np.array(w3, dtype=np.uint32), 129)
        _same(edges, want, (total, env, "postings"))


def _limit_index(oracle_lib, prefix, total):
    """Groups 1 and 2 share three colours whose weights sum to `total`; groups 3 and 4 share one of weight 7."""
    w3 = _three_weights(total)
    oracle_lib.write_index(prefix, np.array([0, 2, 4, 6, 8]), np.array([1, 2, 2, 1, 1, 2, 3, 4]), np.array(w3 + [7], dtype=np.uint32),
                           np.array([1, 2, 3, 4]), np.array([2**32 - 1, 2**32 - 1, 100, 50], dtype=np.uint32))


def test_drop_in_weight_sum_limit(oracle_lib, tmp_path):
    """A group whose colour weights sum to exactly 2^32 - 1 is served; at exactly 2^32 the call is refused with KSP_E_LIMIT and a
    message that names the limit and the group, leaves nothing behind, and the next call is right."""
    (tmp_path / "top").mkdir()
    (tmp_path / "over").mkdir()
    top, over = str(tmp_path / "top" / "ix"), str(tmp_path / "over" / "ix")
    _limit_index(oracle_lib, top, 2**32 - 1)
    _limit_index(oracle_lib, over, 2**32)
    shutil.copytree(tmp_path / "top", tmp_path / "ref")
    oracle_lib.ref_pairwise(str(tmp_path / "ref" / "ix"), 1)
    with open(str(tmp_path / "ref" / "ix") + "_kSpider_pairwise.tsv", "rb") as f:
        want = f.read()
    assert want.split(b"\n")[1].split(b"\t")[:3] == [b"1", b"2", b"4294967295"] and want.count(b"\n") == 3
    before = sorted(os.listdir(tmp_path / "over"))
    with pytest.raises(engine.KspError) as ei:
        engine.pairwise(over, 2)
    assert ei.value.code == engine.KSP_E_LIMIT and "2^32" in str(ei.value) and "group 1" in str(ei.value), str(ei.value)
    assert sorted(os.listdir(tmp_path / "over")) == before
    engine.pairwise(top, 2)
    with open(top + "_kSpider_pairwise.tsv", "rb") as f:
        assert f.read() == want
    assert not [n for n in os.listdir(tmp_path / "top") if n.endswith(".partial")]


# ---- u16 / u32 source tags at 65 536 sources ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_source_tags_width(monkeypatch, n):
    """n sources in pairs (2i, 2i + 1) sharing one key each, and the last source sharing keys with the first."""
    src = np.arange(n, dtype=np.uint64)
    pair_key = (src // 2) * 4 + 10                     # sources 2i, 2i + 1: one key
    runs = [[int(pair_key[s])] for s in range(n)]
    runs[0] += [1, 2, 3]
    runs[n - 1] += [1, 2, 3]
    rs = [np.array(sorted(r), dtype=np.uint64) for r in runs]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in rs])
    keys = np.concatenate(rs)
    rows = [(2 * i, 2 * i + 1, 1) for i in range(n // 2)]
    rows = [(a, b, c + (3 if (a, b) == (0, n - 1) else 0)) for a, b, c in rows]
    if (0, n - 1) not in {(a, b) for a, b, _ in rows}:
        rows.append((0, n - 1, 3))
    want = _edges(rows)
    for env in ({}, {"KSP_TAG32": "1"}):
        edges, st = _run(monkeypatch, env, keys, offsets)
        _same(edges, want, (n, env))
        assert st["n_sources"] == n, st
