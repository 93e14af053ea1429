"""k_label by lane groups: KSP_LABEL_LANES = 1 (a thread per sampled key), 2, 16 and 64 give the same labels — atomicMin
commutes — so the same source order, blocks, lists and edges; and the labels are what a numpy restatement says.

Inputs are built key by key (a chosen number of holders each) and run through the four-bucket hand partition of
tests/test_thresholds_gpu.py.  The join hands out edge positions with an atomic cursor shared by its workgroups, so
the emitted order is not a function of the input even for one setting: the edges are compared row for row after sorting,
the source order and the list / tile counts exactly as they come.

A key's rank inside a bucket is its slot in the bucket's hash table, and which of two colliding keys takes a slot is
decided by a race: with every key looked at the labels do not depend on the ranks, but WHICH keys a sampling pass
(KSP_DEBUG_LABEL_EVERY > 1) looks at differs from build to build, whatever the lanes.  So the sampled cases compare the
lane counts on the sort path (KSP_HASH_GROUP=0: ranks in key order, a function of the input) — there the sampled labels
are restated too — and check the edges alone on the bucket path."""
import numpy as np
import pytest

from kspider_amd import engine

pytestmark = pytest.mark.gpu

KNOBS = ("KSP_LABEL_LANES", "KSP_PART_MIN", "KSP_PARTITION", "KSP_SEG", "KSP_FUSED", "KSP_KEY_GROUPS",
         "KSP_DEBUG_BUCKET_MEAN", "KSP_DEBUG_LABEL_MAX", "KSP_DEBUG_LABEL_EVERY", "KSP_DEBUG_LABEL_SPREAD", "KSP_ALIGN",
         "KSP_REORDER", "KSP_JOIN", "KSP_COLLECT", "KSP_MS")
LANES = (1, 2, 16, 64)
LABEL_MAX = 40
# holders per key: L - 1, L, L + 1 and 2 L + 1 for L = 2, 16, 64 (a kept key has at least two), LABEL_MAX and LABEL_MAX + 1
HOLDERS = (2, 3, 5, 15, 16, 17, 33, 63, 64, 65, 129, LABEL_MAX, LABEL_MAX + 1)


def _build(n_sources, n_keys, seed, singles=300):
    """n_keys shared keys, their holder counts cycling through HOLDERS, held by random sources; some keys of one holder."""
    rng = np.random.default_rng(seed)
    ks = np.unique(rng.integers(1, (1 << 64) - 1, size=n_keys + singles + 16, dtype=np.uint64))
    rng.shuffle(ks)
    runs = [[] for _ in range(n_sources)]
    holders = {}
    for q in range(n_keys):
        h = min(HOLDERS[q % len(HOLDERS)], n_sources)
        who = rng.choice(n_sources, size=h, replace=False)
        holders[int(ks[q])] = np.sort(who)
        for s in who:
            runs[s].append(ks[q])
    for q in range(n_keys, n_keys + singles):
        runs[int(rng.integers(n_sources))].append(ks[q])
    rs = [np.sort(np.asarray(r, dtype=np.uint64)) for r in runs]
    offsets = np.zeros(n_sources + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([r.size for r in rs])
    return np.concatenate(rs), offsets, holders


def _env(n, extra):
    env = {"KSP_PART_MIN": "1", "KSP_DEBUG_BUCKET_MEAN": str((n + 3) // 4)}
    env.update(extra)
    return env


def _engine_run(monkeypatch, env, keys, offsets):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
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


def _across_lanes(oracle_lib, monkeypatch, keys, offsets, extra, label, buckets=True, same_order=True):
    """buckets: the four-bucket hand partition (else the sort path); same_order: the source order and the list counts
    must not depend on the lanes (else only the edges are checked)."""
    ref = oracle_lib.brute_pairs(keys, offsets)
    first = None
    for lanes in LANES:
        env = dict(extra, KSP_LABEL_LANES=str(lanes))
        env = _env(keys.size, env) if buckets else dict(env, KSP_HASH_GROUP="0")
        edges, st, slot = _engine_run(monkeypatch, env, keys, offsets)
        what = (label, lanes)
        if buckets:
            assert st["sort_bits"] == 2 and st["stage1_kind"] == 0, (what, st)   # (four buckets grouped pass by pass: k_label ran)
        else:
            assert st["sort_bits"] > 2 and st["partition_kind"] == 1 and st["stage1_kind"] == 0, (what, st)
        assert len(edges) == len(ref) and (edges == ref).all(), what
        assert np.unique(slot).size == slot.size, (what, "two sources in one slot")
        same = {k: st[k] for k in ("n_blocks", "n_block_keys", "n_tiles", "n_active_tiles", "n_kept_entries", "n_kept_keys")}
        if first is None:
            first = (slot, same)
        elif same_order:
            assert (slot == first[0]).all(), (what, "source order differs from one lane per key")
            assert same == first[1], (what, same, first[1])
    return first[0], first[1]


@pytest.mark.parametrize("n_sources", [200, 1000])
def test_holder_counts_around_every_group_size(oracle_lib, monkeypatch, n_sources):
    keys, offsets, _ = _build(n_sources, 20 * len(HOLDERS) + 1, 5 + n_sources)
    _across_lanes(oracle_lib, monkeypatch, keys, offsets, {}, f"{n_sources} sources")
    _across_lanes(oracle_lib, monkeypatch, keys, offsets, {"KSP_DEBUG_LABEL_MAX": str(LABEL_MAX)}, f"{n_sources} sources, label max")


def _want_order(n_sources, holder_lists):
    """Engine index of every source for blocks cut every 128 sources of the (label, id) order."""
    label = np.arange(n_sources, dtype=np.int64)
    for who in holder_lists:
        if who.size <= LABEL_MAX:
            label[who] = np.minimum(label[who], who[0])
    order = np.lexsort((np.arange(n_sources), label))
    want = np.empty(n_sources, dtype=np.int64)
    want[order] = np.arange(n_sources)
    return want


@pytest.mark.parametrize("n_keys", [4 * 37 + 1, 4 * 37 + 2])
@pytest.mark.parametrize("every", [1, 4])
def test_sampling_and_last_group(oracle_lib, monkeypatch, n_keys, every):
    """Kept keys = 4 m + 1 (the last key is sampled at every 4th) and 4 m + 2 (it is not); neither fills the last lane
    group of a workgroup (256 / lanes groups each)."""
    keys, offsets, holders = _build(200, n_keys, 77 + n_keys)
    assert len(holders) == n_keys and n_keys % 4 != 0
    extra = {"KSP_DEBUG_LABEL_EVERY": str(every), "KSP_DEBUG_LABEL_MAX": str(LABEL_MAX), "KSP_ALIGN": "0"}
    _, st = _across_lanes(oracle_lib, monkeypatch, keys, offsets, extra, f"{n_keys} keys, every {every}", same_order=every == 1)
    assert st["n_kept_keys"] == n_keys, st
    # the sort path: key r of the sorted kept keys is looked at when r is a multiple of `every`
    slot, st = _across_lanes(oracle_lib, monkeypatch, keys, offsets, extra, f"{n_keys} keys, every {every}, sorted", buckets=False)
    assert st["n_kept_keys"] == n_keys, st
    looked_at = sorted(holders)[::every]
    assert (looked_at[-1] == max(holders)) == ((n_keys - 1) % every == 0)
    assert (slot.astype(np.int64) == _want_order(200, [holders[k] for k in looked_at])).all()


def test_labels_not_spread(oracle_lib, monkeypatch):
    keys, offsets, _ = _build(200, 300, 9)
    a, _ = _across_lanes(oracle_lib, monkeypatch, keys, offsets, {"KSP_DEBUG_LABEL_SPREAD": "0"}, "labels in place")
    b, _ = _across_lanes(oracle_lib, monkeypatch, keys, offsets, {}, "labels spread")
    assert (a == b).all()


@pytest.mark.parametrize("n_sources", [130, 700])
def test_labels_against_restatement(oracle_lib, monkeypatch, n_sources):
    """Every key looked at, no padding of the blocks: label[s] = the smallest holder over the kept keys s holds that
    have at most LABEL_MAX holders (s itself otherwise), and the sources in (label, id) order."""
    keys, offsets, holders = _build(n_sources, 400, 31 + n_sources)
    assert sum(who.size > LABEL_MAX for who in holders.values()) > 0
    want = _want_order(n_sources, holders.values())
    slot, _ = _across_lanes(oracle_lib, monkeypatch, keys, offsets,
                            {"KSP_DEBUG_LABEL_EVERY": "1", "KSP_ALIGN": "0", "KSP_DEBUG_LABEL_MAX": str(LABEL_MAX)}, "restatement")
    assert (slot.astype(np.int64) == want).all()
