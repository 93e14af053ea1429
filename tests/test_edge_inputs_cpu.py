"""The bucket-function restatements of tests/edge_inputs.py on hand-computed values (the threshold tests build their
inputs with them, and the GPU stats check them against the device)."""
import numpy as np

import edge_inputs as E


def test_hand_mult_cases():
    assert E.hand_mult(5, 8) == (0, 1)                  # maxkey <= nb: every key its own bucket
    assert E.hand_mult(8, 8) == (0, 1)
    assert E.hand_mult(2**64 - 1, 4) == (4, 0)          # all-ones maxkey: umulhi(key, nb)
    assert E.hand_mult(9, 8) == ((8 << 64) // 10, 0)    # general: floor(nb 2^64 / (maxkey + 1))
    assert E.hand_mult(2**32 - 1, 3) == (3 << 32, 0)    # maxkey + 1 a power of two: exact
    assert E.hand_mult(999, 7) == (129127208515966861, 0)   # floor(7 * 2^64 / 1000)


def test_hand_buckets_identity():
    keys = np.array([0, 1, 2, 3, 5], dtype=np.uint64)
    assert E.hand_buckets(keys, 8).tolist() == [0, 1, 2, 3, 5]
    assert E.hand_buckets(np.array([0, 3, 4], dtype=np.uint64), 4).tolist() == [0, 3, 3]   # (clamped to nb - 1)


def test_hand_buckets_all_ones():
    top = 2**64 - 1
    keys = np.array([0, 2**62 - 1, 2**62, 2**63, 3 * 2**62, top], dtype=np.uint64)
    assert E.hand_buckets(keys, 4).tolist() == [0, 0, 1, 2, 3, 3]
    assert E.hand_buckets(keys, 3).tolist() == [0, 0, 0, 1, 2, 2]   # umulhi(key, 3) = floor(3 key / 2^64)


def test_hand_buckets_general():
    keys = np.arange(0, 1000, dtype=np.uint64)
    b = E.hand_buckets(keys, 7)
    mult = (7 << 64) // 1000
    assert b.tolist() == [(int(k) * mult) >> 64 for k in keys]
    assert b[0] == 0 and b[-1] == 6 and b[142] == 0 and b[143] == 1   # 143 * 7 / 1000 = 1.001
    sizes = E.bucket_sizes(b, 7)
    assert sizes.sum() == 1000 and sizes.tolist() == [143, 143, 143, 143, 143, 143, 142]


def test_umulhi_exact():
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 2**63, size=500, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for mult in (1, 3, 2**32 - 1, 2**32 + 7, 2**63 + 12345, 2**64 - 1):
        got = E._umulhi(keys, mult)
        assert got.tolist() == [(int(k) * mult) >> 64 for k in keys]


def test_hand_nbuckets():
    assert E.hand_nbuckets(1000, 250) == 4
    assert E.hand_nbuckets(1001, 250) == 5
    assert E.hand_nbuckets(10, 1) == 2      # (the engine takes a mean of at least 8)
    assert E.hand_nbuckets(0, 100) == 1


def test_seg_cap():
    assert E.seg_cap(3000, 4) == 1280       # mean 751: 751 + 375 + 191 = 1317 -> 1280
    assert E.seg_cap(1248, 4) == 640        # mean 313: 660 -> 640
    assert E.seg_cap(9000, 4) % 64 == 0


def test_lib_partition():
    assert E.key_bits(0) == 1 and E.key_bits(1) == 1 and E.key_bits(2) == 2 and E.key_bits(2**64 - 1) == 64
    assert E.lib_pb(4095, 64) == (0, 63)    # below 4 096 entries: the sort path
    assert E.lib_pb(4096, 64) == (3, 63)    # 4096 >> 3 = 512 <= 800
    assert E.lib_pb(6407, 64) == (3, 63)    # 6407 >> 3 = 800
    assert E.lib_pb(6408, 64) == (4, 63)    # 801
    assert E.lib_pb(1 << 20, 10) == (0, 10)   # more bits than the keys have: the sort path
    keys = np.array([0, 2**60, 2**62, 2**63 + 5, 2**64 - 1, 7 << 60], dtype=np.uint64)
    # bits [60, 63) of the key; bit 63 is folded away
    assert E.lib_buckets(keys, 3, 63).tolist() == [0, 1, 4, 0, 7, 7]
    assert E.lib_buckets(np.array([5 << 10, 1 << 13], dtype=np.uint64), 3, 13).tolist() == [5, 0]


def test_bucket_input_sizes():
    for size, fill in ((416, 832), (3073, 6000), (1280, 1720)):
        keys, offsets = E.bucket_input(size, fill, 150)
        assert keys.size == size + fill and int(offsets[-1]) == keys.size
        sizes = E.bucket_sizes(E.hand_buckets(keys, 4), 4)
        assert sizes.tolist() == [(fill + 1) // 2, 0, fill // 2, size] and sizes.sum() == keys.size
        pb, topbit = E.lib_pb(keys.size, 64)
        if pb:
            ls = E.bucket_sizes(E.lib_buckets(keys, pb, topbit), 1 << pb)
            assert ls[-1] == size and ls.sum() == keys.size
    keys, _ = E.bucket_input(3072, 6000, 3072, "one")
    assert (keys == np.uint64(2**64 - 1)).sum() == 3072
    keys, _ = E.bucket_input(3200, 6000, 200, "distinct:3073")
    top = keys[E.hand_buckets(keys, 4) == 3]
    assert top.size == 3200 and np.unique(top).size == 3074 and np.unique(top[top != np.uint64(2**64 - 1)]).size == 3073


def test_pair_input():
    keys, offsets = E.pair_input(5, 10, 2, 7)
    assert offsets.tolist() == [0, 0, 0, 5, 5, 5, 5, 5, 10, 10, 10]
    assert keys.tolist() == [1, 2, 3, 4, 5] * 2
