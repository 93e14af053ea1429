"""Key-range sharded stage 1 (the multi-GPU build) on one GPU: build every slice in turn, "exchange"
them through plain device buffers, assemble, join — the result must equal the single-build result and
the brute-force oracle."""
import numpy as np
import pytest

from kspider_amd import engine, synth
from slice_driver import sliced_edges

pytestmark = pytest.mark.gpu


def _sliced_edges(sk, nparts, weights=None):
    return sliced_edges(sk, nparts, weights)[:2]


@pytest.mark.parametrize("nparts", [1, 2, 3, 8])
def test_sliced_build_equals_oracle(oracle_lib, nparts):
    sk = synth.generate("C2", n_sources=420, mean_size=500, cluster_cap=40, seed=321)
    got, sizes = _sliced_edges(sk, nparts)
    ref = oracle_lib.brute_pairs(sk.keys, sk.offsets)
    assert len(got) == len(ref) and (got == ref).all()
    if nparts > 1:
        assert (sizes[3::4] > 0).all()           # every key range holds shared keys


def test_sliced_build_big_postings_weights_and_empty_slices(oracle_lib):
    # contiguous clusters -> postings with > 4 holders (masks); full 64-bit keys; 5 parts
    sk = synth.generate("C4", n_sources=300, mean_size=250, cluster_cap=60, seed=322, shuffle=False)
    got, _ = _sliced_edges(sk, 5)
    ref = oracle_lib.brute_pairs(sk.keys, sk.offsets)
    assert (got == ref).all()
    # weighted mode + keys crowded into the lowest range (most slices are empty)
    runs = [np.arange(1, 60, dtype=np.uint64) * np.uint64(3 + (s % 4)) for s in range(150)]
    runs.append(np.array([1 << 40], dtype=np.uint64))      # stretches the key range: parts 1.. are (almost) empty
    sk2 = synth.from_runs(runs)
    w = (sk2.keys % np.uint64(7) + np.uint64(1)).astype(np.uint32)
    got2, sizes2 = _sliced_edges(sk2, 4, weights=w)
    single, _ = engine.pairwise_host(sk2.keys, sk2.offsets, w)
    assert (got2 == single).all() and len(got2) > 1000
    assert (sizes2[3::4] == 0).any()
