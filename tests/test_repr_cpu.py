"""Representative sketches without a GPU: the restatement of apps/repr_sketches.cpp (tests/repr_restate.py) on
hand-written TSV text, and the host-only critical float of the text test (ksp_repr_critical)."""
import struct

import numpy as np
import pytest

import repr_restate as rr
from kspider_amd import engine

HEADER = "source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n"


def _row(a, b, avg, shared=5, mn="0.1", mx="0.9"):
    return f"{a}\t{b}\t{shared}\t{mn}\t{avg}\t{mx}\n"


def test_restatement_on_hand_written_text():
    tsv = HEADER + "".join([
        _row(1, 2, "0.2"),          # stof("0.2") = 0.200000003 > 0.20: passes
        _row(1, 3, "0.199999"),     # fails
        _row(1, 4, "0.200001"),     # passes
        _row(2, 5, "nan"),          # fails
        _row(2, 6, "-nan"),         # fails
        _row(3, 7, "0"),            # fails
        _row(8, 9, "0.75"),         # passes; 9 is only ever column 1
        _row(3, 9, "1"),            # passes
    ])
    assert rr.counts(tsv) == {1: 2, 2: 1, 4: 1, 8: 1, 9: 2, 3: 1}
    assert rr.ranked(rr.counts(tsv)) == [(1, 2), (9, 2), (2, 1), (3, 1), (4, 1), (8, 1)]
    assert rr.repr_sketches(tsv) == b"1: 2\n9: 2\n2: 1\n3: 1\n4: 1\n8: 1\n"
    # the header is skipped even when it would parse: a first line of numbers is not counted
    assert rr.counts(_row(50, 60, "0.9") + _row(1, 2, "0.9")) == {1: 1, 2: 1}
    # other columns and thresholds
    assert rr.counts(tsv, col=3) == {} and len(rr.counts(tsv, col=5)) == 9
    assert rr.counts(tsv, threshold=-1.0)[7] == 1 and 5 not in rr.counts(tsv, threshold=-1.0)   # "0" passes, a NaN never does
    # strtof, not a double rounded twice: the float of "0.2" is above the double 0.2, the float of "0.7" is below 0.7
    assert rr.strtof("0.2") > 0.2 and rr.strtof("0.7") < 0.7
    assert rr.float_passes(np.float32(0.1999996)) and not rr.float_passes(np.float32(0.1999994))


def _bits(v) -> int:
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def _float(bits: int) -> np.float32:
    return np.float32(struct.unpack("<f", struct.pack("<I", bits))[0])


def test_critical_float_of_the_reference_threshold():
    v, none = engine.repr_critical(0.20)
    assert not none and _bits(v) == 0x3E4CCCAC
    assert _bits(np.float32(0.2)) == 0x3E4CCCCD        # (0.2f itself is 33 floats higher)


@pytest.mark.parametrize("threshold", [0.0, 0.2, 0.5, 0.999999, 1.0, -1.0])
def test_critical_float_is_the_smallest_that_passes_the_text_test(threshold):
    v, none = engine.repr_critical(threshold)
    assert not none
    b = _bits(v)
    assert b < 0x7F800000 and rr.float_passes(v, threshold)
    if b == 0:   # the bisection runs over the non-negative floats: nothing lies below +0.0, and 0 must pass by itself
        assert threshold < 0 and rr.text_passes("0", threshold)
    else:
        assert not rr.float_passes(_float(b - 1), threshold)


def test_critical_float_edges():
    assert engine.repr_critical(float("inf")) == (np.float32(0), True)       # not even +inf is > inf
    v, none = engine.repr_critical(3.0e38)
    assert not none and rr.float_passes(v, 3.0e38) and not rr.float_passes(_float(_bits(v) - 1), 3.0e38)
    v, none = engine.repr_critical(1e39)                                    # above every finite float: only +inf passes
    assert not none and _bits(v) == 0x7F800000
    with pytest.raises(engine.KspError) as ei:
        engine.repr_critical(float("nan"))
    assert ei.value.code == engine.KSP_E_ARG


def test_argument_checks_need_no_device(tmp_path):
    """Refusals that are decided before any device call."""
    with pytest.raises(engine.KspError) as ei:
        engine.repr_sketches(str(tmp_path / "x.tsv"), "ani", 0.20, str(tmp_path / "out"))
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.edges_degrees(4, 0, 0, 0, dist_col=6)
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.edges_degrees(4, 0, 1 << 32, 0)           # (NULL pointers with edges: refused first)
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.edges_repr(4, 0, 0, 0, threshold=float("nan"))
    assert ei.value.code == engine.KSP_E_ARG
    with pytest.raises(engine.KspError) as ei:
        engine.pairwise_and_repr(str(tmp_path / "nope"), 1, "ani", 0.20)
    assert ei.value.code == engine.KSP_E_ARG
    assert not list(tmp_path.iterdir())
