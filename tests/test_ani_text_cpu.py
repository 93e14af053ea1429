"""kspider_estimate_ani reads numbers as Python's int() / float() do, underscores between digits included, and refuses
what they refuse; the Python API needs the scale."""
import os

import pytest

from ani_restate import estimate_ani as restated
from kspider_amd import engine


def _files(tmp_path, rows, extra="21\n"):
    prefix = str(tmp_path / "u")
    with open(prefix + "_kSpider_pairwise.tsv", "w") as f:
        f.write("source_1\tsource_2\tshared_kmers\tmin_containment\tavg_containment\tmax_containment\n")
        f.write("".join(r + "\n" for r in rows))
    with open(prefix + "_kSpider_seqToKmersNo.tsv", "w") as f:
        f.write("ID\tseq\tkmers\n1\t1\t100\n2\t2\t1_000\n3\t1_0\t50\n")
    with open(prefix + ".extra", "w") as f:
        f.write(extra)
    return prefix


def test_underscores_between_digits_are_python_numbers(tmp_path):
    rows = ["1\t2\t3\t0.5_5\t0.6\t0.7_5", "1_0\t2\t1_2\t1_0e-0_1\t0.5\t0.99_99", "2\t1_0\t1\t+0.25\t0.3\t 0.4 "]
    prefix = _files(tmp_path, rows, extra="2_1\n")
    engine.estimate_ani(prefix, 2, 1_000)
    got = open(prefix + "_kSpider_pairwise.ani_col.tsv", "rb").read()
    assert got == restated(prefix, 1000)


@pytest.mark.parametrize("bad", ["0._5", "0.5_", "_0.5", "0.5__5", "0x1p-1"])
def test_texts_python_refuses_are_refused(tmp_path, bad):
    prefix = _files(tmp_path, ["1\t2\t3\t0.5\t0.6\t0.75", f"1\t2\t3\t{bad}\t0.6\t0.75"])
    with pytest.raises(ValueError):
        restated(prefix, 1000)
    with pytest.raises(engine.KspError):
        engine.estimate_ani(prefix, 2, 1000)
    assert not os.path.exists(prefix + "_kSpider_pairwise.ani_col.tsv")


def test_scale_is_required():
    with pytest.raises(TypeError):
        engine.estimate_ani("unused")   # noqa: the scale has no default
    with pytest.raises(TypeError):
        engine.pairwise_ani("unused", 1)
