"""The six-source index of tests/test_tree_gpu.py::test_zero_weight_colours, for the other fused calls.  Colours: {1, 2} weight 7;
{3, 4} weight 0 (the pair shares nothing else: a row that exists only with shared_kmers = 0); {5, 6} weight 0 AND {5, 6} weight 1
(an ordinary row).  "nan": source 4 counts 0 k-mers, so the row 3-4 is a NaN row."""
import numpy as np

COUNTS = {"plain": [10, 20, 30, 40, 50, 60], "nan": [10, 20, 30, 0, 50, 60]}


def write(oracle_lib, prefix: str, sub: str) -> None:
    co = np.array([0, 2, 4, 6, 8], dtype=np.uint32)
    src = np.array([1, 2, 3, 4, 5, 6, 5, 6], dtype=np.uint32)
    w = np.array([7, 0, 0, 1], dtype=np.uint32)
    oracle_lib.write_index(prefix, co, src, w, np.arange(1, 7, dtype=np.uint32), np.array(COUNTS[sub]))
    with open(prefix + ".namesMap", "w") as f:
        f.write("6\n")
        for i in range(6):
            f.write(f"{i + 1} genome_{i + 1}\n")
