"""Weighted gather, restated: the definition of DESIGN.md 7q in Python sets, dicts and ints.  Calls nothing of the product.

The greedy is gather_restate.gather's, written out again here: selection by the unweighted u(s), ties to the smaller source, the
same stops.  Query q has the abundance a(h) of every hash h of its set Q.  For the row of rank r, T = S_s* & R before the removal
and n = |T| = unique; the row also carries
    w_unique = sum of a(h) over T            w_found = the sum of w_unique over the ranks 1 .. r of this query
    sq       = sum of a(h)^2 over T          (a Python int; the product splits it into two 64-bit words)
    median2  = a_(ceil(n/2)) + a_(floor(n/2)+1) of T's abundances in ascending order, counted from 1: twice the median."""
import math


def gather(db_runs, q_runs, q_abunds, min_hashes=1, max_matches=0):
    """The rows as tuples (query, rank, source, overlap, unique, remaining, w_unique, w_found, sq, median2)."""
    sets = [set(int(k) for k in run) for run in db_runs]
    rows = []
    for q, (run, abunds) in enumerate(zip(q_runs, q_abunds)):
        a = {}
        for k, v in zip(run, abunds):
            a[int(k)] = int(v)
        Q = set(a)
        shared = {s: S & Q for s, S in enumerate(sets) if S & Q}
        R, rank, found = set(Q), 0, 0
        while not (max_matches and rank == max_matches):
            u = {s: len(c & R) for s, c in shared.items()}
            best = min(u, key=lambda s: (-u[s], s)) if u else None
            if best is None or u[best] < min_hashes:
                break
            T = shared[best] & R
            taken = sorted(a[h] for h in T)
            n = len(taken)
            rank += 1
            R -= shared[best]
            w = sum(taken)
            found += w
            median2 = taken[(n + 1) // 2 - 1] + taken[n // 2]
            rows.append((q, rank, best, len(shared[best]), n, len(R), w, found, sum(v * v for v in taken), median2))
    return rows


def split_sq(sq):
    """(sq_lo, sq_hi) of the 128-bit sum of squares"""
    return sq & (2**64 - 1), sq >> 64


def columns(row, total_w):
    """The four floating-point columns of the file as Python floats (the file casts each to single precision): f_unique_weighted,
    average_abund, median_abund, std_abund = sqrt(n * sq - w_unique^2) / n with the numerator an exact int, rounded once."""
    n, w, sq, median2 = row[4], row[6], row[8], row[9]
    return (w / total_w if total_w else 0.0, w / n, median2 / 2, math.sqrt(float(n * sq - w * w)) / n)
