"""The definition of compare (include/kspider_amd.h) restated with Python dicts and integers, and its four derived
values with math.  A source is a dict hash -> abundance (>= 1); a flat source has every abundance 1.  Nothing here calls the code
under test."""
import math

CROSS, CROSS_AND_SELF = 0, 1


def totals(sources):
    """([Σ a], [Σ a²]) per source, exact"""
    return [sum(s.values()) for s in sources], [sum(a * a for a in s.values()) for s in sources]


def rows(db, q, mode):
    """The rows (source_1, source_2, shared, dot, mass_1, mass_2) of the mode, sorted: database sources are 0 .. len(db) - 1, the
    queries follow; CROSS keeps database x query, CROSS_AND_SELF also query x query, each pair once with source_1 < source_2."""
    sources = list(db) + list(q)
    n_db = len(db)
    holders = {}
    for s, src in enumerate(sources):
        for h in src:
            holders.setdefault(h, []).append(s)
    acc = {}
    for h, who in holders.items():
        for i, s1 in enumerate(who):
            for s2 in who[i + 1:]:
                if s2 < n_db or (mode == CROSS and s1 >= n_db):
                    continue
                a1, a2 = sources[s1][h], sources[s2][h]
                r = acc.setdefault((s1, s2), [0, 0, 0, 0])
                r[0] += 1
                r[1] += a1 * a2
                r[2] += a1
                r[3] += a2
    return sorted((s1, s2, *r) for (s1, s2), r in acc.items())


def values(row, sum_1, sumsq_1, sum_2, sumsq_2):
    """(cosine, angular similarity, weighted containment 1, weighted containment 2) of a row"""
    _, _, _, dot, mass_1, mass_2 = row
    cosine = 1.0 if dot * dot == sumsq_1 * sumsq_2 else min(1.0, dot / (math.sqrt(sumsq_1) * math.sqrt(sumsq_2)))
    return cosine, 1.0 - 2.0 * math.acos(cosine) / math.pi, mass_1 / sum_1, mass_2 / sum_2
