"""The definition of compare (include/kspider_amd.h) restated with Python dicts and integers, and its four derived
values twice: with math's doubles (values) and with fractions and decimals of 60 digits (values_exact).  A source is a dict hash -> abundance (>= 1); a flat source has every abundance 1.  Nothing here calls the code
under test."""
import decimal
import fractions
import functools
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


def refusal(db_side, q_side):
    """What the check pass says about two sides given as (keys, abund or None, offsets), or None for sides it accepts: the smallest
    source (database first) whose run is not strictly ascending; without one, the smallest source with an abundance of 0."""
    order, zero = [], []
    for side, (keys, abund, off) in (("database", db_side), ("query", q_side)):
        for s in range(len(off) - 1):
            run = [int(k) for k in keys[int(off[s]):int(off[s + 1])]]
            if any(b <= a for a, b in zip(run, run[1:])):
                order.append("the run of %s source %d is not strictly ascending" % (side, s))
            if abund is not None and any(int(a) == 0 for a in abund[int(off[s]):int(off[s + 1])]):
                zero.append("%s source %d has an abundance of 0" % (side, s))
    return (order + zero + [None])[0]


def values(row, sum_1, sumsq_1, sum_2, sumsq_2):
    """(cosine, angular similarity, weighted containment 1, weighted containment 2) of a row"""
    _, _, _, dot, mass_1, mass_2 = row
    cosine = 1.0 if dot * dot == sumsq_1 * sumsq_2 else min(1.0, dot / (math.sqrt(sumsq_1) * math.sqrt(sumsq_2)))
    return cosine, 1.0 - 2.0 * math.acos(cosine) / math.pi, mass_1 / sum_1, mass_2 / sum_2


# ---- the four values again, without a double anywhere: integers, fractions and decimals of DIGITS digits --------------------
DIGITS = 60


def _ctx():
    return decimal.Context(prec=DIGITS + 10, rounding=decimal.ROUND_HALF_EVEN)


def _dec(x, ctx):
    """a Fraction, an int or a Decimal as a Decimal of the context's precision"""
    if isinstance(x, fractions.Fraction):
        return ctx.divide(decimal.Decimal(x.numerator), decimal.Decimal(x.denominator))
    return ctx.create_decimal(x)


def atan_exact(t):
    """atan of t >= 0: the complement above 1, four halvings of the angle (atan t = 2 atan(t / (1 + sqrt(1 + t²)))), which leave
    t below 0.07, and the alternating series t - t³/3 + t⁵/5 - ... to beyond the context's last digit"""
    ctx = _ctx()
    t = _dec(t, ctx)
    if t > 1:
        return ctx.subtract(ctx.divide(pi_exact(), 2), atan_exact(ctx.divide(1, t)))
    for _ in range(4):
        t = ctx.divide(t, ctx.add(1, ctx.sqrt(ctx.add(1, ctx.multiply(t, t)))))
    total, power, t2, n = decimal.Decimal(0), t, ctx.multiply(t, t), 0
    while power != 0 and power.adjusted() > -(DIGITS + 10):
        term = ctx.divide(power, 2 * n + 1)
        total = ctx.subtract(total, term) if n % 2 else ctx.add(total, term)
        power = ctx.multiply(power, t2)
        n += 1
    return ctx.multiply(total, 16)


@functools.lru_cache(maxsize=None)
def pi_exact():
    """Machin: π = 16 atan(1/5) - 4 atan(1/239)"""
    ctx = _ctx()
    return ctx.subtract(ctx.multiply(16, atan_exact(fractions.Fraction(1, 5))), ctx.multiply(4, atan_exact(fractions.Fraction(1, 239))))


def cos_exact(x):
    """cos of a Decimal |x| <= 2 by its series (the identity cos(acos c) = c checks acos_exact with it)"""
    ctx = _ctx()
    x2 = ctx.multiply(x, x)
    total, term, n = decimal.Decimal(0), decimal.Decimal(1), 0
    while term != 0 and term.adjusted() > -(DIGITS + 10):
        total = ctx.subtract(total, term) if n % 2 else ctx.add(total, term)
        n += 1
        term = ctx.divide(ctx.multiply(term, x2), (2 * n - 1) * (2 * n))
    return total


def acos_exact(num, den_sq):
    """acos of c = num / sqrt(den_sq) for integers 0 < num² <= den_sq: the angle whose tangent is sqrt(den_sq - num²) / num.  The
    difference under the root is an exact integer, so nothing cancels however close c is to 1."""
    ctx = _ctx()
    return atan_exact(ctx.divide(ctx.sqrt(decimal.Decimal(den_sq - num * num)), decimal.Decimal(num)))


def values_exact(row, sum_1, sumsq_1, sum_2, sumsq_2):
    """(cosine, angular similarity, weighted containment 1, weighted containment 2) of a row as Decimals good to DIGITS digits;
    exactly 1 and 1 for parallel samples (dot² = Σ a² · Σ a²)"""
    _, _, _, dot, mass_1, mass_2 = (int(v) for v in row)
    ctx = _ctx()
    den_sq = int(sumsq_1) * int(sumsq_2)
    if dot * dot == den_sq:
        cosine, angular = decimal.Decimal(1), decimal.Decimal(1)
    else:
        cosine = ctx.divide(decimal.Decimal(dot), ctx.sqrt(decimal.Decimal(den_sq)))
        angular = ctx.subtract(1, ctx.divide(ctx.multiply(2, acos_exact(dot, den_sq)), pi_exact()))
    return cosine, angular, _dec(fractions.Fraction(mass_1, int(sum_1)), ctx), _dec(fractions.Fraction(mass_2, int(sum_2)), ctx)
