"""Gather, restated: the definition of DESIGN.md 7o in Python sets.  Calls nothing of the product.

Every query q with hash set Q, on its own:  R = Q, rank = 0;  loop: u(s) = |S_s & R| for every database source s; s* = the source
with the largest u, among equals the smallest s; stop when u(s*) < min_hashes or (max_matches and rank == max_matches);
otherwise rank += 1, R -= S_s*, row (q, rank, s*, |S_s* & Q|, u(s*), |R|).  Rows come out ordered by (query, rank)."""


def gather(db_runs, q_runs, min_hashes=1, max_matches=0, counts=None):
    """The rows as tuples (query, rank, source, overlap, unique, remaining).  `counts`, a dict, also receives what a round-by-round
    implementation can be asked about: candidates (pairs with overlap >= min_hashes), dropped (0 < overlap < min_hashes),
    fell_below (candidates found below min_hashes in a round in which their query still counted) and iterations (per query:
    the rounds in which it still counted; a query stopped by max_matches does not count once more)."""
    sets = [set(int(k) for k in run) for run in db_runs]
    rows, tally = [], {"candidates": 0, "dropped": 0, "fell_below": 0, "iterations": []}
    for q, run in enumerate(q_runs):
        Q = set(int(k) for k in run)
        shared = {s: S & Q for s, S in enumerate(sets) if S & Q}          # a source without a shared hash has u = 0 for good
        tally["dropped"] += sum(len(c) < min_hashes for c in shared.values())
        running = {s for s, c in shared.items() if len(c) >= min_hashes}  # neither taken nor found below min_hashes yet
        tally["candidates"] += len(running)
        R, rank, iterations = set(Q), 0, 0
        while not (max_matches and rank == max_matches):
            iterations += 1
            u = {s: len(c & R) for s, c in shared.items()}
            tally["fell_below"] += sum(u[s] < min_hashes for s in running)
            running = {s for s in running if u[s] >= min_hashes}
            best = min(u, key=lambda s: (-u[s], s)) if u else None
            if best is None or u[best] < min_hashes:
                break
            rank += 1
            R -= shared[best]
            running.discard(best)
            rows.append((q, rank, best, len(shared[best]), u[best], len(R)))
        tally["iterations"].append(iterations)
    if counts is not None:
        counts.update(tally)
    return rows
