"""The engine's C API as a state table (DESIGN.md 7g-2 holds the same table as the contract), and seeded walks over it.

Five states, told apart by the fields that decide what a call may do (engine.hip: built, slice_phase, slice_ready):

    fresh      nothing built (or the last build failed)                    built 0, slice_phase 0, slice_ready 0
    whole      build_blocks / step_launch / build_postings went through    built 1
    labels     build_slice / build_postings_slice went through             slice_phase 1
    finished   slice_finish went through                                   slice_ready 1
    assembled  assemble went through                                       built 1, slice_ready 1

A launched, uncollected join is a sixth bit beside the state: it changes the cells of PENDING only, it survives every
call but join_wait and step_launch (which collect it), and it is collected with the count and the edges of the build it
was launched on.

No library call and no GPU here: tests/test_engine_states_cpu.py checks the table and the walks on this model alone;
tests/test_engine_sequences_gpu.py makes the same walks on an engine."""
from collections import namedtuple

import numpy as np

STATES = ("fresh", "whole", "labels", "finished", "assembled")
JOINABLE = ("whole", "assembled")

WHOLE_BUILDS = ("build_blocks", "step_launch", "build_postings")
SLICE_BUILDS = ("build_slice", "build_postings_slice")
AT_LABELS = ("slice_labels", "slice_bounds", "slice_set_bounds", "slice_finish")
AT_READY = ("slice_sizes", "slice_export", "assemble")
JOINS = ("join", "join_launch", "join_to_host")
CALLS = WHOLE_BUILDS + SLICE_BUILDS + AT_LABELS + AT_READY + JOINS + ("join_wait", "balanced_cuts", "edge_bound", "lists_path", "stats")

# kind: "ok" (accepted: made with valid arguments), "refused" (raises `code` with `stem` in its message and changes
# nothing) or "unspecified" (accepted by the code, its result promised by nobody: never offered by a walk).
# zero: an accepted query that must answer 0 in this state.
Cell = namedtuple("Cell", "kind code stem next zero")


def _ok(nxt, zero=False):
    return Cell("ok", None, None, nxt, zero)


def _refused(state, stem):
    return Cell("refused", "KSP_E_ARG", stem, state, False)


def _table():
    t = {}
    for s in STATES:
        for c in WHOLE_BUILDS:
            t[s, c] = _ok("whole")            # an accepted whole build forgets a slice at any phase
        for c in SLICE_BUILDS:
            t[s, c] = _ok("labels")
        for c in AT_LABELS:
            t[s, c] = _refused(s, "build_slice has not been run")
        t[s, "slice_sizes"] = _refused(s, "build_slice has not been run")
        t[s, "slice_export"] = _refused(s, "build_slice has not been run")
        t[s, "assemble"] = _refused(s, "build_slice must run on this engine first")
        for c in JOINS:
            t[s, c] = _ok(s) if s in JOINABLE else _refused(s, "build_blocks has not been run")
        t[s, "balanced_cuts"] = _ok(s) if s in JOINABLE else _refused(s, "build_blocks / assemble has not been run")
        t[s, "join_wait"] = _ok(s)            # (nothing pending: a count of 0)
        t[s, "edge_bound"] = _ok(s, zero=s not in JOINABLE)
        t[s, "lists_path"] = _ok(s, zero=s not in JOINABLE)
        t[s, "stats"] = _ok(s)
    for c in ("slice_labels", "slice_bounds", "slice_set_bounds"):
        t["labels", c] = _ok("labels")
    t["labels", "slice_finish"] = _ok("finished")          # (a second slice_finish finds the state `finished`: refused)
    for s in ("finished", "assembled"):
        t[s, "slice_sizes"] = _ok(s)
        t[s, "assemble"] = _ok("assembled")                # (twice over the same stacked buffers: the same lists)
    t["finished", "slice_export"] = _ok("finished")
    t["assembled", "slice_export"] = Cell("unspecified", None, None, "assembled", False)
    return t


TABLE = _table()

# with a launched join uncollected, in the joinable states (elsewhere the state's own refusal comes first)
PENDING = {c: Cell("refused", "KSP_E_ARG", "a launched join is pending", None, False) for c in JOINS}

# ---- the walks ---------------------------------------------------------------------------------------------------------
# name -> has a key that two sources share (a join on the others launches nothing, so nothing becomes pending)
SKETCH_INPUTS = {"n129": True, "n127": True, "one": False, "empty": False, "weighted_low20": True}
POSTINGS_INPUTS = {"post129": True, "post129w": True}      # (n129's shared keys as an inverted index, plain and weighted)
SHARES = dict(SKETCH_INPUTS, **POSTINGS_INPUTS)

WALK_SEEDS = range(12)
WALK_STEPS = 100     # (12 walks of 100 calls: the fewest seeds from 0 on that reach every cell, `assembled` being the rare state)
# the calls that move a protocol forward are drawn more often, or a walk hardly ever gets past `labels`
WEIGHTS = {"slice_finish": 5, "assemble": 5, "build_slice": 2, "build_postings_slice": 2, "join_launch": 2, "join_wait": 2}

# one step of a walk.  inp: the input a build call takes; nparts, part: of a slice build.  pending: the input whose join
# is launched and uncollected before the call; cur: the input whose edges a join gives before the call (joinable states).
Step = namedtuple("Step", "state pending cur call cell inp nparts part")


def cell_of(state, pending, call):
    if pending is not None and state in JOINABLE and call in PENDING:
        return PENDING[call]._replace(next=state)
    return TABLE[state, call]


def walk(seed, steps=WALK_STEPS):
    """The seeded walk: `steps` calls drawn from the table, then a join_wait if a join is still pending."""
    rng = np.random.default_rng(77000 + seed)
    w = np.array([WEIGHTS.get(c, 1) for c in CALLS], dtype=np.float64)
    w /= w.sum()
    state, pending, cur, ctx = "fresh", None, None, None
    out = []
    for _ in range(steps):
        while True:
            call = CALLS[int(rng.choice(len(CALLS), p=w))]
            cell = cell_of(state, pending, call)
            if cell.kind != "unspecified":
                break
        inp = nparts = part = None
        if call in WHOLE_BUILDS or call in SLICE_BUILDS:
            names = sorted(POSTINGS_INPUTS if "postings" in call else SKETCH_INPUTS)
            inp = names[int(rng.integers(len(names)))]
            if call in SLICE_BUILDS:
                nparts = int(rng.integers(1, 4))
                part = int(rng.integers(nparts))
        out.append(Step(state, pending, cur, call, cell, inp, nparts, part))
        if cell.kind == "refused":
            continue
        if call in WHOLE_BUILDS:
            cur, ctx = inp, None
            if call == "step_launch":
                pending = inp if SHARES[inp] else None     # (the pending join is collected by the call, its own launched)
        elif call in SLICE_BUILDS:
            cur, ctx = None, inp
        elif call == "assemble":
            cur = ctx
        elif call == "join_launch":
            pending = cur if SHARES[cur] else None
        elif call == "join_wait":
            pending = None
        state = cell.next
    if pending is not None:
        out.append(Step(state, pending, cur, "join_wait", cell_of(state, pending, "join_wait"), None, None, None))
    return out
