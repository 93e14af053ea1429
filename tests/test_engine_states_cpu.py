"""tests/engine_states.py on its own, without a GPU and without the library: the state table is total and consistent,
and the seeded walks that tests/test_engine_sequences_gpu.py makes on an engine visit every cell of it."""
import engine_states as S


def test_the_table_is_total():
    assert set(S.TABLE) == {(s, c) for s in S.STATES for c in S.CALLS}
    assert len(set(S.CALLS)) == len(S.CALLS)
    for (s, c), cell in S.TABLE.items():
        assert cell.kind in ("ok", "refused", "unspecified"), (s, c)
        assert cell.next in S.STATES, (s, c)
        if cell.kind == "refused":   # a refused call names its code and its message, and changes nothing
            assert cell.next == s and cell.code in ("KSP_E_ARG", "KSP_E_LIMIT", "KSP_E_OVERFLOW") and cell.stem, (s, c)
        else:
            assert cell.code is None and cell.stem is None, (s, c)
        assert not cell.zero or cell.kind == "ok", (s, c)
    assert set(S.PENDING) == set(S.JOINS)


def test_what_the_state_flags_decide():
    """The rows that the issue behind the table names, read off the table."""
    t = S.TABLE
    for s in S.STATES:
        for c in S.WHOLE_BUILDS:
            assert t[s, c].kind == "ok" and t[s, c].next == "whole"          # a whole build is accepted anywhere ...
        for c in S.AT_LABELS + S.AT_READY:
            assert t["whole", c].kind == "refused"                           # ... and forgets a slice at any phase
        for c in S.JOINS + ("balanced_cuts",):
            assert (t[s, c].kind == "ok") == (s in S.JOINABLE)               # not joinable until assembled
        assert t[s, "edge_bound"].zero == t[s, "lists_path"].zero == (s not in S.JOINABLE)
    assert t["finished", "slice_finish"].kind == "refused"                   # slice_finish twice
    assert t["labels", "slice_sizes"].kind == t["labels", "slice_export"].kind == "refused"   # the next slice, unfinished
    assert t["assembled", "assemble"].kind == "ok"                           # assemble twice
    assert [k for k, cell in t.items() if cell.kind == "unspecified"] == [("assembled", "slice_export")]


def test_the_walks_visit_every_cell_and_leave_no_join_pending():
    seen = set()
    for seed in S.WALK_SEEDS:
        steps = S.walk(seed)
        assert steps == S.walk(seed)                       # (a walk is a function of its seed)
        assert len(steps) in (S.WALK_STEPS, S.WALK_STEPS + 1)
        state, pending = "fresh", None
        for st in steps:
            assert (st.state, st.pending) == (state, pending), (seed, st)
            assert st.cell == S.cell_of(state, pending, st.call) and st.cell.kind != "unspecified", (seed, st)
            assert (st.inp is not None) == (st.call in S.WHOLE_BUILDS + S.SLICE_BUILDS), (seed, st)
            if st.call in S.SLICE_BUILDS:
                assert 1 <= st.nparts <= 3 and 0 <= st.part < st.nparts, (seed, st)
            if st.inp is not None:
                assert st.inp in (S.POSTINGS_INPUTS if "postings" in st.call else S.SKETCH_INPUTS), (seed, st)
            if st.state in S.JOINABLE:
                assert st.cur is not None, (seed, st)
            seen.add((st.state, st.pending is not None and st.state in S.JOINABLE and st.call in S.PENDING, st.call))
            if st.cell.kind == "ok":
                state = st.cell.next
                if st.call == "join_wait":
                    pending = None
                elif st.call == "step_launch":
                    pending = st.inp if S.SHARES[st.inp] else None
                elif st.call == "join_launch":
                    pending = st.cur if S.SHARES[st.cur] else None
        assert pending is None, seed                       # no walk ends with a launched join uncollected
    want = {(s, False, c) for (s, c), cell in S.TABLE.items() if cell.kind != "unspecified"}
    want |= {(s, True, c) for s in S.JOINABLE for c in S.PENDING}
    assert want - seen == set(), sorted(want - seen)
    assert seen - want == set(), sorted(seen - want)
