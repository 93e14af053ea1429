"""Engine.step_launch's own bookkeeping, against a stub of the library: which join the wrapper believes to be in flight,
what it returns and what it raises for every (rc, prev_status) the C call can give.  No GPU: the stub stands in for
ksp_engine_step_launch and writes the out-parameters a real call would."""
import numpy as np
import pytest

from kspider_amd import engine


class _Fn:
    """A stub entry point that, like a ctypes function, takes .argtypes / .restype."""

    def __init__(self, f):
        self.f = f

    def __call__(self, *a):
        return self.f(*a)


class _StubLib:
    """The handful of entry points Engine.__init__ / step_launch / join_launch / join_wait call."""

    def __init__(self):
        self.script = []      # (rc, prev_status, prev_count) per step_launch call
        self.calls = []
        self.engines = []
        for name in dir(self):
            if name.startswith("ksp_"):
                setattr(self, name, _Fn(getattr(self, name)))

    def ksp_engine_create(self, device, out):
        out._obj.value = 0x1234
        return engine.KSP_OK

    def ksp_engine_destroy(self, h):
        pass

    def ksp_last_error(self):
        return b"stub error"

    def ksp_engine_join_launch(self, h, t0, t1, d_edges, capacity, stream):
        self.calls.append(("join_launch", t0, t1))
        return engine.KSP_OK

    def ksp_engine_join_wait(self, h, cnt):
        self.calls.append(("join_wait",))
        cnt._obj.value = 5
        return engine.KSP_OK

    def ksp_engine_step_launch(self, h, d_keys, d_weights, h_offsets, n_sources, key_bits, part, nparts, d_edges, capacity,
                               rng, bound, prev, prev_rc, prev_ms, stream):
        rc, prev_status, prev_count = self.script.pop(0)
        self.calls.append(("step_launch", d_weights, key_bits, n_sources, part, nparts, stream))
        if rc in (engine.KSP_OK, engine.KSP_E_OVERFLOW):
            rng[0], rng[1] = 3, 9
            bound._obj.value = 77
            prev._obj.value = prev_count
            prev_rc._obj.value = prev_status
            prev_ms._obj.value = 1.5
        return rc


@pytest.fixture
def stub(monkeypatch):
    s = _StubLib()
    monkeypatch.setattr(engine, "lib", lambda: s)
    yield s
    for e in s.engines:     # (closed while the stub is in place: the real library must never see the stub's handle)
        e.close()


def _engine(stub):
    e = engine.Engine(0)
    stub.engines.append(e)
    return e


OFF = np.array([0, 2, 4], dtype=np.uint64)


def _step(e, **kw):
    return e.step_launch(0x1000, OFF, 0, 1, 0x2000, 100, **kw)


def test_first_step_has_no_previous_count(stub):
    e = _engine(stub)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0)]
    assert _step(e) == (3, 9, 77, True, None)
    assert e._join_in_flight
    # defaults: no weights, key_bits 0, default stream
    assert stub.calls[-1] == ("step_launch", None, 0, 2, 0, 1, None)


def test_weights_key_bits_and_stream_reach_the_library(stub):
    e = _engine(stub)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0)]
    _step(e, d_weights_ptr=0x3000, key_bits=41, stream=0x4000)
    assert stub.calls[-1] == ("step_launch", 0x3000, 41, 2, 0, 1, 0x4000)


def test_chain_collects_the_previous_count(stub):
    e = _engine(stub)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0), (engine.KSP_OK, engine.KSP_OK, 11), (engine.KSP_E_OVERFLOW, engine.KSP_OK, 12)]
    assert _step(e)[4] is None
    assert _step(e) == (3, 9, 77, True, 11)
    # over the bound: nothing launched, the previous count still delivered, no join in flight afterwards
    assert _step(e) == (3, 9, 77, False, 12)
    assert not e._join_in_flight
    assert e.prev_ms_join == 1.5
    # the next step has nothing to collect
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0)]
    assert _step(e)[4] is None


def test_failed_previous_join_keeps_the_new_step(stub):
    """The previous join overflowed its buffer; the new step was built and launched all the same: the exception says so
    and carries the new step, and the wrapper knows the new join is in flight."""
    e = _engine(stub)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0), (engine.KSP_OK, engine.KSP_E_OVERFLOW, 500)]
    _step(e)
    with pytest.raises(engine.PrevJoinError) as ei:
        _step(e)
    assert ei.value.code == engine.KSP_E_OVERFLOW
    assert isinstance(ei.value, engine.KspError)
    assert ei.value.step == (3, 9, 77, True, 500)
    assert e._join_in_flight
    # the next step collects the new join (it is not lost)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 7)]
    assert _step(e)[4] == 7


def test_failed_previous_join_and_new_step_over_the_bound(stub):
    e = _engine(stub)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0), (engine.KSP_E_OVERFLOW, engine.KSP_E_OVERFLOW, 500)]
    _step(e)
    with pytest.raises(engine.PrevJoinError) as ei:
        _step(e)
    assert ei.value.step == (3, 9, 77, False, 500)
    assert not e._join_in_flight


@pytest.mark.parametrize("rc", [engine.KSP_E_ARG, engine.KSP_E_LIMIT])
def test_refused_step_leaves_the_pending_join_pending(stub, rc):
    """A refused call changes nothing in the engine: the join launched before it is still to be collected."""
    e = _engine(stub)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0), (rc, engine.KSP_OK, 0), (engine.KSP_OK, engine.KSP_OK, 21)]
    _step(e)
    with pytest.raises(engine.KspError) as ei:
        _step(e)
    assert ei.value.code == rc and not isinstance(ei.value, engine.PrevJoinError)
    assert e._join_in_flight
    assert _step(e)[4] == 21          # ... and the next step reports its count
    # without a join in flight a refused call leaves none behind
    e2 = _engine(stub)
    stub.script = [(rc, engine.KSP_OK, 0)]
    with pytest.raises(engine.KspError):
        _step(e2)
    assert not getattr(e2, "_join_in_flight", False)


def test_device_failure_clears_the_join_in_flight(stub):
    e = _engine(stub)
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0), (engine.KSP_E_HIP, engine.KSP_OK, 0)]
    _step(e)
    with pytest.raises(engine.KspError) as ei:
        _step(e)
    assert ei.value.code == engine.KSP_E_HIP
    assert not e._join_in_flight


def test_join_launch_and_wait_track_the_join(stub):
    e = _engine(stub)
    e.join_launch(0, 4, 0x2000, 10)
    assert e._join_in_flight
    assert e.join_wait() == 5
    assert not e._join_in_flight
    stub.script = [(engine.KSP_OK, engine.KSP_OK, 0)]
    assert _step(e)[4] is None
