"""Every C entry point that takes a `device` refuses one that is not there — ksp_device_count() and -1 — with KSP_E_HIP and
"<entry point>: no such device", before it touches a device: the name in the message is what the entry point hands to the one
shared device check (kspider_amd/csrc/device_call.h).  Every call is otherwise valid, on the smallest input that is not empty
(2 nodes, 1 edge; device buffers live on device 0), and no kernel is launched.  A valid ksp_edges_cut on device 0 afterwards
must still return the right records: the refusals left nothing behind."""
import ctypes

import numpy as np
import pytest

from kspider_amd import engine

pytestmark = pytest.mark.gpu

KSP_E_HIP = 2


@pytest.fixture(scope="module")
def inputs():
    edges = np.zeros(1, dtype=engine.EDGE_DTYPE)
    edges["source_1"], edges["source_2"], edges["shared"] = 0, 1, 6      # containment 6/10 and 6/8
    bufs = {
        "edges": engine.DeviceBuffer.from_numpy(edges),
        "counts": engine.DeviceBuffer.from_numpy(np.array([10, 8], dtype=np.uint32)),
        "rows": engine.DeviceBuffer.from_numpy(np.array([[0.0, 0.25], [0.25, 0.0]])),
        "out": engine.DeviceBuffer(64),
    }
    yield edges, bufs
    for b in bufs.values():
        b.free()


def _calls(L, bufs):
    """name -> call(device): each entry point with valid arguments for the 2-node, 1-edge input."""
    ed, cnt, rows, out = (bufs[k].ptr for k in ("edges", "counts", "rows", "out"))
    a, b = np.array([0], dtype=np.uint32), np.array([1], dtype=np.uint32)
    one = np.array([1], dtype=np.uint32)
    level = np.array([1], dtype=np.uint8)
    cutoffs = np.array([0.5])
    h = [np.zeros(8, dtype=np.uint64) for _ in range(4)]                  # host outputs, larger than any call needs
    p = [x.ctypes.data for x in h]
    n32, n64 = ctypes.c_uint32(0), ctypes.c_uint64(0)
    L.ksp_components_edges.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_void_p]
    return {
        "ksp_components": lambda d: L.ksp_components(d, 2, a.ctypes.data, b.ctypes.data, 1, p[0]),
        "ksp_components_edges": lambda d: L.ksp_components_edges(d, 2, ed, 1, cnt, 5, 0.5, p[0]),
        "ksp_components_edges_ani": lambda d: L.ksp_components_edges_ani(d, 2, ed, 1, cnt, 31, 0.5, p[0]),
        "ksp_edges_ani": lambda d: L.ksp_edges_ani(d, ed, 1, cnt, 31, out),
        "ksp_single_linkage_rows": lambda d: L.ksp_single_linkage_rows(d, 2, rows, p[0]),
        "ksp_single_linkage_prim": lambda d: L.ksp_single_linkage_prim(d, 2, rows, p[0]),
        "ksp_row_distances": lambda d: L.ksp_row_distances(d, 2, rows, p[0]),
        "ksp_edges_degrees": lambda d: L.ksp_edges_degrees(d, 2, ed, 1, cnt, 4, 0.2, p[0]),
        "ksp_edges_repr": lambda d: L.ksp_edges_repr(d, 2, ed, 1, cnt, 4, 0.2, p[0], p[1], ctypes.byref(n32)),
        "ksp_edges_cut": lambda d: L.ksp_edges_cut(d, ed, 1, cnt, 5, 0.5, out, ctypes.byref(n64)),
        "ksp_components_edges_sweep": lambda d: L.ksp_components_edges_sweep(d, 2, ed, 1, cnt, 5, cutoffs.ctypes.data, 1, p[0], p[1]),
        "ksp_components_sweep": lambda d: L.ksp_components_sweep(d, 2, a.ctypes.data, b.ctypes.data, level.ctypes.data, 1, 1, p[0]),
        "ksp_edges_forest": lambda d: L.ksp_edges_forest(d, 2, ed, 1, cnt, 5, p[0], ctypes.byref(n32)),
        "ksp_forest_ranked": lambda d: L.ksp_forest_ranked(d, 2, a.ctypes.data, b.ctypes.data, one.ctypes.data, 1, p[0], ctypes.byref(n32)),
        "ksp_edges_dereplicate": lambda d: L.ksp_edges_dereplicate(d, 2, ed, 1, cnt, 4, 0.2, p[0], p[1], p[2], p[3], ctypes.byref(n32)),
    }


ENTRY_POINTS = ("ksp_components", "ksp_components_edges", "ksp_components_edges_ani", "ksp_edges_ani", "ksp_single_linkage_rows",
                "ksp_single_linkage_prim", "ksp_row_distances", "ksp_edges_degrees", "ksp_edges_repr", "ksp_edges_cut",
                "ksp_components_edges_sweep", "ksp_components_sweep", "ksp_edges_forest", "ksp_forest_ranked", "ksp_edges_dereplicate")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_a_device_that_is_not_there_is_refused_by_name(inputs, name):
    L = engine.lib()
    call = _calls(L, inputs[1])[name]
    for device in (engine.device_count(), -1):
        assert call(device) == KSP_E_HIP, (name, device)
        assert L.ksp_last_error().decode() == name + ": no such device", (name, device)


def test_a_valid_cut_after_the_refusals(inputs):
    edges, bufs = inputs
    L = engine.lib()
    for name, call in _calls(L, bufs).items():                            # all of them again, in one process state
        assert call(engine.device_count()) == KSP_E_HIP and call(-1) == KSP_E_HIP, name
    out = engine.DeviceBuffer.from_numpy(np.zeros(2, dtype=engine.EDGE_DTYPE))
    try:
        # max containment 6/8 = 0.75: kept at 0.5, cut at 0.8
        assert engine.edges_cut(bufs["edges"].ptr.value, 1, bufs["counts"].ptr.value, out.ptr.value, 5, 0.5) == 1
        got = out.to_numpy(engine.EDGE_DTYPE, 2)
        assert (got[:1] == edges).all() and (got[1:] == np.zeros(1, dtype=engine.EDGE_DTYPE)).all()
        assert engine.edges_cut(bufs["edges"].ptr.value, 1, bufs["counts"].ptr.value, out.ptr.value, 5, 0.8) == 0
    finally:
        out.free()
