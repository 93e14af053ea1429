"""ksp_engine_lists_path without a device: the getter is exported, bound, and refuses NULL arguments."""
import ctypes

from kspider_amd import engine


def test_lists_path_refuses_null_arguments():
    lib = engine.lib()
    out = ctypes.c_int(-7)
    assert lib.ksp_engine_lists_path(None, ctypes.byref(out)) == engine.KSP_E_ARG
    assert out.value == -7   # (nothing was written)
    assert b"lists_path" in lib.ksp_last_error()
    assert lib.ksp_engine_lists_path(None, None) == engine.KSP_E_ARG


def test_lists_path_values_and_abi_listing():
    assert "ksp_engine_lists_path" in engine.ABI_SYMBOLS
    assert (engine.LISTS_NONE, engine.LISTS_KEYED, engine.LISTS_COMPACTED, engine.LISTS_SORTED, engine.LISTS_FUSED) == (0, 1, 2, 3, 4)
    assert callable(engine.Engine.lists_path)


def test_no_gpu_stub_refuses_the_getter():
    """The host-only sanitizer build has no engine: its lists_path answers KSP_E_HIP like every compute entry."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kspider_amd", "csrc", "host_nogpu_stub.cpp")).read()
    body = src.split("int ksp_engine_lists_path(const ksp_engine*, int*) {", 1)[1].split("}", 1)[0]
    assert "KSP_E_HIP" in body and "set_error" in body
