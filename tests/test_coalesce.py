"""smartgpu_coalesce and smartgpu_coalesce_stats without a device: the setting's range and the product library's exports."""
import ctypes

from smart_amd import engine


def test_coalesce_accepts_0_and_2_to_8_and_returns_the_previous_value():
    L = engine.lib()
    default = L.smartgpu_coalesce(0)
    try:
        assert default == 0 or 2 <= default <= 8
        prev = 0
        for g in (2, 3, 4, 5, 6, 7, 8, 0, 8):
            assert L.smartgpu_coalesce(g) == prev
            prev = g
        for bad in (1, 9, -1):
            assert L.smartgpu_coalesce(bad) < 0
            assert b"coalesce" in L.smartgpu_last_error()
        assert L.smartgpu_coalesce(8) == 8  # a refused value changed nothing
    finally:
        L.smartgpu_coalesce(default)


def test_product_library_exports_the_coalesce_calls():
    L = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(L, "smartgpu_coalesce") and hasattr(L, "smartgpu_coalesce_stats")
    launches, passes = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert engine.lib().smartgpu_coalesce_stats(0, ctypes.byref(launches), ctypes.byref(passes)) == 0
    assert passes.value <= launches.value
    assert engine.lib().smartgpu_coalesce_stats(-1, None, None) < 0
