"""acm_scan_graph_stats without a device: the argument contract (the counters themselves are checked where
graphs run, tests/test_gpu_streams.py)."""
import ctypes as C

from gpu_pattern_matching_amd import _lib


def test_null_dfa_is_an_argument_error(lib):
    captured, launched = C.c_uint64(7), C.c_uint64(9)
    assert lib.acm_scan_graph_stats(None, C.byref(captured), C.byref(launched)) == -1      # ACM_ERR_ARG
    assert b"acm_scan_graph_stats" in lib.acm_last_error()
    assert (captured.value, launched.value) == (7, 9)                                      # nothing written
    assert lib.acm_scan_graph_stats(None, None, None) == -1


def test_binding_matches_the_header(lib):
    res, args = _lib.NATIVE_API["acm_scan_graph_stats"]
    assert res is C.c_int and len(args) == 3
