"""Guarded device buffers for the post-processing ops (a test helper, not a conftest), in the style of
tests/test_gpu_lines.py: every buffer an op gets has G guard cells on each side and is filled with a
poison byte before the call, so "nothing outside", "every defined cell written" and "every other cell
left alone" are checked by each download.

  Guarded    cells of `itemsize` bytes between two guards; ptr is the first cell; read() asserts the
             guards and returns the cells
  Workspace  nbytes filled with one of poison.FILLS' bytes and 256 bytes behind them that must stay
"""
import numpy as np

import poison
from gpu_pattern_matching_amd import DeviceArray
from gpu_pattern_matching_amd._lib import check

G = 64
FILL = 0x5A
FILL32 = poison.cell(FILL)
WS_FILLS = tuple(f for f in poison.FILLS if f != "stale")


class Guarded:
    def __init__(self, cells, host=None, fill=FILL, dtype=np.int32):
        """host: what the cells hold (an input, or the data of an in-place call); else they hold the fill"""
        self.dtype = np.dtype(dtype)
        self.cells, self.fill = int(cells), fill
        self.guard = G * self.dtype.itemsize
        self.buf = DeviceArray(self.cells * self.dtype.itemsize + 2 * self.guard)
        self.buf.fill(fill)
        self.ptr = self.buf.ptr + self.guard
        if host is not None:
            host = np.ascontiguousarray(host, dtype=self.dtype)
            assert host.size <= self.cells
            if host.nbytes:
                check(self.buf.lib.acm_rt_memcpy_h2d(self.ptr, host.ctypes.data, host.nbytes, None), "acm_rt_memcpy_h2d")
        check(self.buf.lib.acm_rt_stream_sync(None), "acm_rt_stream_sync")   # (the fill ran on the NULL stream)

    def at(self, cell):
        return self.ptr + cell * self.dtype.itemsize

    def read(self, stream=None, what=""):
        a = self.buf.to_numpy(self.dtype, self.cells + 2 * G, stream=stream)
        v = np.frombuffer(bytes([self.fill]) * self.dtype.itemsize, dtype=self.dtype)[0]
        assert np.all(a[:G] == v), "%s: a guard cell in front of the buffer was written" % what
        assert np.all(a[G + self.cells:] == v), "%s: a guard cell behind the buffer was written" % what
        return a[G:G + self.cells].copy()

    def untouched(self, stream=None, what=""):
        a = self.read(stream, what)
        v = np.frombuffer(bytes([self.fill]) * self.dtype.itemsize, dtype=self.dtype)[0]
        assert np.all(a == v), "%s: cell %d was written" % (what, int(np.flatnonzero(a != v)[0]))

    def free(self):
        self.buf.free()


class Workspace:
    TAIL = 256

    def __init__(self, nbytes, fill=0xFF):
        self.nbytes, self.fill = int(nbytes), fill
        self.buf = DeviceArray(self.nbytes + self.TAIL)
        self.buf.fill(fill)
        check(self.buf.lib.acm_rt_stream_sync(None), "acm_rt_stream_sync")
        self.ptr = self.buf.ptr

    def check(self, stream=None, what=""):
        tail = self.buf.to_numpy(np.uint8, self.TAIL, offset_bytes=self.nbytes, stream=stream)
        assert np.all(tail == self.fill), "%s: a byte behind the workspace was written" % what

    def free(self):
        self.buf.free()


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, "%s: %d cells, expected %d" % (what, got.size, exp.size)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: cell %d = %d, expected %d (%d cells differ)" % (
        what, bad[0], got[bad[0]], exp[bad[0]], bad.size)
