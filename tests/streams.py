"""Streams, events and per-batch buffers for tests that run scans the way callers do (a test helper,
not a conftest): on streams made by acm_rt_stream_create -- non-blocking, so nothing orders them against
the NULL stream or against each other but what the test enqueues -- with every batch owning its text,
workspace and planes.

  Rig      makes streams, events and device buffers and destroys them all in close(), after a device sync
  Triple   one batch's text, workspace and planes; poison() fills the planes with poison.PLANE_POISON on
           the stream the scan will run on, check() compares them whole with the oracle's records
           (poison.check_planes: count cell, records, trailer, poison behind the trailer)
  words    the word pass in Python for a variants.VariantSet (word_model.bounded_mask on the oracle's
           all-patterns records)

Uploads made on the NULL stream are synchronised before they return (DeviceArray.from_numpy); downloads
go through the stream the scan ran on.
"""
import ctypes as C

import numpy as np

import poison
import word_model as wm
from gpu_pattern_matching_amd import DeviceArray, _lib
from gpu_pattern_matching_amd._lib import check

EE = poison.PLANE_POISON
HALF = frozenset(range(0, 256, 2))      # a word set that splits any alphabet: the even bytes


class Rig:
    def __init__(self):
        self.lib = _lib.load()
        self.streams, self.events, self.bufs = [], [], []

    def stream(self):
        s = C.c_void_p()
        check(self.lib.acm_rt_stream_create(C.byref(s)), "acm_rt_stream_create")
        assert s.value, "acm_rt_stream_create gave the NULL stream"
        self.streams.append(s.value)
        return s.value

    def event(self):
        e = C.c_void_p()
        check(self.lib.acm_rt_event_create(C.byref(e)), "acm_rt_event_create")
        self.events.append(e.value)
        return e.value

    def record(self, event, stream):
        check(self.lib.acm_rt_event_record(event, stream), "acm_rt_event_record")
        return event

    def elapsed(self, start, stop):
        """(status, milliseconds) of acm_rt_event_elapsed_ms: the status is not ACM_OK when either event
        was never recorded (or has not completed)"""
        ms = C.c_float(-1.0)
        return self.lib.acm_rt_event_elapsed_ms(start, stop, C.byref(ms)), ms.value

    def sync(self, stream):
        check(self.lib.acm_rt_stream_sync(stream), "acm_rt_stream_sync")

    def buf(self, nbytes, fill=None):
        b = DeviceArray(max(int(nbytes), 16))
        self.bufs.append(b)
        if fill is not None:
            b.fill(fill)
            self.sync(None)
        return b

    def upload(self, a, pad_to=16):
        b = DeviceArray.from_numpy(a, pad_to=pad_to)
        self.bufs.append(b)
        return b

    def planes(self, cap):
        return self.buf(cap * 4, EE), self.buf(cap * 4, EE)

    def triple(self, m, text, room=None, cap=None):
        return Triple(self, m, text, room, cap)

    def h2d(self, dst, host, stream):
        """host -> device on stream; the caller keeps host alive until the stream is synchronised"""
        check(self.lib.acm_rt_memcpy_h2d(dst.ptr if isinstance(dst, DeviceArray) else dst, host.ctypes.data,
                                         host.nbytes, stream), "acm_rt_memcpy_h2d")

    def d2d(self, dst, src, nbytes, stream):
        check(self.lib.acm_rt_memcpy_d2d(dst.ptr if isinstance(dst, DeviceArray) else dst,
                                         src.ptr if isinstance(src, DeviceArray) else src, nbytes, stream),
              "acm_rt_memcpy_d2d")

    def close(self):
        self.lib.acm_rt_device_sync()
        for e in self.events:
            self.lib.acm_rt_event_destroy(e)
        for s in self.streams:
            self.lib.acm_rt_stream_destroy(s)
        for b in self.bufs:
            b.free()
        self.streams, self.events, self.bufs = [], [], []


class Triple:
    """text (room bytes and the ABI's pad, zero behind the text), workspace for room bytes, planes of cap cells"""

    def __init__(self, rig, m, text, room=None, cap=None):
        self.rig, self.m = rig, m
        self.t = np.ascontiguousarray(text, dtype=np.uint8)
        self.n = self.t.size
        self.room = max(self.n, room or 0, 1)
        host = np.zeros(poison.round16(self.room) + 16, dtype=np.uint8)
        host[:self.n] = self.t
        self.text = rig.upload(host)
        self.wsb = m.lib.acm_scan_workspace_bytes(m.dfa, self.room)
        self.ws = rig.buf(self.wsb)
        self.cap = cap if cap is not None else self.room + 2
        self.pat, self.off = rig.planes(self.cap)

    @property
    def workspace(self):
        return (self.ws.ptr, self.wsb)

    def poison(self, stream):
        self.pat.fill(EE, stream)
        self.off.fill(EE, stream)

    def set_text(self, text, stream):
        """another text of at most room bytes, copied in on stream (stream order alone protects the reuse)"""
        self.t = np.ascontiguousarray(text, dtype=np.uint8)
        assert self.t.size <= self.room
        self.n = self.t.size
        self.rig.h2d(self.text, self.t, stream)

    def batch(self, stream, wait=None, record=None, **kw):
        b = self.m.make_batch(self.text, self.n, stream, self.pat, self.off, self.cap, self.workspace, **kw)
        b.wait_before_walk = wait
        b.record_after_walk = record
        return b

    def check(self, exp, stream, what="", pat_cells=True):
        poison.check_planes(self.pat, self.off, self.cap, exp, what=what, pat_cells=pat_cells, stream=stream)

    def path(self, stream):
        return self.m.path_taken(self.n, stream=stream, workspace=self.workspace)


def oracle_all(o, t, init=0):
    cap = 4 * t.size // 16 + 4096
    while True:
        try:
            return o.scan_all(t, init, cap=cap)
        except OverflowError:
            cap *= 4


def words(o, vs, t, init=0, all_patterns=True, word_set=HALF):
    """(offsets, patterns, final state) of the word pass over the scan of t: the oracle's all-patterns
    records whose pattern is word-bounded in the raw text (word_model.bounded_mask); head form: the first
    such pattern per offset"""
    offs, pats, last = oracle_all(o, vs.text_of(t), init)
    lens = np.array([len(p) for p in vs.patterns], dtype=np.int64)
    ok = wm.bounded_mask(t, offs, lens[pats] if pats.size else np.zeros(0, np.int64), word_set)
    offs, pats = offs[ok], pats[ok]
    if not all_patterns and offs.size:
        first = np.concatenate([[True], offs[1:] != offs[:-1]])
        offs, pats = offs[first], pats[first]
    return offs, pats, last
