"""Normalised scanning on the device (acm_normalize_async, acm_normalize_remap_async, Matcher.scan_normalized), byte
for byte and cell for cell against the serial model of tests/normalize_model.py.  Every output lies between guard
bands and is poisoned before the call; the text is followed by poison that is made of hex digits (it would complete a
trailing "%4"); the workspace is exactly of the queried size and poisoned."""
import ctypes as C

import numpy as np
import pytest

import normalize_model as nm
import ops_guard as og
import orc
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib
from gpu_pattern_matching_amd._lib import check
from normalize_model import PERCENT, SQUEEZE, STRIP

pytestmark = pytest.mark.gpu

INT32_MAX = 0x7FFFFFFF
PAST = 4096
TILE = 16384
ALPHABET = b"%%%%0123456789abcdefABCDEF \t\n\v\f\r\x00gG+zZ"
MODES = [0, PERCENT, SQUEEZE, STRIP, PERCENT | SQUEEZE, PERCENT | STRIP]
BOUNDS = (16, 64, 1024, TILE, 2 * TILE)


def mode_id(f):
    return "+".join(n for b, n in ((PERCENT, "percent"), (SQUEEZE, "squeeze"), (STRIP, "strip")) if f & b) or "none"


def random_text(n, seed, alphabet=ALPHABET):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].copy()


def upload_text(text):
    t = np.asarray(text, dtype=np.uint8)
    h = np.tile(np.frombuffer(b"1A", dtype=np.uint8), (((t.size + 15) & ~15) + PAST) // 2)
    h[:t.size] = t
    return DeviceArray.from_numpy(h)


@pytest.fixture(scope="module", autouse=True)
def needs_gpu(gpu):
    return gpu


class Call:
    """one call from poisoned outputs; read() checks the guard bands"""

    def __init__(self, lib, d_text, n, flags, cap, origin=0, blank_mask=None, blank_byte=0x20, seg_start=None, with_out=True,
                 ws_fill=0xFF, stream=None):
        nseg = 0 if seg_start is None else len(seg_start)
        self.out = og.Guarded(cap if with_out else 16, dtype=np.uint8)
        self.keep = og.Guarded((n + 63) // 64, dtype=np.uint64)
        self.block = og.Guarded((n + nm.BLOCK - 1) // nm.BLOCK + 1)
        self.seg_in = og.Guarded(nseg, host=np.asarray(seg_start, dtype=np.int32)) if nseg else None
        self.seg = og.Guarded(nseg) if nseg else None
        self.info = og.Guarded(8)
        nb = lib.acm_normalize_workspace_bytes(n, nseg)
        assert nb % 256 == 0 and nb > 0
        self.ws = og.Workspace(nb, ws_fill)
        check(lib.acm_normalize_async(d_text.ptr, n, origin, flags, blank_mask, blank_byte, self.out.ptr if with_out else None,
                                      cap if with_out else 0, self.keep.ptr, self.block.ptr, self.seg_in.ptr if nseg else None,
                                      nseg, self.seg.ptr if nseg else None, self.info.ptr, self.ws.ptr, nb, stream),
              "acm_normalize_async")
        self.stream = stream

    def read(self, what=""):
        st = self.stream
        self.ws.check(st, what)
        res = dict(out=self.out.read(st, what), keep=self.keep.read(st, what), block=self.block.read(st, what),
                   info=self.info.read(st, what), seg=self.seg.read(st, what) if self.seg else None)
        if self.seg_in:
            self.seg_in.read(st, what)
        for x in (self.out, self.keep, self.block, self.seg_in, self.seg, self.info, self.ws):
            if x is not None:
                x.free()
        return res


def run(lib, text, flags, cap=None, origin=0, blanks=None, blank_byte=0x20, seg_start=None, with_out=True, what="",
        d_text=None):
    """one call compared whole with the model; returns the model's result"""
    text = np.asarray(text, dtype=np.uint8)
    x = nm.normalize(text.tobytes(), flags, blanks, blank_byte, origin, seg_start)
    cap = x.m + 37 if cap is None else cap
    x.info[4] = int(with_out and x.m > cap)
    dt = d_text if d_text is not None else upload_text(text)
    mask = nm.blank_mask(blanks) if blanks is not None else None
    got = Call(lib, dt, text.size, flags, cap, origin, mask, blank_byte, seg_start, with_out).read(what)
    what = "%s %s n=%d cap=%d origin=%d" % (what, mode_id(flags), text.size, cap, origin)
    assert got["info"].tolist() == x.info, "%s: info %s, model %s" % (what, got["info"].tolist(), x.info)
    og.same(got["keep"], x.keep_words, what + ": keep words")
    og.same(got["block"], x.block, what + ": block cells")
    if with_out:
        k = min(x.m, cap)
        og.same(got["out"][:k], np.frombuffer(x.out[:k], dtype=np.uint8), what + ": output")
        assert (got["out"][k:] == og.FILL).all(), "%s: a byte at or behind min(m, capacity) = %d was written" % (what, k)
    else:
        assert (got["out"] == og.FILL).all()
    if seg_start is not None:
        og.same(got["seg"], x.seg_out, what + ": seg_out")
    if d_text is None:
        dt.free()
    return x


# ------------------------------------------------------------------ 1. text lengths


@pytest.mark.parametrize("flags", MODES, ids=mode_id)
def test_text_lengths(lib, flags):
    for n in (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 5):
        text = random_text(n, 10 * n + flags)
        run(lib, text, flags, what="lengths")
        run(lib, text, flags, seg_start=[0, n // 3, n // 3, n - n // 4, n, n + 5], what="lengths, texts")


# ------------------------------------------------------------------ 2. triples and blank runs on the boundaries


def boundary_texts(seed):
    """(name, text, starts): structures laid over random adversarial text at every boundary a kernel has"""
    n = 2 * TILE + 300
    out = []
    for shift in (-3, -2, -1, 0):                                     # a triple at every alignment across each boundary
        t = random_text(n, seed + 3 + shift)
        for b in BOUNDS:
            t[b + shift:b + shift + 3] = np.frombuffer(b"%20" if b % 32 else b"%4a", dtype=np.uint8)
            t[b + shift - 1] = 0x78
        out.append(("triple at boundary %+d" % shift, t, None))
    for k in (1, 2, 5, 70):                                           # a blank run that ends, then one that begins, on each
        for side in (0, 1):
            t = random_text(n, seed + 10 * k + side)
            for b in BOUNDS:
                lo, hi = (b - k, b) if side == 0 else (b, b + k)
                if lo < 1:
                    continue
                t[lo:hi] = np.frombuffer(b" \t\n\r", dtype=np.uint8)[np.arange(hi - lo) % 4]
                t[lo - 1] = t[hi] = 0x78
            out.append(("run of %d %s boundary" % (k, "in front of" if side == 0 else "behind"), t, None))
    t = random_text(3 * TILE + 100, seed + 99)                        # a run longer than two tiles, a %20 and a %09 in it
    t[50:50 + 2 * TILE + 500] = 0x20
    t[TILE + 7:TILE + 10] = np.frombuffer(b"%20", dtype=np.uint8)
    t[2 * TILE - 1:2 * TILE + 2] = np.frombuffer(b"%09", dtype=np.uint8)
    out.append(("long run", t, [0, 60, TILE, 2 * TILE + 1]))
    # text starts inside triples and runs: a triple across a start stays literal, a run across one emits twice
    t = random_text(n, seed + 7)
    starts = []
    for j, b in enumerate(BOUNDS):
        t[b - 8:b - 5] = np.frombuffer(b"%41", dtype=np.uint8)
        starts.append(b - 8 + 1 + j % 2)                              # at the first digit, at the second
        t[b + 3:b + 9] = 0x20
        starts.append(b + 5)
        starts.append(b)
    out.append(("starts in triples and runs", t, sorted(starts)))
    return out


@pytest.mark.parametrize("flags", MODES, ids=mode_id)
def test_boundaries(lib, flags):
    for name, t, starts in boundary_texts(1000 * flags):
        x = run(lib, t, flags, seg_start=starts, what=name)
        if name == "long run" and flags & SQUEEZE:
            assert x.info[3] >= 4                                   # one blank a text at the least
    # a run across a text start emits twice; a triple across one stays
    x = run(lib, np.frombuffer(b"a   " + b"   b%4" + b"1", dtype=np.uint8), flags, seg_start=[0, 4, 10], what="twice")
    if flags & SQUEEZE:
        assert x.out == b"a  b%41"
    if flags == PERCENT:
        assert x.out == b"a      b%41" and x.info[2] == 0


@pytest.mark.parametrize("flags", MODES, ids=mode_id)
def test_ends_of_the_text(lib, flags):
    """%, %4, %4g, %%41, %2541 at the end of the text (the poison behind n would complete the first two), with the end
    on, in front of and behind a 16-byte and a 64-byte boundary"""
    for tail in (b"%", b"%4", b"%4g", b"%%41", b"%2541", b"%41", b" ", b"  ", b"%20", b" %20"):
        for n in (len(tail), 16, 17, 18, 19, 64, 65, 66, 1024, 1025, 1026):
            if n < len(tail):
                continue
            t = np.full(n, 0x78, dtype=np.uint8)
            t[n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
            x = run(lib, t, flags, what="tail %r" % tail)
            if flags == PERCENT and tail in (b"%", b"%4", b"%4g"):
                assert x.out == t.tobytes()
            # the same tail at the end of a text that another follows
            run(lib, np.concatenate([t, np.frombuffer(b"1Ab ", dtype=np.uint8)]), flags, seg_start=[0, n], what="tail, then a text")


# ------------------------------------------------------------------ 3. whole texts


def test_whole_texts(lib):
    n = TILE + 77
    blank = np.frombuffer(b" \t\n\v\f\r", dtype=np.uint8)[np.arange(n) % 6]
    starts = [0, 5, 1024, 1025, TILE, n - 1]
    assert run(lib, blank, SQUEEZE, seg_start=starts).out == b" " * len(starts)
    assert run(lib, blank, SQUEEZE).out == b" "
    assert run(lib, blank, STRIP, seg_start=starts).m == 0
    assert run(lib, blank, PERCENT | STRIP).m == 0
    plain = random_text(n, 3, b"abcxyz")
    for flags in MODES:
        x = run(lib, plain, flags, what="nothing dropped")
        assert x.out == plain.tobytes() and x.info[:4] == [n, 0, 0, 0]
    mixed = random_text(n, 4)
    assert run(lib, mixed, 0, seg_start=starts, what="flags == 0").out == mixed.tobytes()
    every = np.frombuffer(b"%41", dtype=np.uint8)[np.arange(3 * 5000) % 3]
    assert run(lib, every, PERCENT).out == b"A" * 5000


@pytest.mark.parametrize("origin", [-1000, 12345, -(2 ** 31) + 100, 2 ** 31 - 70000])
def test_text_origin(lib, origin):
    n = 20000
    text = random_text(n, 5)
    starts = [origin - 5, origin, origin + 501, origin + TILE, origin + n, origin + n + 9]
    starts = [min(max(s, -(2 ** 31)), INT32_MAX) for s in starts]
    for flags in (PERCENT | SQUEEZE, STRIP):
        x = run(lib, text, flags, origin=origin, seg_start=starts, what="origin")
        assert x.out == nm.normalize(text.tobytes(), flags, seg_start=[0, 501, TILE]).out


def test_capacities(lib):
    n = 3 * TILE + 19
    text = random_text(n, 6)
    dt = upload_text(text)
    for flags in (PERCENT | SQUEEZE, 0):
        m = nm.normalize(text.tobytes(), flags).m
        for cap in (0, 1, 15, 16, 17, TILE, m - 1, m, m + 1):
            x = run(lib, text, flags, cap=cap, d_text=dt, what="capacity")
            assert x.info[4] == int(cap < m)
        x = run(lib, text, flags, cap=0, with_out=False, d_text=dt, seg_start=[0, 100, n], what="no output")
        assert x.info[0] == m and x.info[4] == 0
    dt.free()


def test_custom_blank_set_and_byte(lib):
    text = random_text(40000, 8)
    for blanks, byte in ((b"\0", 0x20), (b"\0 %", 0x5F), (b"4a", 0), (bytes(range(256)), 0xFF), (b"", 0x20)):
        for flags in (SQUEEZE, STRIP, PERCENT | SQUEEZE, PERCENT | STRIP):
            run(lib, text, flags, blanks=blanks, blank_byte=byte, seg_start=[0, 7, 20000], what="blank set %r" % blanks[:4])
    wide = "needle in a haystack".encode("utf-16-le")
    assert run(lib, np.frombuffer(wide, dtype=np.uint8), STRIP, blanks=b"\0").out == b"needle in a haystack"


def test_a_block_of_several_tiles(lib):
    """a text of more tiles than the grid has blocks.  The model walks one period; the period begins and ends with a
    letter, so no unit and no run crosses from one repetition into the next, and the whole result is the period's,
    repeated"""
    period = random_text(4 * TILE + 1024, 9)
    period[0] = period[-1] = 0x78
    reps = 520
    flags = PERCENT | SQUEEZE
    p = nm.normalize(period.tobytes(), flags)
    text = np.tile(period, reps)
    n = text.size
    assert n // TILE > 2 * 1024
    dt = upload_text(text)
    got = Call(lib, dt, n, flags, reps * p.m).read("several tiles")
    dt.free()
    assert got["info"].tolist() == [reps * p.m, reps * p.info[1], reps * p.info[2], reps * p.info[3], 0, 0, 0, 0]
    og.same(got["keep"], np.tile(p.keep_words, reps), "keep words")
    cells = period.size // nm.BLOCK
    block = (np.arange(reps, dtype=np.int64)[:, None] * p.m + p.block[None, :cells]).reshape(-1)
    og.same(got["block"], np.r_[block, reps * p.m], "block cells")
    og.same(got["out"], np.tile(np.frombuffer(p.out, dtype=np.uint8), reps), "output")


def test_stability_and_streams(lib):
    n = 5 * TILE + 3
    text = random_text(n, 11)
    flags = PERCENT | SQUEEZE
    starts = [0, 1000, TILE + 1]
    x = run(lib, text, flags, seg_start=starts)
    dt = upload_text(text)
    s = C.c_void_p()
    check(lib.acm_rt_stream_create(C.byref(s)), "acm_rt_stream_create")
    runs = [Call(lib, dt, n, flags, x.m, seg_start=starts, ws_fill=f, stream=st).read("streams")
            for f, st in ((0xFF, None), (0xA5, None), (0x00, s.value), (0xFF, s.value))]
    for r in runs:
        assert bytes(r["out"]) == x.out and r["info"].tolist() == x.info
        for key in ("keep", "block", "seg"):
            assert np.array_equal(r[key], runs[0][key]), key
    lib.acm_rt_stream_destroy(s.value)
    dt.free()


def test_argument_errors(lib):
    prev = 0
    for n in (0, 1, 1023, 1024, 100000, 1 << 24, 2 ** 31 - 17):
        for segs in (0, 1, 1 << 20):
            b = lib.acm_normalize_workspace_bytes(n, segs)
            assert b % 256 == 0 and b > 0 and b >= prev and b >= lib.acm_normalize_workspace_bytes(n, 0)
        prev = lib.acm_normalize_workspace_bytes(n, 0)
    buf = og.Guarded(1 << 14)
    check(lib.acm_rt_memset(buf.ptr, 0, 1 << 16, None), "acm_rt_memset")
    out = og.Guarded(1 << 14)
    ws = lib.acm_normalize_workspace_bytes(1000, 4)
    w = DeviceArray(ws)
    big = 2 ** 31 - 16
    base = dict(text=buf.ptr, n=1000, origin=0, flags=PERCENT | SQUEEZE, mask=None, byte=0x20, out=out.ptr, cap=1000,
                keep=out.ptr + 4096, block=out.ptr + 8192, st=buf.ptr + 8192, segs=4, sg=out.ptr + 12288, info=out.ptr + 16384,
                ws=w.ptr, ws_bytes=ws)
    bad = [dict(text=None), dict(info=None), dict(keep=None), dict(block=None), dict(text=buf.ptr + 8), dict(out=out.ptr + 4),
           dict(n=big), dict(cap=big), dict(out=None), dict(st=None), dict(sg=None), dict(segs=0), dict(ws_bytes=ws - 1),
           dict(ws=None), dict(origin=2 ** 31), dict(origin=-(2 ** 31) - 1), dict(flags=8), dict(flags=0x80000001),
           dict(flags=SQUEEZE | STRIP), dict(flags=7), dict(byte=256), dict(byte=-1)]

    def call(x):
        return lib.acm_normalize_async(x["text"], x["n"], x["origin"], x["flags"], x["mask"], x["byte"], x["out"], x["cap"],
                                       x["keep"], x["block"], x["st"], x["segs"], x["sg"], x["info"], x["ws"], x["ws_bytes"], None)

    for args in bad:
        x = dict(base)
        x.update(args)
        assert call(x) == -1, args
        assert lib.acm_last_error()
    check(lib.acm_rt_device_sync(), "sync")
    out.untouched(what="argument errors")                           # nothing was enqueued
    # good arguments are accepted: so are a NULL text of no bytes, a NULL output of no room, any blank_byte without squeeze
    for args in (dict(), dict(text=None, n=0), dict(out=None, cap=0), dict(flags=STRIP, byte=-5), dict(flags=0, byte=999)):
        x = dict(base)
        x.update(args)
        assert call(x) == 0, args
        got = out.read()
        assert got[16384 // 4:16384 // 4 + 8].tolist() == [x["n"], 0, 0, 0, 0, 0, 0, 0]
    # the remap
    rbase = dict(dfa=None, text=buf.ptr, n=1000, origin=0, flags=PERCENT, keep=out.ptr + 4096, block=out.ptr + 8192, pat=None,
                 off=buf.ptr + 4096, mr=100, oo=out.ptr + 20000, so=None, info=out.ptr + 16384)
    rbad = [dict(text=None), dict(keep=None), dict(block=None), dict(off=None), dict(oo=None), dict(info=None), dict(n=big),
            dict(mr=0x7FFFFFFF), dict(flags=8), dict(flags=6), dict(so=out.ptr + 24000), dict(pat=buf.ptr + 4096),
            dict(origin=2 ** 31)]
    out.buf.fill(og.FILL)
    check(lib.acm_rt_device_sync(), "sync")
    for args in rbad:
        x = dict(rbase)
        x.update(args)
        rc = lib.acm_normalize_remap_async(x["dfa"], x["text"], x["n"], x["origin"], x["flags"], x["keep"], x["block"], x["pat"],
                                           x["off"], x["mr"], x["oo"], x["so"], x["info"], None)
        assert rc == -1, args
    check(lib.acm_rt_device_sync(), "sync")
    out.untouched(what="remap argument errors")
    for b in (buf, out, w):
        b.free()


# ------------------------------------------------------------------ 4. the remap

PATS = [b"a", b"%4", b"a b", b" b", b"href", b"a href", b"0A"]


@pytest.fixture(scope="module")
def matcher(gpu):
    a = Automaton()
    for i, p in enumerate(PATS):
        a.add(p, i)
    a.compile()
    m = Matcher(a, 0, max_text=1 << 16)
    yield m
    m.close()


class Mapped:
    """a normalise call whose map stays on the device"""

    def __init__(self, lib, text, flags, origin=0, seg_start=None):
        self.text, self.flags, self.origin = np.asarray(text, dtype=np.uint8), flags, origin
        self.x = nm.normalize(self.text.tobytes(), flags, origin=origin, seg_start=seg_start)
        self.dt = upload_text(self.text)
        self.call = Call(lib, self.dt, self.text.size, flags, self.x.m + 16, origin, seg_start=seg_start)

    def remap(self, lib, matcher, offs, pats=None, max_records=None, count=None, in_place=False, what=""):
        offs = np.asarray(offs, dtype=np.int64)
        R = offs.size if max_records is None else max_records
        cnt = offs.size if count is None else count
        plane = np.r_[cnt, offs].astype(np.int64).astype(np.int32)
        off_in = og.Guarded(offs.size + 1, host=plane)
        off_out = off_in if in_place else og.Guarded(offs.size + 1)
        pat_in = og.Guarded(offs.size + 1, host=np.r_[cnt, pats].astype(np.int64).astype(np.int32)) if pats is not None else None
        start = og.Guarded(offs.size + 1) if pats is not None else None
        info = og.Guarded(8)
        check(lib.acm_normalize_remap_async(matcher.dfa if pats is not None else None, self.dt.ptr, self.text.size, self.origin,
                                            self.flags, self.call.keep.ptr, self.call.block.ptr,
                                            pat_in.ptr if pats is not None else None, off_in.ptr, R, off_out.ptr,
                                            start.ptr if pats is not None else None, info.ptr, None), "acm_normalize_remap_async")
        seen = min(max(cnt, 0), R)
        xo, xs, bad = nm.remap(self.x, offs[:seen], None if pats is None else pats[:seen], [len(p) for p in PATS])
        got_o, got_i = off_out.read(what=what), info.read(what=what)
        assert got_i.tolist() == [seen, bad, 0, 0, 0, 0, 0, 0], (what, got_i.tolist(), seen, bad)
        exp = np.full(offs.size + 1, og.FILL32, dtype=np.int64)
        if in_place:
            exp[:] = plane                                          # (the count cell stays what it is)
        else:
            exp[0] = seen
        exp[1:1 + seen] = xo
        og.same(got_o, exp, what + ": remapped offsets")
        if pats is not None:
            exp = np.full(offs.size + 1, og.FILL32, dtype=np.int64)
            exp[0] = seen
            exp[1:1 + seen] = xs
            og.same(start.read(what=what), exp, what + ": remapped starts")
            og.same(pat_in.read(what=what), np.r_[cnt, pats].astype(np.int64).astype(np.int32), what + ": the pattern plane")
        for b in {off_in, off_out, pat_in, start, info} - {None}:
            b.free()

    def close(self):
        self.call.read("map")
        self.dt.free()


@pytest.mark.parametrize("flags", MODES, ids=mode_id)
def test_remap_every_offset(lib, matcher, flags):
    rng = np.random.default_rng(flags)
    for origin, starts in ((0, None), (-777, [-777 + 100, -777 + 1030, -777 + TILE])):
        mp = Mapped(lib, random_text(2 * TILE + 100, 50 + flags), flags, origin, starts)
        m = mp.x.m
        offs = np.arange(m)
        mp.remap(lib, matcher, offs, what="every offset")
        mp.remap(lib, matcher, offs, pats=rng.integers(0, len(PATS), m), what="starts")
        mp.remap(lib, matcher, offs[::-1].copy(), in_place=True, what="in place")
        mp.close()


def test_remap_hostile_planes(lib, matcher):
    mp = Mapped(lib, random_text(5000, 60), PERCENT | SQUEEZE)
    m = mp.x.m
    offs = np.array([0, -1, m - 1, m, m + 1, INT32_MAX, -(2 ** 31), 5, 1, 2, 3], dtype=np.int64)
    pats = np.array([0, 0, 5, 0, 0, 0, 0, len(PATS), -1, INT32_MAX, 5], dtype=np.int64)    # (pattern 5 of 6 bytes at 3: no start)
    mp.remap(lib, matcher, offs, what="hostile offsets")
    mp.remap(lib, matcher, offs, pats=pats, what="hostile patterns")
    mp.remap(lib, matcher, offs, pats=pats, in_place=True, what="hostile, in place")
    for cnt, R in ((offs.size, 4), (INT32_MAX, offs.size), (-1, offs.size), (3, offs.size), (offs.size, 0)):
        mp.remap(lib, matcher, offs, pats=pats, max_records=R, count=cnt, what="count %d of %d" % (cnt, R))
    mp.close()
    # an empty map
    mp = Mapped(lib, np.zeros(0, dtype=np.uint8), PERCENT)
    mp.remap(lib, matcher, [0, -1, 1], what="empty")
    mp.close()


# ------------------------------------------------------------------ 5. end to end


def cpu_matches(pats, texts, kw):
    """(pattern, start, end) in the coordinates of the concatenation: the model normalises each text, the CPU oracle
    finds every pattern on the normalised bytes, the model's arrays map back"""
    o = orc.Oracle()
    for i, p in enumerate(pats):
        o.add(p, i)
    o.compile()
    found, base = set(), 0
    for t in texts:
        x = nm.normalize(t, **kw)
        pos, pat, _ = o.scan_all(x.out)
        for e, p in zip(pos.tolist(), pat.tolist()):
            found.add((p, base + int(x.first[e - len(pats[p]) + 1]), base + int(x.last[e])))
        base += len(t)
    o.close()
    return found


def gpu_matches(res):
    pats, starts, ends, m = res
    return set(zip(pats.tolist(), starts.tolist(), ends.tolist()))


def test_scan_normalized_the_point(matcher):
    for text, span in ((b"<a \t\n href>", (1, 9)), (b"<a%20href>", (1, 8)), (b"<a%20 %09href>", (1, 12))):
        offs, pats, _ = matcher.scan_all(text)
        assert 5 not in pats.tolist()                               # Matcher.scan finds none of them
        assert 5 not in matcher.scan(text)[1].tolist()
        got = gpu_matches(matcher.scan_normalized(text, percent=True, squeeze=True, all_patterns=True))
        assert (5, span[0], span[1]) in got, (text, got)
        assert got == cpu_matches(PATS, [text], dict(flags=PERCENT | SQUEEZE))
        first = matcher.scan_normalized(text, percent=True, squeeze=True)
        assert gpu_matches(first) <= got and first[3] == 8


def test_scan_normalized_against_the_cpu(matcher):
    text = bytes(random_text(30000, 70, b"a b%4%200Ahref \t"))
    for kw, fl in ((dict(percent=True), PERCENT), (dict(squeeze=True), SQUEEZE), (dict(percent=True, strip=True), PERCENT | STRIP),
                   (dict(percent=True, squeeze=True), PERCENT | SQUEEZE), (dict(), 0)):
        res = matcher.scan_normalized(text, all_patterns=True, **kw)
        exp = cpu_matches(PATS, [text], dict(flags=fl))
        assert gpu_matches(res) == exp and len(exp) == res[0].size > 1000 and res[3] == nm.normalize(text, fl).m
    res = matcher.scan_normalized(text, strip=True, blank_set=b"%4 ", all_patterns=True)
    assert gpu_matches(res) == cpu_matches(PATS, [text], dict(flags=STRIP, blanks=b"%4 "))
    assert matcher.scan_normalized(b"   ", strip=True)[3] == 0
    with pytest.raises(AcmError) as e:
        matcher.scan_normalized(text, squeeze=True, out_capacity=100)
    assert e.value.code == _lib.ACM_ERR_CAPACITY


def test_scan_normalized_texts(matcher):
    """matches that would span two texts only if runs joined or the scan ran on: 'a ' ends a text and ' b' begins the next
    (squeezed into one run it would read 'a b'), 'a hr' + 'ef'"""
    texts = [b"xa  ", b"  b", b"a hr", b"ef a%20", b"%20b a  href", b"", b"a \t b"]
    got = gpu_matches(matcher.scan_normalized(texts=texts, percent=True, squeeze=True, all_patterns=True))
    assert got == cpu_matches(PATS, texts, dict(flags=PERCENT | SQUEEZE))
    joined = gpu_matches(matcher.scan_normalized(b"".join(texts), percent=True, squeeze=True, all_patterns=True))
    assert (2, 1, 6) in joined and (2, 1, 6) not in got and (3, 4, 6) in got
    assert (5, 7, 12) in joined and (5, 7, 12) not in got
    rng = np.random.default_rng(5)
    big = bytes(random_text(20000, 71, b"a b%4%200Ahref \t"))
    cuts = np.sort(rng.integers(0, 20000, 40))
    parts = [big[a:b] for a, b in zip(np.r_[0, cuts], np.r_[cuts, 20000])]
    got = gpu_matches(matcher.scan_normalized(texts=parts, percent=True, squeeze=True, all_patterns=True))
    assert got == cpu_matches(PATS, parts, dict(flags=PERCENT | SQUEEZE)) and len(got) > 500
