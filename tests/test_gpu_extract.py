"""The context and extract passes on the device (acm_line_context_async, acm_extract_async, Matcher.scan_extract),
through the C ABI, compared cell for cell and byte for byte with tests/extract_model.py.  Every output has guard
cells or bytes on both sides and is pre-filled (tests/ops_guard.py), the workspace and the text's tail are poisoned
as tests/test_gpu_lines.py and tests/test_gpu_rewrite.py do."""
import numpy as np
import pytest

import extract_model as xm
import line_model as lm
import ops_guard as og
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib
from gpu_pattern_matching_amd._lib import check
from streams import Rig
from test_gpu_lines import Index, device_text

pytestmark = pytest.mark.gpu

MiB = 1 << 20
TILE = 16384                 # output bytes a workgroup of the copy kernel owns
INT32_MAX = 0x7FFFFFFF
PAST = 4096


def upload_text(text):
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    h = np.full(((t.size + 15) & ~15) + PAST, 0xC3, dtype=np.uint8)
    h[:t.size] = t
    return DeviceArray.from_numpy(h)


def random_text(n, seed=0, newline=1 / 60):
    rng = np.random.default_rng(seed)
    t = rng.integers(0x20, 0x7F, n).astype(np.uint8)
    t[rng.random(n) < newline] = 0x0A
    return bytes(t)


class Extract:
    """one extract call from poisoned outputs; read() checks the guard bands"""

    def __init__(self, lib, d_text, n, bp, ep, max_ranges, cap, origin=0, flags=0, glue=b"", term=-1, at_cap=None, seg=None,
                 with_out=True, ws_fill=0xA5, stream=None):
        self.lib, self.stream, self.with_out = lib, stream, with_out
        self.out = og.Guarded(cap if with_out else 16, dtype=np.uint8)
        self.at = og.Guarded(at_cap) if at_cap is not None else None
        nseg = 0 if seg is None else len(seg)
        self.seg_in = og.Guarded(max(nseg, 1), host=np.asarray(seg, dtype=np.int32)) if nseg else None
        self.seg = og.Guarded(nseg) if nseg else None
        self.info = og.Guarded(8)
        nb = lib.acm_extract_workspace_bytes(max_ranges, nseg)
        self.ws = og.Workspace(nb, ws_fill)
        self.go = lambda: check(lib.acm_extract_async(
            d_text.ptr if d_text is not None else None, n, origin, _ptr(bp), _ptr(ep), max_ranges, flags, glue if glue else None,
            len(glue), term, self.out.ptr if with_out else None, cap if with_out else 0, self.at.ptr if self.at else None,
            at_cap or 0, self.seg_in.ptr if nseg else None, nseg, self.seg.ptr if nseg else None, self.info.ptr, self.ws.ptr, nb,
            stream), "acm_extract_async")
        self.go()

    def read(self, what="", free=True):
        st = self.stream
        self.ws.check(st, what)
        res = dict(out=self.out.read(st, what), info=self.info.read(st, what),
                   at=self.at.read(st, what) if self.at else None, seg=self.seg.read(st, what) if self.seg else None)
        if free:
            for x in (self.out, self.at, self.seg_in, self.seg, self.info, self.ws):
                if x is not None:
                    x.free()
        return res


def _ptr(x):
    return x if isinstance(x, int) or x is None else x.ptr


def compare(got, exp, cap, at_cap, with_out, what):
    """the downloads of an Extract against the model's dict (made with limit = cap)"""
    assert got["info"].tolist() == exp["info"].tolist(), "%s: info %s, model %s" % (what, got["info"].tolist(), exp["info"].tolist())
    if with_out:
        k = min(exp["m"], cap)
        e = np.frombuffer(exp["out"], dtype=np.uint8)
        assert e.size == k
        bad = np.flatnonzero(got["out"][:k] != e)
        assert bad.size == 0, "%s: output byte %d = %d, model %d (%d differ)" % (what, bad[0], got["out"][bad[0]], e[bad[0]], bad.size)
        assert (got["out"][k:] == og.FILL).all(), "%s: a byte at or behind min(m, capacity) = %d was written" % (what, k)
    else:
        assert (got["out"] == og.FILL).all()
    if at_cap is not None:
        og.same(got["at"], xm.at_plane(exp["at"], at_cap, og.FILL32), what + ": at plane")
    if exp["seg_out"] is not None:
        og.same(got["seg"], exp["seg_out"], what + ": seg_out")


def run(lib, text, begins, ends, origin=0, cap=None, incl=False, glue=b"", term=-1, seg=None, max_ranges=None, count=None,
        at_cap="fit", with_out=True, what="", d_text=None, ws_fill=0xA5):
    """one call over host ranges, compared whole with the model; returns the model's dict"""
    begins, ends = np.asarray(begins, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    mr = len(begins) if max_ranges is None else max_ranges
    bp, ep = xm.plane_of(begins, count), xm.plane_of(ends, count)
    full = xm.extract(text, origin, bp, ep, mr, incl, glue, term, seg)
    cap = full["m"] + 37 if cap is None else cap
    exp = xm.extract(text, origin, bp, ep, mr, incl, glue, term, seg, limit=cap) if with_out else full
    at_cap = len(full["at"]) + 5 if at_cap == "fit" else at_cap
    dt = d_text if d_text is not None else upload_text(text)
    dbp, dep = DeviceArray.from_numpy(bp, pad_to=0), DeviceArray.from_numpy(ep, pad_to=0)
    got = Extract(lib, dt, len(text), dbp, dep, mr, cap, origin, 1 if incl else 0, glue, term, at_cap, seg, with_out,
                  ws_fill).read(what)
    compare(got, exp, cap, at_cap, with_out, "%s n=%d ranges=%d cap=%d origin=%d" % (what, len(text), len(begins), cap, origin))
    for b in (dbp, dep) + ((dt,) if d_text is None else ()):
        b.free()
    return full


def pieces(total, seed, lo=20, hi=200):
    """lengths in [lo, hi] that sum to total (the last one shorter if need be)"""
    rng = np.random.default_rng(seed)
    out = []
    while total > 0:
        k = min(int(rng.integers(lo, hi + 1)), total)
        out.append(k)
        total -= k
    return out


# ------------------------------------------------------------------ extract

LENGTHS = (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)


@pytest.mark.parametrize("m", LENGTHS)
def test_output_lengths(gpu, lib, m):
    t = random_text(m + m // 10 + 300, m)
    # one range of m bytes at an odd source phase: a tile inside one range streams
    run(lib, t, [7] if m else [], [7 + m] if m else [], what="one range")
    # ranges of 20 to 200 bytes with gaps between them: m bytes of output
    lens = pieces(m, m + 1)
    if len(lens) > 1:
        gaps = np.arange(len(lens)) % 3
        b = np.cumsum(np.r_[0, lens[:-1]]) + np.cumsum(gaps)
        assert b[-1] + lens[-1] <= len(t)
        full = run(lib, t, b, b + np.asarray(lens), what="lines")
        assert full["m"] == m
        # ... and with glue and terminators the same ranges give more
        run(lib, t, b, b + np.asarray(lens), glue=b"--\n", term=0x0A, seg=[0, int(b[len(b) // 2])], what="glued lines")


def test_every_source_and_destination_phase(gpu, lib):
    """a 40-byte range at each of the 16 x 16 (source phase, destination phase) pairs, in one call: a filler range in
    front of each brings the output to the wanted phase"""
    t = random_text(4096, 5)
    begins, ends, pos, want = [], [], 0, []
    for s in range(16):
        for d in range(16):
            fill = (d - pos) % 16
            if fill:
                begins.append(1000)
                ends.append(1000 + fill)
                pos += fill
            b = 64 + 48 * d + s + 16 * ((s * 16 + d) % 3)
            assert b % 16 == s
            want.append((b % 16, pos % 16))
            begins.append(b)
            ends.append(b + 40)
            pos += 40
    assert len(set(want)) == 256
    full = run(lib, t, begins, ends, what="phases")
    assert full["m"] == pos


def test_more_ranges_in_a_tile_than_threads(gpu, lib):
    t = random_text(20000, 6)
    rng = np.random.default_rng(6)
    b = np.sort(rng.integers(0, len(t), size=5000))
    full = run(lib, t, b, b + 1, what="5000 one-byte ranges")
    assert full["m"] == 5000
    run(lib, t, b, b + 1, glue=b"+", term=0x0A, what="5000 one-byte ranges, glue and terminator")


def test_a_range_longer_than_a_tile(gpu, lib):
    n = 5 * TILE // 2
    t = random_text(n + 100, 7, newline=0)
    for b in (0, 3, 16):
        run(lib, t, [b], [b + n], what="2.5 tiles")
        run(lib, t, [50, b, 60], [53, b + n, 70], glue=b"--\n", term=0x0A, what="2.5 tiles between two short ranges")


@pytest.mark.parametrize("n", (17, 4099, TILE + 13))
def test_ranges_that_end_at_n(gpu, lib, n):
    t = random_text(n, n, newline=0)
    assert n % 16
    run(lib, t, [n - 5], [n], what="tail")
    run(lib, t, [0], [n], what="whole")
    run(lib, t, [0, n - 1, n - 16, n - 17], [n, n, n, n], glue=b"ab", term=0x0A, what="four ends")
    run(lib, t, [0, n - 5], [n - 1, n - 1], incl=True, what="inclusive ends")


@pytest.mark.parametrize("glue", (b"", b"-", b"--\n", b"0123456789abcdef"))
def test_glue_lengths(gpu, lib, glue):
    t = random_text(3000, 8)
    lens = pieces(2000, 9, 1, 50)
    b = np.cumsum(np.r_[0, lens[:-1]]) + np.arange(len(lens))
    run(lib, t, b, b + np.asarray(lens), glue=glue, what="glue %d" % len(glue))
    run(lib, t, b, b + np.asarray(lens), glue=glue, term=0x41, seg=[int(x) for x in b[::7]], what="glue %d, texts" % len(glue))


def test_glue_and_terminators_on_a_tile_border(gpu, lib):
    t = bytearray(random_text(3 * TILE, 10, newline=0))
    for first in range(TILE - 18, TILE + 2):
        # the first range's terminator and the glue behind it lie at first, first + 1 ...: every split of the 1 + 16
        # bytes over the border between two tiles
        for glue in (b"--\n", b"0123456789abcdef"):
            run(lib, bytes(t), [5, TILE + 100], [5 + first, TILE + 140], glue=glue, term=0x0A, what="border %d" % first)
    # the terminator's byte decides: the last byte equal and unequal
    t[99] = 0x0A
    full = run(lib, bytes(t), [0, 200, 90], [100, 300, 100], term=0x0A, what="terminators")
    assert full["info"][7] == 1 and full["m"] == 100 + 101 + 10


def test_descending_overlapping_and_repeated_ranges(gpu, lib):
    t = random_text(5000, 11)
    rng = np.random.default_rng(11)
    b = rng.integers(0, 4900, size=300)
    e = b + rng.integers(1, 100, size=300)
    run(lib, t, b, e, glue=b"|", term=0x0A, seg=[1000, 1000, 2500, 6000], what="any order")
    d = np.sort(b)[::-1]
    run(lib, t, d, d + 50, glue=b"|", seg=[0, 2500], what="descending")
    run(lib, t, [100] * 50, [400] * 50, glue=b"--\n", term=0x0A, what="repeated")


def test_skipped_ranges(gpu, lib):
    t = random_text(1000, 12)
    P = og.FILL32
    for origin in (0, -300, 5000):
        o = origin
        b = [o - 1, o, o + 10, o + 990, o + 20, o + 30, P, o + 40, -P, o + 1000, o + 999]
        e = [o + 5, o + 5, o + 10, o + 1001, o + 19, o + 35, o + 50, P, o + 60, o + 1001, o + 1000]
        full = run(lib, t, b, e, origin=origin, glue=b"--\n", term=0x0A, seg=[o + 25], what="skipped, origin %d" % origin)
        assert full["info"][0] == 3 and full["info"][1] == len(b) - 3
    # all skipped: no output, the figures only
    full = run(lib, t, [-5, 2000], [3, 2001], what="all skipped")
    assert full["m"] == 0 and full["info"][1] == 2


def test_the_count_cell(gpu, lib):
    t = random_text(1000, 13)
    b = np.arange(0, 900, 30)
    for count, mr in ((-1, 30), (-(1 << 31), 30), (1000, 30), (INT32_MAX, 12), (7, 30), (0, 30), (30, 0)):
        run(lib, t, b, b + 20, glue=b"-", count=count, max_ranges=mr, what="count %d max_ranges %d" % (count, mr))


@pytest.mark.parametrize("origin", (-1000, -7, 4096, INT32_MAX - 5000))
def test_text_origin(gpu, lib, origin):
    t = random_text(3000, 14)
    lens = pieces(2500, 15)
    b = np.cumsum(np.r_[0, lens[:-1]]) + np.arange(len(lens)) + origin
    run(lib, t, b, b + np.asarray(lens), origin=origin, glue=b"--\n", term=0x0A, seg=[origin, origin + 1500],
        what="origin %d" % origin)


def test_capacities(gpu, lib):
    t = random_text(40000, 16)
    b, e = [10, 20000, 100], [10 + 18000, 20000 + 17000, 150]
    full = xm.extract(t, 0, xm.plane_of(b), xm.plane_of(e), 3, glue=b"0123456789abcdef", terminator=0x0A)
    m = full["m"]
    glue_at = full["at"][1] - 16
    for cap in (0, 1, 15, 16, 17, 9000, TILE, glue_at, glue_at + 1, glue_at + 7, glue_at + 16, m - 1, m, m + 1):
        run(lib, t, b, e, cap=cap, glue=b"0123456789abcdef", term=0x0A, what="capacity %d of %d" % (cap, m))
    # no output buffer: the figures, the at plane and seg_out only
    run(lib, t, b, e, glue=b"0123456789abcdef", term=0x0A, seg=[0, 150], with_out=False, what="NULL output")
    # the at plane's overflow contract
    for at_cap in (2, 3, 4, 5, None):
        run(lib, t, b, e, glue=b"-", at_cap=at_cap, what="at_capacity %s" % at_cap)


def test_an_output_beyond_two_to_the_31(gpu, lib):
    n, k = MiB, 3000
    t = random_text(n, 17)
    full = run(lib, t, [0] * k, [n] * k, cap=MiB, glue=b"-", seg=[0, 1], what="3000 MiB")
    m = full["m"]
    assert m == k * n + (k - 1) and m > 1 << 31
    assert (int(np.uint32(full["info"][3])) << 32 | int(np.uint32(full["info"][2]))) == m
    assert full["at"][-1] == INT32_MAX and full["at"][1] == n + 1 and full["seg_out"].tolist() == [0, INT32_MAX]


def test_workspace_fills_and_repeat(gpu, lib):
    """the same call over differently poisoned workspaces, on a created stream, twice into the same buffers"""
    t = random_text(50000, 18)
    lens = pieces(40000, 19)
    b = np.cumsum(np.r_[0, lens[:-1]]) + np.arange(len(lens))
    e = b + np.asarray(lens)
    for fill in og.WS_FILLS:
        run(lib, t, b, e, glue=b"--\n", term=0x0A, seg=[0, 20000, 45000], ws_fill=fill, what="workspace fill %r" % fill)
    rig = Rig()
    s = rig.stream()
    bp, ep = xm.plane_of(b), xm.plane_of(e)
    exp = xm.extract(t, 0, bp, ep, len(b), glue=b"--\n", terminator=0x0A, seg_start=[0, 20000, 45000])
    dt, dbp, dep = upload_text(t), DeviceArray.from_numpy(bp, pad_to=0), DeviceArray.from_numpy(ep, pad_to=0)
    lib.acm_rt_device_sync()
    c = Extract(lib, dt, len(t), dbp, dep, len(b), exp["m"] + 5, 0, 0, b"--\n", 0x0A, len(b) + 2, [0, 20000, 45000], stream=s)
    first = c.read("first run", free=False)
    c.go()
    second = c.read("second run")
    compare(first, exp, exp["m"] + 5, len(b) + 2, True, "first run")
    for k in first:
        assert np.array_equal(first[k], second[k]), "the second run left other %s" % k
    for x in (dt, dbp, dep):
        x.free()
    rig.close()


# ------------------------------------------------------------------ context

def run_context(lib, ix, origin, end, off_plane, max_records, invert, before, after, seg, ocap, with_lines=True, stream=None,
                ws_fill=0xA5):
    nseg = 0 if seg is None else len(seg)
    outs = [og.Guarded(ocap) for _ in range(4 if with_lines else 3)]
    cinfo = og.Guarded(4)
    seg_in = og.Guarded(max(nseg, 1), host=np.asarray(seg, dtype=np.int32)) if nseg else None
    nb = lib.acm_line_context_workspace_bytes(ix.cap, nseg)
    ws = og.Workspace(nb, ws_fill)
    check(lib.acm_line_context_async(ix.start_ptr, ix.cap, ix.info_ptr, origin, end, off_plane, max_records, invert, before, after,
                                     seg_in.ptr if nseg else None, nseg, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                     outs[3].ptr if with_lines else None, ocap, cinfo.ptr, ws.ptr, nb, stream),
          "acm_line_context_async")
    ws.check(stream)
    got = [b.read(stream) for b in outs], cinfo.read(stream)
    for b in outs + [cinfo, ws] + ([seg_in] if seg_in else []):
        b.free()
    return got


def check_context(lib, t, offs, origin=0, prev=-1, invert=False, before=0, after=0, seg=None, ocap=None, with_lines=True,
                  what="", ix=None, d_off=None):
    own = ix is None
    if own:
        ix = Index(lib, t, 0x0A, origin, prev)
    _, e_info, e_st = lm.index(t, origin, 0x0A, prev)
    end = origin + len(t)
    exp, e_ctx = xm.context(e_st, e_info, origin, end, offs, invert, before, after, () if seg is None else seg)
    ocap = len(exp[0]) + 5 if ocap is None else ocap
    plane = d_off if d_off is not None else DeviceArray.from_numpy(xm.plane_of(offs), pad_to=0)
    got, ctx = run_context(lib, ix, origin, end, plane.ptr, len(offs), 1 if invert else 0, before, after, seg, ocap, with_lines)
    what = "%s lines=%d before=%d after=%d invert=%d capacity=%d" % (what, e_st.size, before, after, invert, ocap)
    assert ctx.tolist() == e_ctx.tolist(), "%s: ctx_info %s, model %s" % (what, ctx.tolist(), e_ctx.tolist())
    for g, x, name in zip(got, lm.planes(exp[:len(got)], ocap, og.FILL32), ("rel", "begin", "next", "lines")):
        og.same(g, x, "%s: %s plane" % (what, name))
    if d_off is None:
        plane.free()
    if own:
        ix.free()
    return exp, e_ctx


def text_of_lines(lines, seed, last_newline=True):
    rng = np.random.default_rng(seed)
    parts = [bytes(rng.integers(0x61, 0x7B, size=int(k)).astype(np.uint8)) + b"\n" for k in rng.integers(0, 12, size=lines)]
    t = b"".join(parts)
    return t if last_newline or not t else t[:-1] + b"x"


WINDOWS = ((0, 0), (1, 0), (0, 2), (2, 1), (31, 33), (32, 31), (33, 32), (1000, 2), (INT32_MAX, 0), (1, INT32_MAX),
           (INT32_MAX, INT32_MAX))


@pytest.mark.parametrize("lines", (0, 1, 31, 32, 33, 10007))
def test_context_line_counts(gpu, lib, lines):
    rng = np.random.default_rng(lines)
    for prev in (-1, 0x41):                      # with a lead line and without
        t = text_of_lines(lines, lines + 1, last_newline=prev < 0)
        n = len(t)
        ix = Index(lib, t, 0x0A, 100, prev)
        picks = []
        if n:
            picks = [np.sort(rng.integers(0, n, size=max(1, lines // 60))) + 100, np.array([100, 100 + n - 1])]
        picks += [np.zeros(0, dtype=np.int64)]
        for offs in picks:
            d_off = DeviceArray.from_numpy(xm.plane_of(offs), pad_to=0)
            for i, (before, after) in enumerate(WINDOWS if lines > 1000 else WINDOWS[::2]):
                for invert in (False, True):
                    check_context(lib, t, offs, 100, prev, invert, before, after, with_lines=bool(i % 2 or invert),
                                  what="prev %d" % prev, ix=ix, d_off=d_off)
            d_off.free()
        ix.free()


def test_context_everything_and_nothing_selected(gpu, lib):
    t = text_of_lines(3000, 20)
    _, _, st = lm.index(t)
    ix = Index(lib, t, 0x0A)
    for offs in (st, np.zeros(0, dtype=np.int64)):
        for invert in (False, True):
            exp, ctx = check_context(lib, t, offs, invert=invert, before=2, after=2, ix=ix)
            assert ctx[2] == (1 if ctx[0] else 0) and ctx[1] == ctx[0]
    # the first and the last line alone
    for offs in ([0], [len(t) - 1], [0, len(t) - 1]):
        for w in ((0, 0), (3, 3), (INT32_MAX, INT32_MAX)):
            check_context(lib, t, offs, before=w[0], after=w[1], ix=ix)
    ix.free()


def test_context_text_barriers(gpu, lib):
    t = text_of_lines(4000, 21)
    n = len(t)
    _, _, st = lm.index(t, 50)
    rng = np.random.default_rng(21)
    offs = np.sort(rng.integers(0, n, size=120)) + 50
    on_lines = [int(x) for x in st[::500]]
    inside = [int(x) + 1 for x in st[100::700] if x + 1 < 50 + n]
    segs = {
        "on line starts": on_lines,
        "inside lines": inside,
        "equal starts": sorted(on_lines[:3] * 3),
        "beyond the end": on_lines[:2] + [50 + n, 50 + n + 10, INT32_MAX],
        "in front of the origin": [0, 49] + on_lines[1:3],
        "every line its own text": [int(x) for x in st],
        "mixed": sorted(on_lines + inside),
    }
    ix = Index(lib, t, 0x0A, 50)
    d_off = DeviceArray.from_numpy(xm.plane_of(offs), pad_to=0)
    for name, seg in segs.items():
        for before, after in ((0, 0), (2, 2), (0, 40), (1000, 1), (INT32_MAX, INT32_MAX)):
            for invert in (False, True):
                check_context(lib, t, offs, 50, invert=invert, before=before, after=after, seg=seg, what=name, ix=ix, d_off=d_off)
    d_off.free()
    ix.free()


def test_context_capacities(gpu, lib):
    t = text_of_lines(500, 22)
    offs = np.arange(3, len(t), 97)
    ix = Index(lib, t, 0x0A)
    _, e_info, e_st = lm.index(t)
    groups = len(xm.context(e_st, e_info, 0, len(t), offs, False, 1, 1)[0][0])
    assert groups > 10
    for ocap in (2, 3, 4, groups + 1, groups + 2, groups + 3):
        for with_lines in (True, False):
            check_context(lib, t, offs, before=1, after=1, ocap=ocap, with_lines=with_lines, ix=ix)
    ix.free()


# ------------------------------------------------------------------ both passes

PATS = [b"needle", b"hay", b"ne"]
WORDS = [b"needle", b"hay", b"straw", b"pin", b"x", b"", b"nee dle", b"chaff", b"stubble and dust"]


def word_lines(lines, seed, hit=0.08):
    """lines of words, a pattern in about one line of twelve; the last line has no newline"""
    rng = np.random.default_rng(seed)
    picks = rng.integers(2, len(WORDS), size=(lines, 4))
    counts = rng.integers(0, 5, size=lines)
    hits = rng.random(lines) < hit
    out = []
    for i in range(lines):
        words = [WORDS[int(k)] for k in picks[i, :counts[i]]]
        if hits[i]:
            words.append(WORDS[i % 2])
        out.append(b" ".join(words))
    return b"\n".join(out)


def small_matcher(pats, n, wild=False):
    a = Automaton()
    for i, p in enumerate(pats):
        a.add(p, i)
    if wild:
        a.add_wildcard([b"q", bytes(range(256)), b"z"], len(pats))
    a.compile()
    return Matcher(a, 0, max_text=n)


def find_all(t, pats):
    """the offset every occurrence of a pattern ends at, ascending"""
    out = set()
    for p in pats:
        at = t.find(p)
        while at >= 0:
            out.add(at + len(p) - 1)
            at = t.find(p, at + 1)
    return sorted(out)


def test_scan_index_context_extract_on_one_stream(gpu, lib):
    """behind the index and the scan on a created stream, no sync in between, then once more into the same buffers"""
    t = word_lines(76000, 25)
    n = len(t)
    assert 800000 < n <= MiB + 3
    m = small_matcher(PATS, n)
    offs = np.asarray(find_all(t, PATS), dtype=np.int64)
    rig = Rig()
    s = rig.stream()
    d = device_text(t, 0x0A)
    _, e_info, e_st = lm.index(t)
    lcap = int(e_st.size) + 7
    groups, e_ctx = xm.context(e_st, e_info, 0, n, offs, False, 1, 2, [0, n // 2])
    k = len(groups[0])
    assert k > 1000
    bp, ep = xm.plane_of(groups[1]), xm.plane_of(groups[2])
    exp = xm.extract(t, 0, bp, ep, k, glue=b"--\n", terminator=0x0A, seg_start=[0, n // 2])
    cap = m.plane_capacity
    starts, linfo, cinfo, xinfo = og.Guarded(lcap), og.Guarded(8), og.Guarded(4), og.Guarded(8)
    planes = [og.Guarded(k + 2) for _ in range(4)]
    out, at, seg_out = og.Guarded(exp["m"], dtype=np.uint8), og.Guarded(k + 2), og.Guarded(2)
    seg_in = og.Guarded(2, host=np.array([0, n // 2], dtype=np.int32))
    wss = [og.Workspace(lib.acm_line_index_workspace_bytes(n)), og.Workspace(lib.acm_line_context_workspace_bytes(lcap, 2)),
           og.Workspace(lib.acm_extract_workspace_bytes(k, 2))]
    lib.acm_rt_device_sync()
    runs = []
    for _ in range(2):
        m.line_index_async(d, n, starts.ptr, lcap, linfo.ptr, workspace=(wss[0].ptr, wss[0].nbytes), stream=s)
        m.scan_async(d, n, 0, stream=s)
        m.line_context_async(starts.ptr, lcap, linfo.ptr, 0, n, m.off_plane, cap - 2, planes[0].ptr, planes[1].ptr, planes[2].ptr,
                             k + 2, cinfo.ptr, before=1, after=2, lines_out=planes[3].ptr, seg_start=seg_in.ptr, segments=2,
                             workspace=(wss[1].ptr, wss[1].nbytes), stream=s)
        m.extract_async(d, n, planes[1].ptr, planes[2].ptr, k, out.ptr, exp["m"], xinfo.ptr, glue=b"--\n", terminator=0x0A,
                        at_out=at.ptr, at_capacity=k + 2, seg_start=seg_in.ptr, segments=2, seg_out=seg_out.ptr,
                        workspace=(wss[2].ptr, wss[2].nbytes), stream=s)
        runs.append([x.read(s) for x in planes + [cinfo, xinfo, out, at, seg_out]])
    for w in wss:
        w.check(s)
    first, second = runs
    for g, x in zip(first[:4], lm.planes(groups, k + 2, og.FILL32)):
        og.same(g, x, "groups")
    assert first[4].tolist() == e_ctx.tolist() and first[5].tolist() == exp["info"].tolist()
    assert first[6].tobytes() == exp["out"]
    og.same(first[7], xm.at_plane(exp["at"], k + 2, og.FILL32), "at plane")
    og.same(first[8], exp["seg_out"], "seg_out")
    for x, y in zip(first, second):
        assert np.array_equal(x, y), "the second run left other cells"
    for b in [starts, linfo, cinfo, xinfo, out, at, seg_out, seg_in, d] + planes + wss:
        b.free()
    rig.close()
    m.close()


def test_scan_extract(gpu, lib):
    pats = PATS
    t = word_lines(6000, 23, hit=0.15)
    m = small_matcher(pats, len(t))
    offs = find_all(t, pats)
    assert len(offs) > 1000
    _, e_info, e_st = lm.index(t)
    for before, after, invert in ((0, 0, False), (2, 2, False), (1, 3, True), (0, 0, True), (INT32_MAX, 0, False)):
        data, groups, at, info, seg = m.scan_extract(t, before=before, after=after, invert=invert)
        exp_out, exp_groups, ex = xm.grep_like(t, offs, before, after, invert)
        assert data == exp_out and seg is None and info.tolist() == ex["info"].tolist() and at.tolist() == ex["at"]
        assert np.array_equal(groups, np.stack([exp_groups[0] + 1] + list(exp_groups[1:]), axis=1))
    # a glue and a terminator of the caller's; another delimiter
    data = m.scan_extract(t, before=1, after=1, glue=b"~", terminator=-1)[0]
    assert data == xm.grep_like(t, offs, 1, 1, glue=b"~", terminator=-1)[0]
    data = m.scan_extract(t, delimiter=b" ", after=1)[0]
    assert data == xm.grep_like(t, offs, 0, 1, delimiter=0x20)[0]
    # per_line: no match spans two lines
    assert m.scan_extract(b"needle", delimiter=b"d")[0] == b"need" + b"led"
    assert m.scan_extract(b"needle", delimiter=b"d", per_line=True)[0] == b"need"
    # texts: each matched alone, context and glue stay inside a text
    texts = [b"a\nneedle\nb\nc\n", b"d\ne\nhay\n", b"", b"f\n", b"g\nne\n"]
    data, groups, at, info, seg = m.scan_extract(texts=texts, before=1, after=1)
    starts = np.cumsum([0] + [len(x) for x in texts[:-1]])
    whole = b"".join(texts)
    exp_out, exp_groups, ex = xm.grep_like(whole, find_all(whole, pats), 1, 1, seg_start=[int(x) for x in starts])
    assert data == exp_out == b"a\nneedle\nb\n" + b"e\nhay\n" + b"g\nne\n" and seg.tolist() == ex["seg_out"].tolist()
    assert len(groups) == 3 and info[7] == 0 and groups[:, 0].tolist() == [1, 6, 9]
    # only_matching: grep -o's bytes
    data, groups, at, info, seg = m.scan_extract(t, only_matching=True)
    sel = m.scan_select(t)
    assert data == b"".join(t[s:o + 1] + b"\n" for s, o in zip(sel[2].tolist(), sel[0].tolist()))
    assert len(groups) == sel[0].size > 1000 and b"needle\n" in data and info[7] == sel[0].size
    # an output that does not fit is an error
    with pytest.raises(AcmError) as e:
        m.scan_extract(t, before=1, after=1, out_capacity=1000)
    assert e.value.code == _lib.ACM_ERR_CAPACITY
    m.close()
    w = small_matcher(pats, 4096, wild=True)
    with pytest.raises(ValueError):
        w.scan_extract(b"needle q.z\n", only_matching=True)
    assert w.scan_extract(b"a\nneedle q.z\n")[0] == b"needle q.z\n"
    w.close()


def test_end_inclusive_over_select_planes(gpu, lib):
    """the select pass's (start, offset) planes as they lie on the device"""
    pats = [b"ab", b"abc", b"bcd", b"d"]
    rng = np.random.default_rng(24)
    t = bytes(rng.integers(0x61, 0x66, size=50000).astype(np.uint8))
    m = small_matcher(pats, len(t))
    offs, ps, starts, _ = m.scan_select(t)
    assert offs.size > 3000
    sp, op = xm.plane_of(starts), xm.plane_of(offs.astype(np.int64))
    full = xm.extract(t, 0, sp, op, offs.size, inclusive=True, terminator=0x0A)
    dt, dsp, dop = upload_text(t), DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(op, pad_to=0)
    got = Extract(lib, dt, len(t), dsp, dop, offs.size, full["m"] + 3, flags=_lib.EXTRACT_END_INCLUSIVE, term=0x0A,
                  at_cap=offs.size + 2).read("select planes")
    exp = xm.extract(t, 0, sp, op, offs.size, inclusive=True, terminator=0x0A, limit=full["m"] + 3)
    compare(got, exp, full["m"] + 3, offs.size + 2, True, "select planes")
    assert exp["out"].split(b"\n")[:-1] == [t[s:o + 1] for s, o in zip(starts.tolist(), offs.tolist())]
    for x in (dt, dsp, dop):
        x.free()
    m.close()
