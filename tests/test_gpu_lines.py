"""The line passes on the device (acm_line_index_async, acm_line_number_async, acm_line_select_async,
Matcher.scan_lines), through the C ABI, compared cell for cell with tests/line_model.py.  Every output
has guard cells on both sides and is pre-filled, so "written whole" (sentinels included) and "nothing
outside" are checked by every call; the text's 16-byte tail and far beyond it is filled with delimiters,
the workspace with tests/poison.py's fills."""
import numpy as np
import pytest

import fixtures
import line_model as lm
import poison
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib
from streams import Rig
from tally_model import tally
from test_host_lines import DELIMS, TEXTS, prev_cases
from test_host_segments import oracle_segments, text_of

pytestmark = pytest.mark.gpu

MiB = 1 << 20
G = 64
FILL = 0x5A
FILL32 = poison.cell(FILL)
SIZES = (0, 1, 15, 16, 17, 4095, 4097, MiB + 3, 32 * MiB)


def guarded(cells):
    b = DeviceArray((cells + 2 * G) * 4)
    b.fill(FILL)
    return b


def unguard(b, cells, stream=None):
    a = b.to_numpy(np.int32, cells + 2 * G, stream=stream)
    assert np.all(a[:G] == FILL32) and np.all(a[G + cells:] == FILL32), "a guard cell was written"
    return a[G:G + cells].copy()


def device_text(t, d):
    """t on the device, followed by delimiters up to round16 and 4 KiB beyond"""
    t = np.frombuffer(bytes(t), dtype=np.uint8) if isinstance(t, (bytes, bytearray)) else np.asarray(t, dtype=np.uint8)
    h = np.full(poison.round16(t.size) + poison.PAST_PAD, d, dtype=np.uint8)
    h[:t.size] = t
    return DeviceArray.from_numpy(h)


class Index:
    """one index call with guarded, pre-filled outputs"""

    def __init__(self, lib, t, d, origin=0, prev=-1, prev_info=None, cap=None, stream=None, ws_fill=0xFF, d_text=None,
                 launch=True):
        self.lib, self.stream = lib, stream
        self.n = len(t)
        self.cap = cap if cap is not None else self.n + 1
        self.text = d_text if d_text is not None else device_text(t, d)
        self.own_text = d_text is None
        self.out, self.info = guarded(self.cap), guarded(8)
        wsb = lib.acm_line_index_workspace_bytes(self.n)
        self.ws = DeviceArray(wsb + 256)
        self.ws.fill(ws_fill)
        self.wsb = wsb
        self.go = lambda: _lib.check(lib.acm_line_index_async(
            self.text.ptr, self.n, origin, d, prev, prev_info.info_ptr if prev_info is not None else None, self.start_ptr,
            self.cap, self.info_ptr, self.ws.ptr, wsb, stream), "acm_line_index_async")
        if launch:
            lib.acm_rt_device_sync()   # (the fills ran on the NULL stream)
            self.go()

    @property
    def info_ptr(self):
        return self.info.ptr + G * 4

    @property
    def start_ptr(self):
        return self.out.ptr + G * 4

    def result(self, ws_fill=0xFF):
        ls, info = unguard(self.out, self.cap, self.stream), unguard(self.info, 8, self.stream)
        tail = self.ws.to_numpy(np.uint8, 256, offset_bytes=self.wsb, stream=self.stream)
        assert np.all(tail == ws_fill), "a byte behind the workspace was written"
        return ls, info

    def free(self):
        for b in (self.out, self.info, self.ws) + ((self.text,) if self.own_text else ()):
            b.free()


def check_index(lib, t, d, origin=0, prev=-1, cap=None, stream=None, ws_fill=0xFF, what=""):
    ix = Index(lib, t, d, origin, prev, cap=cap, stream=stream, ws_fill=ws_fill)
    ls, info = ix.result(ws_fill)
    ix.free()
    e_ls, e_info, _ = lm.index(t, origin, d, prev, capacity=ix.cap)
    assert np.array_equal(info, e_info), "%s: info %s, expected %s" % (what, info.tolist(), e_info.tolist())
    bad = np.flatnonzero(ls != e_ls)
    assert bad.size == 0, "%s: line_start[%d] = %d, expected %d" % (what, bad[0], ls[bad[0]], e_ls[bad[0]])


def big_text(n, d, seed, density=1 / 140):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, size=n, dtype=np.uint8)
    t[t == d] = (d + 1) % 256
    t[rng.random(n) < density] = d
    return t


def test_host_grid(gpu, lib):
    for i, (t, d) in enumerate(TEXTS):
        for prev, _ in prev_cases(d):
            check_index(lib, t, d, origin=(0, 1000)[i % 2], prev=prev, ws_fill=poison.FILLS[1 + i % 2],
                        what="text %d prev %d" % (i, prev))


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, lib, n):
    rig = Rig()
    s = rig.stream()
    for j, d in enumerate(DELIMS):
        for k, dens in enumerate((1 / 140, 0.5) if n < 32 * MiB else (1 / 140,)):
            t = big_text(n, d, 3 + j, dens)
            if n:
                t[n - 1] = d if (j + k) % 2 else (d + 1) % 256
            prev = (-1, d, (d + 1) % 256)[j]
            check_index(lib, t, d, origin=j * 77, prev=prev, stream=(None, s)[(j + k) % 2], ws_fill=0xA5 if k else 0xFF,
                        what="n %d delimiter %d density %g" % (n, d, dens))
    only = np.full(n, 0x0A, dtype=np.uint8)
    check_index(lib, only, 0x0A, stream=s, what="n %d only delimiters" % n)
    check_index(lib, np.full(n, 0x41, dtype=np.uint8), 0x0A, prev=0x0A, what="n %d no delimiter" % n)
    rig.close()


@pytest.mark.parametrize("n", (17, 4097, MiB + 3))
def test_capacity_overflow(gpu, lib, n):
    t = big_text(n, 0x0A, 8, 0.2)
    m = int(lm.index(t)[1][0])
    for cap in (1, 2, m - 1, m, m + 1):
        if cap >= 1:
            check_index(lib, t, 0x0A, cap=cap, what="n %d capacity %d of %d" % (n, cap, m))


def test_three_chained_pieces(gpu, lib):
    rig = Rig()
    s = rig.stream()
    for d in DELIMS:
        for prev in (-1, 0x41):
            t = big_text(3 * MiB + 5, d, 21, 1 / 100)
            t[MiB] = d               # the first piece of the first cutting ends with a delimiter
            t[2 * MiB - 1] = (d + 1) % 256
            whole = lm.index(t, 500, d, prev)
            # (the middle piece of the first cutting is empty: it hands on what it was given)
            for cuts in (((0, MiB + 1), (MiB + 1, MiB + 1), (MiB + 1, t.size)), ((0, 777), (777, 2 * MiB), (2 * MiB, t.size))):
                exp = lm.chain([t[a:b] for a, b in cuts], 500, d, prev)
                calls, last = [], None
                for a, b in cuts:
                    last = Index(lib, t[a:b], d, 500 + a, prev, prev_info=last, stream=s, launch=False)
                    calls.append(last)
                lib.acm_rt_device_sync()
                for c in calls:      # no host sync between the three
                    c.go()
                got = [c.result() for c in calls]
                for (ls, info), (_, e_info, e_st), c in zip(got, exp, calls):
                    assert np.array_equal(info, e_info), "info %s, expected %s" % (info.tolist(), e_info.tolist())
                    full = np.full(c.cap, lm.SENTINEL, dtype=np.int32)
                    full[:e_st.size] = e_st
                    assert np.array_equal(ls, full)
                assert np.concatenate([ls[:info[0]] for ls, info in got]).tolist() == whole[2].tolist()
                assert sum(int(info[1]) for _, info in got) == int(whole[1][1])
                assert lm.stream_delims(got[2][1]) == int(got[0][1][1]) + int(got[1][1][1])
                for c in calls:
                    c.free()
    rig.close()


def matcher(name, max_text):
    a = Automaton()
    path, hx, max_len = fixtures.set_source(name)
    a.load_file(path, hx, max_len)
    a.compile()
    return Matcher(a, 0, max_text=max_text), a


def lined(name, n, seed):
    """a text of the set's kind with lines in it: every 20th space of the word corpus becomes a newline
    (about 140-byte lines); a clamav corpus has a newline every 256 bytes or so as it is"""
    t = text_of(name, n, seed).copy()
    if not name.startswith("clamav"):
        sp = np.flatnonzero(t == 0x20)
        rng = np.random.default_rng(seed)
        t[sp[rng.random(sp.size) < 0.05]] = 0x0A
    return t


def host_lines(t):
    """the lines of t split on the host, delimiter kept"""
    parts = bytes(t).split(b"\n")
    out = [p + b"\n" for p in parts[:-1]]
    if parts[-1]:
        out.append(parts[-1])
    return out


def read_planes(bufs, cap, stream=None):
    out = [b.to_numpy(np.int32, cap, stream=stream) for b in bufs]
    m = int(out[0][0])
    assert m <= cap - 2
    return m, [p[1:1 + m] for p in out], [int(p[m + 1]) for p in out]


@pytest.mark.parametrize("name", ["sentiment", "clamav2000_m12"])
def test_index_feeds_the_segment_and_tally_passes(gpu, lib, name):
    n = MiB
    m, a = matcher(name, n)
    o = fixtures.oracle_for(name)
    t = lined(name, n, 5)
    lines = host_lines(t)
    assert len(lines) > 1000
    exp = m.scan_segments(lines)                  # the same lines, split and packed on the host
    starts = np.cumsum([0] + [len(x) for x in lines[:-1]])
    orc_offs, orc_pats, orc_segs, _, _ = oracle_segments(o, t, starts)
    assert np.array_equal(exp[0], orc_offs) and np.array_equal(exp[1], orc_pats) and exp[0].size > 100
    d = device_text(t, 0x0A)
    cap = m.plane_capacity
    ix = Index(lib, t, 0x0A, d_text=d)
    m.scan_async(d, n, 0, report=_lib.REPORT_STATE)
    pat, off, seg = (DeviceArray(cap * 4) for _ in range(3))
    m.segment_async(m.pat_plane, m.off_plane, cap - 2, ix.start_ptr, ix.cap, n, pat, off, cap, seg_out=seg)
    cnt, (p, q, sg), trailers = read_planes((pat, off, seg), cap)
    assert np.array_equal(q.astype(np.uint32), exp[0]) and np.array_equal(p, exp[1]) and np.array_equal(sg, exp[2])
    assert trailers[0] == exp[3]
    # per-line tallies over the device-made starts
    rows = guarded(ix.cap)
    tot, lead = guarded(2), guarded(1)
    one = DeviceArray.from_numpy(np.zeros(a.num_patterns, dtype=np.int32), pad_to=0)
    m.tally_async(pat, off, cap - 2, tot.ptr + G * 4, class_of=one, num_classes=1, seg_start=ix.start_ptr, segments=ix.cap,
                  seg_class=rows.ptr + G * 4, lead=lead.ptr + G * 4)
    e_tot, e_rows, e_lead = tally(exp[0], exp[1], np.zeros(a.num_patterns, dtype=np.int32), 1, starts)
    got_rows = unguard(rows, ix.cap)
    assert np.array_equal(got_rows[:starts.size], e_rows[:, 0]) and not got_rows[starts.size:].any()
    assert unguard(lead, 1)[0] == 0
    assert int(unguard(tot, 2).view(np.uint64)[0]) == int(e_tot[0])
    ix.free()
    for b in (d, pat, off, seg, rows, tot, lead, one):
        b.free()
    m.close()


def run_select(lib, ix, origin, end, off_plane, max_records, invert, ocap, stream=None, ws_fill=0xA5):
    outs = [guarded(ocap) for _ in range(3)]
    wsb = lib.acm_line_select_workspace_bytes(ix.cap)
    ws = DeviceArray(wsb)
    ws.fill(ws_fill)
    lib.acm_rt_device_sync()
    _lib.check(lib.acm_line_select_async(ix.start_ptr, ix.cap, ix.info_ptr, origin, end, off_plane, max_records, invert,
                                         outs[0].ptr + G * 4, outs[1].ptr + G * 4, outs[2].ptr + G * 4, ocap, ws.ptr, wsb,
                                         stream), "acm_line_select_async")
    got = [unguard(b, ocap, stream) for b in outs]
    for b in outs + [ws]:
        b.free()
    return got


@pytest.mark.parametrize("prev", (-1, 0x41))
def test_number_and_select_over_a_scan(gpu, lib, prev):
    name, n, origin = "sentiment", MiB + 3, 4096
    m, a = matcher(name, n)
    o = fixtures.oracle_for(name)
    t = lined(name, n, 9)
    offs, pats, _ = o.scan(t)
    offs = offs.astype(np.int64) + origin
    assert offs.size > 10000
    rig = Rig()
    s = rig.stream()
    d = device_text(t, 0x0A)
    ix = Index(lib, t, 0x0A, origin, prev, stream=s, d_text=d)
    m.scan_async(d, n, 0, stream=s, offset_shift=origin)
    _, e_info, e_st = lm.index(t, origin, 0x0A, prev)
    cap = m.plane_capacity
    # the number pass over the scan's planes: the count comes from the header cell on the device
    num = guarded(cap)
    m.line_number_async(ix.start_ptr, ix.cap, ix.info_ptr, m.off_plane.ptr + 4, cap - 2, num.ptr + G * 4, d_count=m.off_plane,
                        stream=s)
    got = unguard(num, cap, s)
    assert np.array_equal(got[:offs.size], lm.number(e_st, e_info, offs))
    assert np.all(got[offs.size:] == FILL32), "a cell behind the record count was written"
    # ... and over an unsorted offset array
    rng = np.random.default_rng(4)
    any_offs = rng.integers(origin, origin + n, size=5000).astype(np.int32)
    d_any = DeviceArray.from_numpy(any_offs, pad_to=0)
    num2 = guarded(any_offs.size)
    m.line_number_async(ix.start_ptr, ix.cap, ix.info_ptr, d_any, any_offs.size, num2.ptr + G * 4, stream=s)
    assert np.array_equal(unguard(num2, any_offs.size, s), lm.number(e_st, e_info, any_offs))
    # select, both senses, with room and overflowing
    lines = lm.lines_of(e_st, e_info, origin, origin + n)[0].size
    sel = {}
    for inv in (0, 1):
        e = lm.select(e_st, e_info, origin, origin + n, offs, bool(inv))
        assert e[0].size > 100
        for ocap in (lines + 2, e[0].size + 1, 50, 2):
            got = run_select(lib, ix, origin, origin + n, m.off_plane.ptr, cap - 2, inv, ocap, stream=s)
            for g, x in zip(got, lm.planes(e, ocap, FILL32)):
                assert np.array_equal(g, x), "select invert %d capacity %d" % (inv, ocap)
        sel[inv] = set(e[0].tolist())
        # max_records bounds the records that are looked at
        part = run_select(lib, ix, origin, origin + n, m.off_plane.ptr, 100, inv, lines + 2, stream=s)
        e100 = lm.select(e_st, e_info, origin, origin + n, offs[:100], bool(inv))
        for g, x in zip(part, lm.planes(e100, lines + 2, FILL32)):
            assert np.array_equal(g, x)
    assert not (sel[0] & sel[1]) and len(sel[0] | sel[1]) == lines
    ix.free()
    for b in (d, num, num2, d_any):
        b.free()
    rig.close()
    m.close()


def test_select_small_grid(gpu, lib):
    """every host-grid text with a handful of records, both senses"""
    rng = np.random.default_rng(2)
    for i, (t, d) in enumerate(TEXTS[::5]):
        for prev, _ in prev_cases(d)[:3]:
            ix = Index(lib, t, d, 64, prev)
            _, e_info, e_st = lm.index(t, 64, d, prev)
            offs = np.sort(rng.integers(0, max(len(t), 1), size=4)) + 64 if t else np.zeros(0, dtype=np.int64)
            plane = np.concatenate([[offs.size], offs, [0]]).astype(np.int32)
            d_off = DeviceArray.from_numpy(plane, pad_to=0)
            for inv in (0, 1):
                e = lm.select(e_st, e_info, 64, 64 + len(t), offs, bool(inv))
                got = run_select(lib, ix, 64, 64 + len(t), d_off.ptr, 16, inv, len(t) + 3)
                for g, x in zip(got, lm.planes(e, len(t) + 3, FILL32)):
                    assert np.array_equal(g, x), "text %d prev %d invert %d" % (i, prev, inv)
            d_off.free()
            ix.free()


@pytest.mark.parametrize("name", ["sentiment", "clamav2000_m12"])
@pytest.mark.parametrize("per_line", [False, True])
def test_scan_lines(gpu, lib, name, per_line):
    n = 256 * 1024 + 37
    m, a = matcher(name, n)
    o = fixtures.oracle_for(name)
    t = lined(name, n, 13)
    _, e_info, e_st = lm.index(t)
    for all_patterns in (False, True):
        if per_line:
            offs, pats = oracle_segments(o, t, e_st, all_patterns=all_patterns)[:2]
        else:
            offs, pats, _ = (o.scan_all if all_patterns else o.scan)(t)
        offs = offs.astype(np.int64)
        assert offs.size > 100
        for invert in (False, True):
            p, q, ln, sel, lines = m.scan_lines(t, per_line=per_line, all_patterns=all_patterns, invert=invert)
            assert np.array_equal(q.astype(np.int64), offs) and np.array_equal(p, pats)
            assert np.array_equal(ln, 1 + lm.number(e_st, e_info, offs).astype(np.int64))
            assert ln.tolist() == [1 + bytes(t[:x]).count(b"\n") for x in offs[:50]] + ln.tolist()[50:]
            e = lm.select(e_st, e_info, 0, n, offs, invert)
            assert np.array_equal(sel, np.stack([e[0] + 1, e[1], e[2]], axis=1))
            assert lines == e_st.size
    m.close()
