"""Match tallies on the device (acm_tally_matches_async, Matcher.tally_async, Matcher.scan_tally): every
output is compared, by exact equality of integer arrays, with tests/tally_model.py applied to the
oracle's records.  Every output array is pre-filled with 0x5A and has guard cells on both sides, so
"written whole" (zeros included) and "nothing outside" are checked by every call.

The kernel keeps class totals in LDS up to 5632 classes and uses merged global atomics above; the class
maps here have 1, 2, 5, num_patterns (198 / 2000 / 4376) and 1 << 20 classes, so both sides are run.
Segment rows are summed in LDS when rows x classes of a tile <= 2048 cells, else added per entry; the
grids here give both (2 classes on 140-byte segments; 4376 classes; a start at every byte)."""
import numpy as np
import pytest

import fixtures
import word_model as wm
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib, api
from streams import Rig
from tally_model import tally
from test_host_segments import oracle_segments, text_of

pytestmark = pytest.mark.gpu

MiB = 1 << 20
G = 64          # guard cells on either side of every output
FILL = 0x5A
BIG = 1 << 20   # classes: far above the LDS threshold


def matcher(name, max_text, plane_capacity=None):
    a = Automaton()
    path, hx, max_len = fixtures.set_source(name)
    a.load_file(path, hx, max_len)
    a.compile()
    return Matcher(a, 0, max_text=max_text, plane_capacity=plane_capacity), a


def guarded(cells, itemsize):
    b = DeviceArray((cells + 2 * G) * itemsize)
    b.fill(FILL)
    return b


def unguard(b, cells, dtype, stream=None):
    a = b.to_numpy(dtype, cells + 2 * G, stream=stream)
    v = np.frombuffer(bytes([FILL]) * np.dtype(dtype).itemsize, dtype=dtype)[0]
    assert np.all(a[:G] == v) and np.all(a[G + cells:] == v), "a guard cell was written"
    return a[G:G + cells].copy()


class Call:
    """one tally call with fresh guarded outputs; .result() reads them back"""

    def __init__(self, m, planes, mr, C, report=0, cmap=None, starts=None, rows=True, lead=True, all_patterns=False,
                 accumulate=False, stream=None, ws_fill=None, tot=None, map_tail=0, start_tail=0, launch=True):
        self.m, self.C, self.stream = m, C, stream
        self.S = 0 if starts is None else len(starts)
        self.tot = tot if tot is not None else guarded(C, 8)
        self.own_tot = tot is None
        self.bufs = []
        d_map = d_st = None
        if cmap is not None:   # map_tail / start_tail: hostile cells behind the cells the call may read
            h = np.concatenate([np.asarray(cmap, dtype=np.int32), np.full(map_tail, 3, dtype=np.int32)])
            d_map = DeviceArray.from_numpy(h, pad_to=0)
            self.bufs.append(d_map)
        if self.S:
            h = np.concatenate([np.asarray(starts, dtype=np.int32), np.full(start_tail, 7, dtype=np.int32)])
            d_st = DeviceArray.from_numpy(h, pad_to=0)
            self.bufs.append(d_st)
        self.rows = guarded(self.S * C, 4) if rows and self.S else None
        self.lead = guarded(C, 4) if lead else None
        wsb = m.lib.acm_tally_workspace_bytes(mr, C)
        ws = DeviceArray(wsb)
        if ws_fill is not None:
            ws.fill(ws_fill)
        self.bufs += [b for b in (ws, self.rows, self.lead) if b is not None]
        self.go = lambda: m.tally_async(
            planes[0], planes[1], mr, self.tot.ptr + G * 8, report=report, all_patterns=all_patterns,
            accumulate=accumulate, class_of=d_map, num_classes=C, seg_start=d_st, segments=self.S,
            seg_class=self.rows.ptr + G * 4 if self.rows is not None else None,
            lead=self.lead.ptr + G * 4 if self.lead is not None else None, workspace=(ws.ptr, wsb), stream=stream)
        if launch:
            m.lib.acm_rt_device_sync()   # (the fills ran on the NULL stream)
            self.go()

    def result(self):
        st = self.stream
        out = (unguard(self.tot, self.C, np.uint64, st),
               unguard(self.rows, self.S * self.C, np.int32, st).reshape(self.S, self.C) if self.rows is not None else None,
               unguard(self.lead, self.C, np.int32, st) if self.lead is not None else None)
        for b in self.bufs + ([self.tot] if self.own_tot else []):
            b.free()
        return out


def run(m, planes, mr, C, **kw):
    return Call(m, planes, mr, C, **kw).result()


def same(got, exp, what):
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], exp[0]), "%s: class totals differ" % what
    if got[1] is not None:
        assert got[1].shape == exp[1].shape and np.array_equal(got[1], exp[1]), "%s: segment rows differ" % what
    if got[2] is not None:
        assert np.array_equal(got[2], exp[2]), "%s: lead differs" % what


def class_maps(a):
    """name -> (class map or None, classes)"""
    P = a.num_patterns
    labels, sign = api.class_map(np.sign(a.iids()))
    return {"identity-null": (None, P), "identity": (np.arange(P, dtype=np.int32), P), "sign": (sign, len(labels)),
            "one": (np.zeros(P, dtype=np.int32), 1), "hostile": ((np.arange(P) % 7 - 1).astype(np.int32), 5),
            "big": (((np.arange(P, dtype=np.int64) * 9973 + 11) % BIG).astype(np.int32), BIG)}


def scan_planes(m, text, report, init_state=0):
    d = DeviceArray.from_numpy(np.ascontiguousarray(text, dtype=np.uint8))
    m.scan_async(d, len(text), init_state, report=report)
    m.lib.acm_rt_device_sync()
    d.free()
    return (m.pat_plane, m.off_plane), m.plane_capacity - 2


def expand(m, planes, mr, factor=8):
    cap = factor * m.plane_capacity
    wsb = m.lib.acm_expand_workspace_bytes(mr)
    ws, pat, off = DeviceArray(wsb), DeviceArray(cap * 4), DeviceArray(cap * 4)
    _lib.check(m.lib.acm_expand_matches_async(m.dfa, planes[0].ptr, planes[1].ptr, mr, pat.ptr, off.ptr, cap, ws.ptr,
                                              wsb, None), "acm_expand_matches_async")
    m.lib.acm_rt_device_sync()
    assert int(pat.to_numpy(np.int32, 1)[0]) <= cap - 2
    return (pat, off), cap - 2, ws


@pytest.mark.parametrize("name,mode", [(n, md) for n in ("tests", "sentiment", "clamav2000_m12", "clamav2000")
                                       for md in ("auto", "chain")])
def test_forms_and_class_maps(gpu, name, mode):
    m, a = matcher(name, MiB)
    assert m.set_mode(mode) == mode
    o = fixtures.oracle_for(name)
    text = text_of(name, MiB, 7)
    seg = 4096 if name.startswith("clamav") else 140
    starts = np.arange(0, text.size, seg, dtype=np.int64)
    head, every = o.scan(text), o.scan_all(text)
    assert head[0].size > 100 and every[0].size >= head[0].size
    maps = class_maps(a)
    planes, mr = scan_planes(m, text, _lib.REPORT_HEAD)
    for key, (cm, C) in maps.items():
        st = starts[:3] if C == BIG else starts   # (segments x classes must stay below 2^31)
        exp = tally(head[0], head[1], cm, C, st)
        assert exp[0].sum() > 0
        same(run(m, planes, mr, C, cmap=cm, starts=st), exp, "%s HEAD %s" % (name, key))
        same(run(m, planes, mr, C, cmap=cm), tally(head[0], head[1], cm, C), "%s HEAD %s, no segments" % (name, key))
    planes, mr = scan_planes(m, text, _lib.REPORT_STATE)
    for key in ("identity-null", "sign", "hostile", "big"):
        cm, C = maps[key]
        st = starts[:3] if C == BIG else starts
        same(run(m, planes, mr, C, report=_lib.REPORT_STATE, cmap=cm, starts=st), tally(head[0], head[1], cm, C, st),
             "%s STATE head-counted %s" % (name, key))
        exp_all = tally(every[0], every[1], cm, C, st)
        same(run(m, planes, mr, C, report=_lib.REPORT_STATE, all_patterns=True, cmap=cm, starts=st), exp_all,
             "%s STATE all patterns %s" % (name, key))
    xp, xmr, xws = expand(m, planes, mr)
    cm, C = maps["sign"]
    same(run(m, xp, xmr, C, cmap=cm, starts=starts), tally(every[0], every[1], cm, C, starts), name + " expanded planes")
    for b in xp + (xws,):
        b.free()
    m.close()


def test_sentiment_32_mib(gpu):
    n = 32 * MiB
    m, a = matcher("sentiment", n)
    o = fixtures.oracle_for("sentiment")
    text = fixtures.text_for({"kind": "words", "n": n, "seed": 81}, [])
    starts = np.arange(0, n, 140, dtype=np.int64)
    offs, pats, _ = o.scan(text)
    assert offs.size > 800000
    planes, mr = scan_planes(m, text, _lib.REPORT_HEAD)
    maps = class_maps(a)
    for key, st in (("sign", starts), ("identity-null", starts[::64]), ("big", None)):
        cm, C = maps[key]
        same(run(m, planes, mr, C, cmap=cm, starts=st), tally(offs, pats, cm, C, st), "32 MiB " + key)
    m.close()


def test_word_pass_output(gpu):
    name = "sentiment"
    m, a = matcher(name, MiB)
    model = wm.WordModel(name)
    text = wm.planted_text(model.pats, 256 * 1024, 3)
    m.reserve(text.size)
    d = DeviceArray.from_numpy(text)
    m.scan_async(d, text.size, 0, report=_lib.REPORT_STATE)
    cap = m.plane_capacity
    wp, wo = DeviceArray(cap * 4), DeviceArray(cap * 4)
    m.word_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, wp, wo, cap)
    offs, pats, _ = model.words(text)
    assert offs.size > 1000
    cm, C = class_maps(a)["sign"]
    starts = np.arange(0, text.size, 140, dtype=np.int64)
    same(run(m, (wp, wo), cap - 2, C, cmap=cm, starts=starts), tally(offs, pats, cm, C, starts), "word pass output")
    for b in (d, wp, wo):
        b.free()
    m.close()


def test_segment_grids(gpu):
    name = "sentiment"
    m, a = matcher(name, MiB)
    o = fixtures.oracle_for(name)
    text = fixtures.text_for({"kind": "words", "n": MiB, "seed": 7}, [])
    n = text.size
    front = fixtures.text_for({"kind": "words", "n": 5000, "seed": 8}, [])[:4999]   # ends inside a word or not
    init = o.scan(front)[2]
    offs, pats, _ = o.scan(text, init)
    maps = class_maps(a)
    sign, ident = maps["sign"], maps["identity-null"]
    planes, mr = scan_planes(m, text, _lib.REPORT_HEAD, init_state=init)
    grid = np.arange(0, n, 140, dtype=np.int64)
    rows = tally(offs, pats, sign[0], 2, grid)[1]
    # (the oracle finds 201 of the 7490 segments without a record: zero rows that must be written)
    assert grid.size == 7490 and 150 < int((rows.sum(axis=1) == 0).sum()) < 250, "empty segments of the 140-byte grid"
    first = int(offs[5])   # start[0] behind the first records: they are the lead
    cases = {
        "140 bytes": (grid, sign), "4 KiB x identity": (np.arange(0, n, 4096, dtype=np.int64), ident),
        "single": (np.array([0]), sign), "single x identity": (np.array([0]), ident),
        "100000 empty in front": (np.concatenate([np.zeros(100000, dtype=np.int64), grid]), sign),
        "empty runs": (np.repeat(grid, 3), sign),
        "starts beyond the text": (np.concatenate([grid, [n, n + 5, 2 * n, 2 ** 31 - 1]]), sign),
        "lead": (grid[grid > first], sign), "lead x identity": (np.array([first + 1, n // 2]), ident),
        "all lead": (np.array([n + 10]), sign),
        "a start at every byte": (np.arange(0, n, dtype=np.int64), sign),   # > 2048 starts per 1024-record tile
        "a start at every byte, lead": (np.arange(first + 1, n, dtype=np.int64), sign),
    }
    for key, (st, (cm, C)) in cases.items():
        exp = tally(offs, pats, cm, C, st)
        if "lead" in key:
            assert exp[2].sum() > 0
        same(run(m, planes, mr, C, cmap=cm, starts=st), exp, key)
        got = run(m, planes, mr, C, cmap=cm, starts=st, rows=False)   # lead without rows
        assert got[1] is None
        same(got, exp, key + ", no rows")
        same(run(m, planes, mr, C, cmap=cm, starts=st, lead=False), exp, key + ", no lead")
    # with a start at every byte the records of every 1024-record tile span more than 2048 starts
    assert offs.size > 4096 and np.diff(offs[::1024].astype(np.int64)).min() > 2048
    m.close()


def test_streaming_accumulate(gpu):
    name = "sentiment"
    m, a = matcher(name, MiB)
    o = fixtures.oracle_for(name)
    text = fixtures.text_for({"kind": "words", "n": MiB, "seed": 17}, [])
    n = text.size
    cuts = [0, 200003, 140 * 2900, 611111, 900001, n]   # (one cut on a start of the grid)
    grid = np.arange(0, n, 140, dtype=np.int64)
    cm, C = class_maps(a)["sign"]
    offs, pats, last = o.scan(text)
    exp = tally(offs, pats, cm, C, grid)
    cap = m.plane_capacity
    sets = [(m.pat_plane, m.off_plane), (DeviceArray(cap * 4), DeviceArray(cap * 4))]
    tot = guarded(C, 8)
    _lib.check(m.lib.acm_rt_memset(tot.ptr + G * 8, 0, C * 8, None), "memset")
    got_rows = np.zeros((grid.size, C), dtype=np.int64)
    prev, keep = None, []
    for i in range(5):
        lo, hi = cuts[i], cuts[i + 1]
        d = DeviceArray.from_numpy(text[lo:hi])
        keep.append(d)
        P, Q = sets[i % 2]
        b = m.make_batch(d, hi - lo, m.stream, P, Q, cap, (m.ws.ptr, m.ws_bytes), report=_lib.REPORT_HEAD,
                         init_plane=prev, init_plane_capacity=cap if prev is not None else 0)
        m.enqueue(b)
        k0, k1 = np.searchsorted(grid, [lo, hi])
        call = Call(m, (P, Q), cap - 2, C, cmap=cm, starts=grid[k0:k1] - lo, accumulate=True, tot=tot)
        _, rows, lead = call.result()
        got_rows[k0:k1] += rows
        if lead.any():
            assert k0 > 0
            got_rows[k0 - 1] += lead   # the text the previous piece ended in
        prev = P
    assert np.array_equal(unguard(tot, C, np.uint64), exp[0]), "running totals"
    assert np.array_equal(got_rows, exp[1]), "rows with the leads folded in"
    for b in keep + list(sets[1]) + [tot]:
        b.free()
    m.close()


def test_limits(gpu):
    name = "sentiment"
    o = fixtures.oracle_for(name)
    text = fixtures.text_for({"kind": "words", "n": 300000, "seed": 27}, [])
    offs, pats, _ = o.scan(text)
    starts = np.arange(0, text.size, 140, dtype=np.int64)
    m, a = matcher(name, MiB)
    cm, C = class_maps(a)["sign"]
    planes, mr = scan_planes(m, text, _lib.REPORT_HEAD)
    for k in (0, 1, 1023, 1024, 1025, 5000):   # only the first max_records records count
        same(run(m, planes, k, C, cmap=cm, starts=starts), tally(offs[:k], pats[:k], cm, C, starts), "max_records %d" % k)
    for empty in (np.zeros(4096, dtype=np.uint8), np.zeros(0, dtype=np.uint8)):   # m = 0, n = 0
        planes, mr = scan_planes(m, empty, _lib.REPORT_HEAD)
        got = run(m, planes, mr, C, cmap=cm, starts=starts[:50])
        assert not got[0].any() and not got[1].any() and not got[2].any()
    m.close()
    cap = 1000   # a plane that overflowed: the count cell says more than the plane holds
    m, a = matcher(name, MiB, plane_capacity=cap)
    planes, _ = scan_planes(m, text, _lib.REPORT_HEAD)
    assert int(m.pat_plane.to_numpy(np.int32, 1)[0]) == offs.size > cap
    same(run(m, planes, cap - 2, C, cmap=cm, starts=starts), tally(offs[:cap - 2], pats[:cap - 2], cm, C, starts),
         "overflowed plane")
    m.close()


@pytest.mark.parametrize("poison", [0xEE, 0x00, 0x7F])
def test_poisoned_inputs(gpu, poison):
    """cells behind the trailer (0x00: pattern 0 / state 0 at offset 0, valid records), the workspace, the
    class map's and the start array's cells behind the ones in use: none of them changes an output"""
    name = "sentiment"
    m, a = matcher(name, MiB)
    o = fixtures.oracle_for(name)
    text = fixtures.text_for({"kind": "words", "n": 200000, "seed": 37}, [])
    head, every = o.scan(text), o.scan_all(text)
    starts = np.arange(0, text.size, 140, dtype=np.int64)
    maps = class_maps(a)
    for report in (_lib.REPORT_HEAD, _lib.REPORT_STATE):
        m.pat_plane.fill(poison)
        m.off_plane.fill(poison)
        planes, mr = scan_planes(m, text, report)
        for key in ("sign", "identity", "big"):
            cm, C = maps[key]
            st = starts[:3] if C == BIG else starts
            got = run(m, planes, mr, C, report=report, cmap=cm, starts=st, ws_fill=0xFF, map_tail=256, start_tail=256)
            same(got, tally(head[0], head[1], cm, C, st), "poison %#x %s" % (poison, key))
            if report:
                got = run(m, planes, mr, C, report=report, all_patterns=True, cmap=cm, starts=st, ws_fill=0xA5,
                          map_tail=256, start_tail=256)
                same(got, tally(every[0], every[1], cm, C, st), "poison %#x %s, all patterns" % (poison, key))
    m.close()


def test_hostile_planes_stay_in_bounds(gpu):
    """planes that are no scan's output (random cells, offsets out of order): the outputs and nothing else
    are written, and every count is bounded by the records looked at"""
    m, a = matcher("sentiment", MiB)
    rng = np.random.default_rng(5)
    mr = 50000
    cells = rng.integers(-2 ** 31, 2 ** 31 - 1, size=mr + 2, dtype=np.int64).astype(np.int32)
    cells[::3] = rng.integers(0, a.num_patterns, size=cells[::3].size)
    offs = rng.integers(-2 ** 31, 2 ** 31 - 1, size=mr + 2, dtype=np.int64).astype(np.int32)
    cells[0] = offs[0] = mr
    P, Q = DeviceArray.from_numpy(cells, pad_to=0), DeviceArray.from_numpy(offs, pad_to=0)
    starts = np.sort(rng.integers(-2 ** 31, 2 ** 31 - 1, size=3000, dtype=np.int64))
    for report in (0, 1):
        for key, (cm, C) in class_maps(a).items():
            st = starts[:3] if C == BIG else starts
            got = run(m, (P, Q), mr, C, report=report, all_patterns=bool(report), cmap=cm, starts=st)
            assert int(got[1].sum()) + int(got[2].sum()) == int(got[0].sum())
            if not report:
                ok = (cells[1:mr + 1] >= 0) & (cells[1:mr + 1] < a.num_patterns)
                exp = tally(np.zeros(int(ok.sum())), cells[1:mr + 1][ok], cm, C)[0]
                assert np.array_equal(got[0], exp), key
    P.free()
    Q.free()
    m.close()


def test_argument_errors(gpu):
    m, a = matcher("tests", 4096)
    P = a.num_patterns
    planes, mr = scan_planes(m, np.frombuffer(b"nothing here", dtype=np.uint8), 0)
    tot, rows, lead = guarded(P, 8), guarded(4 * P, 4), guarded(P, 4)
    buf = DeviceArray(4096)
    wsb = m.lib.acm_tally_workspace_bytes(mr, P)
    base = dict(report=0, flags=0, cmap=None, C=P, st=None, S=0, tot=tot.ptr + G * 8, rows=None, lead=lead.ptr + G * 4,
                ws=buf.ptr, wsb=wsb)
    bad = [
        (dict(flags=_lib.TALLY_ALL_PATTERNS), -1), (dict(flags=8), -1), (dict(report=2), -1), (dict(tot=None), -1),
        (dict(rows=rows.ptr + G * 4), -1),                      # rows without segments
        (dict(C=P + 1), -1), (dict(C=1), -1), (dict(C=0, cmap=buf.ptr), -1),   # identity needs C = patterns; C = 0
        (dict(S=3), -1),                                        # segments without starts
        (dict(wsb=wsb - 1), -1), (dict(ws=None), -1),
        (dict(S=1 << 30, st=buf.ptr, rows=rows.ptr + G * 4), -5),   # segments x classes > 2^31 - 1
    ]
    for change, code in bad:
        k = dict(base)
        k.update(change)
        rc = m.lib.acm_tally_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, mr, k["report"], k["flags"], k["cmap"],
                                           k["C"], k["st"], k["S"], k["tot"], k["rows"], k["lead"], k["ws"], k["wsb"], None)
        assert rc == code, (change, rc)
    assert m.lib.acm_tally_matches_async(None, m.pat_plane.ptr, m.off_plane.ptr, mr, 0, 0, None, P, None, 0,
                                         tot.ptr + G * 8, None, None, buf.ptr, wsb, None) == -1
    with pytest.raises(AcmError):
        m.tally_async(m.pat_plane, m.off_plane, mr, tot.ptr + G * 8, all_patterns=True)
    m.lib.acm_rt_device_sync()
    v8 = np.frombuffer(bytes([FILL]) * 8, dtype=np.uint64)[0]
    v4 = np.frombuffer(bytes([FILL]) * 4, dtype=np.int32)[0]
    assert np.all(unguard(tot, P, np.uint64) == v8), "a refused call wrote the totals"
    assert np.all(unguard(rows, 4 * P, np.int32) == v4) and np.all(unguard(lead, P, np.int32) == v4)
    for b in (tot, rows, lead, buf):
        b.free()
    m.close()


def test_two_streams(gpu):
    name = "sentiment"
    m, a = matcher(name, MiB)
    o = fixtures.oracle_for(name)
    rig = Rig()
    cm, C = class_maps(a)["sign"]
    cap = m.plane_capacity
    jobs = []
    for i, (n, seg) in enumerate(((MiB, 140), (700001, 333))):
        text = fixtures.text_for({"kind": "words", "n": n, "seed": 47 + i}, [])
        st = rig.stream()
        d = rig.upload(text)
        P, Q = rig.buf(cap * 4), rig.buf(cap * 4)
        ws = rig.buf(m.ws_bytes)
        jobs.append((text, np.arange(0, n, seg, dtype=np.int64), st, d, P, Q, ws))
    m.lib.acm_rt_device_sync()
    calls = []
    for rounds in range(3):
        for text, starts, st, d, P, Q, ws in jobs:
            m.scan_async(d, text.size, 0, stream=st, pat_plane=P, off_plane=Q, plane_capacity=cap,
                         workspace=(ws.ptr, m.ws_bytes))
    for text, starts, st, d, P, Q, ws in jobs:
        calls.append(Call(m, (P, Q), cap - 2, C, cmap=cm, starts=starts, stream=st, launch=False))
        calls.append(Call(m, (P, Q), cap - 2, a.num_patterns, starts=starts[::50], stream=st, launch=False))
    m.lib.acm_rt_device_sync()
    for k in (0, 2, 1, 3):   # the streams' tallies interleaved, all enqueued before any is read
        calls[k].go()
    for j, (text, starts, st, d, P, Q, ws) in enumerate(jobs):
        offs, pats, _ = o.scan(text)
        same(calls[2 * j].result(), tally(offs, pats, cm, C, starts), "stream %d, sign" % j)
        same(calls[2 * j + 1].result(), tally(offs, pats, None, a.num_patterns, starts[::50]), "stream %d, identity" % j)
    rig.close()
    m.close()


@pytest.mark.parametrize("all_patterns", [False, True], ids=["head", "all"])
def test_scan_tally(gpu, all_patterns):
    name = "sentiment"
    m, a = matcher(name, MiB)
    o = fixtures.oracle_for(name)
    text = fixtures.text_for({"kind": "words", "n": 300000, "seed": 57}, [])
    texts = [bytes(text[i:i + 140]) for i in range(0, text.size, 140)] + [b"", b"x"]
    t, starts = Matcher.pack_segments(texts)
    eo, ep, _, _, elast = oracle_segments(o, t, starts, all_patterns=all_patterns)
    labels, cm = api.class_map(np.sign(a.iids()))
    got = m.scan_tally(texts, class_of=cm, all_patterns=all_patterns)
    same(got[:3], tally(eo, ep, cm, 2, starts), "scan_tally, sign")
    assert got[1].shape == (len(texts), 2) and got[3] == elast
    got = m.scan_tally((t, starts), all_patterns=all_patterns, per_text=False)
    assert got[1] is None
    same(got[:3], tally(eo, ep, None, a.num_patterns, starts), "scan_tally, identity, no rows")
    whole = o.scan_all(t) if all_patterns else o.scan(t)
    got = m.scan_tally(bytes(t), class_of=cm, num_classes=2, all_patterns=all_patterns)
    same(got[:3], tally(whole[0], whole[1], cm, 2), "scan_tally, one text")
    assert got[1] is None and got[3] == whole[2]
    m.close()
