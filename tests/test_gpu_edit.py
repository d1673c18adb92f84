"""Edit patterns on the device (acm_edit_matches_async, Matcher.scan_edit): the four planes bit for bit against the
model of tests/edit_model.py, and the three properties -- sound, unique, complete -- against a brute-force Sellers
matrix that knows nothing of pieces.  k = 1 .. 4 at n = k + 1, 3 (k + 1), 63, 64, 67, 300 and 4096; planted
insertions and deletions at the front, the end and around the only exact piece; ties in runs of one letter; spans at
T0, Tend, segment borders, `before` and an open end with the pattern's completion behind text_end; a mixed set in
both input forms; capped planes; 40 k candidates across blocks and radix digits; the refusal of the Hamming pass; a
set without edit patterns; and what -k alone misses."""
import numpy as np
import pytest

import approx_model as am
import edit_model as em
import poison
import position_model as pm
from edit_model import Edit
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16
LETTERS = np.frombuffer(b"abc", dtype=np.uint8)


def rnd(rng, n, letters=LETTERS):
    return bytes(rng.choice(letters, size=n))


def short_set():
    """k = 1 .. 4 at n = k + 1 (every piece one byte) and 3 (k + 1)"""
    rng = np.random.default_rng(2)
    return [Edit(rnd(rng, n), k) for k in range(1, 5) for n in (k + 1, 3 * (k + 1))]


def long_set():
    rng = np.random.default_rng(3)
    return [Edit(rnd(rng, 63), 1), Edit(rnd(rng, 64), 2), Edit(rnd(rng, 67), 3), Edit(rnd(rng, 300), 4), Edit(rnd(rng, 64), 4)]


def build(pats):
    a = Automaton()
    for x, p in enumerate(em.as_pats(pats)):
        if em.is_edit(p):
            a.add_edit(p.bytes, p.k, iid=x, nocase=p.nocase)
        else:
            a.add_approx(p.bytes, p.k, iid=x, nocase=p.nocase)
    a.compile()
    return a


class Env:
    def __init__(self, pats, text, max_text=16384):
        self.pats = em.as_pats(pats)
        self.model = em.EditModel(self.pats)
        self.a = build(self.pats)
        assert self.a.num_patterns == self.model.num_patterns and self.a.num_states == self.model.num_states
        self.m = Matcher(self.a, 0, max_text=max_text)
        self.text = pm.as_u8(text)
        self.states, self.offs, self.last = self.model.walk(self.text)
        self.ent_p, self.ent_o = self.model.all_entries(self.text)

    def planes(self, report, m=1 << 30):
        return (self.states[:m], self.offs[:m]) if report == em.STATE else (self.ent_p[:m], self.ent_o[:m])

    def recs(self, got):
        """(pattern x, end offset, distance, length) of the records of a call"""
        return [(self.model.owner[p], e, d, ln) for p, e, d, ln in zip(*(x.tolist() for x in got[:4]))]

    def close(self):
        self.m.close()
        self.a.close()


def upload(cells, offs, count=None, trailer=77):
    m = len(cells) if count is None else count
    sp = np.concatenate([[m], cells, [trailer]]).astype(np.int64).astype(np.int32)
    so = np.concatenate([[m], offs, [trailer]]).astype(np.int64).astype(np.int32)
    return DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(so, pad_to=0)


def text_at(text, align, tail=b""):
    """(buffer, pointer): text ++ tail on the device at an address that is `align` modulo 4, letters around it"""
    host = np.ascontiguousarray(pm.as_u8(bytes(pm.as_u8(text)) + bytes(tail)))
    buf = DeviceArray(host.size + 64)
    buf.fill(0x62)                            # 'b' all around: a read outside the text finds a letter, not a zero
    if host.size:
        _lib.check(buf.lib.acm_rt_memcpy_h2d(buf.ptr + 16 + align, host.ctypes.data, host.size, None), "h2d")
    _lib.check(buf.lib.acm_rt_stream_sync(None), "sync")
    return buf, buf.ptr + 16 + align


def run_pass(env, planes, cells, offs, report, text, origin=0, before=b"", starts=(), lead_begin=0, open_end=None, cap=None,
             max_records=None, trailer=77, align=0, dist=True, length=True, expect=None, tail=b"", what=""):
    """one call from poisoned outputs and a poisoned workspace, compared whole with the model; returns the model's
    (patterns, offsets, distances, lengths, undecided, candidates)"""
    matcher, model = env.m, env.model
    d_sp, d_so = planes
    m = len(cells)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    if expect is None:
        expect = model.records(cells[:mm], offs[:mm], report, text, origin, before, starts, lead_begin, open_end)
    ep, eo, ed, el, und, cands = expect
    last = trailer if mm == m else int(cells[mm])
    cap = ep.size + 9 if cap is None else cap
    pat, off, dst, ln = (DeviceArray((cap + SLACK) * 4) for _ in range(4))
    info = DeviceArray((4 + SLACK) * 4)
    poison.fill([pat, off, dst, ln, info], P)
    nb = matcher.lib.acm_edit_workspace_bytes(matcher.dfa, mr)
    ws = DeviceArray(nb + 256)
    ws.fill(0xA5)
    _lib.check(matcher.lib.acm_rt_stream_sync(None), "sync")
    S = len(starts)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int64).astype(np.int32), pad_to=0) if S else None
    tbuf, tptr = text_at(text, align, tail)
    bbuf, bptr = text_at(before, (align + 1) % 4) if len(before) else (None, None)
    matcher.edit_async(d_sp, d_so, mr, tptr, origin, origin + len(text), pat, off, cap, info, dist_out=dst if dist else None,
                       len_out=ln if length else None, report=report, before=bptr, before_len=len(before), seg_start=d_st,
                       segments=S, lead_begin=lead_begin, open_end=-1 if open_end is None else open_end, workspace=(ws.ptr, nb))
    what = "%s m=%d max_records=%d report=%d cap=%d S=%d align=%d" % (what, m, mr, report, cap, S, align)
    xp, xo = pm.planes(ep, eo, cap, PV, last)
    none = np.full(cap, PV, dtype=np.int32)
    xd = pm.planes(ed, ed, cap, PV, last)[0] if dist else none
    xl = pm.planes(el, el, cap, PV, last)[0] if length else none
    gp, go, gd, gl = (x.to_numpy(np.int32, cap + SLACK) for x in (pat, off, dst, ln))
    gi = info.to_numpy(np.int32, 4 + SLACK)
    assert int(gp[0]) == ep.size and int(go[0]) == ep.size, "%s: count %d/%d, model %d" % (what, gp[0], go[0], ep.size)
    for name, g, x in (("pattern", gp, xp), ("offset", go, xo), ("distance", gd, xd), ("length", gl, xl)):
        assert np.array_equal(g[:cap], x), "%s: %s plane differs at %s" % (what, name, np.flatnonzero(g[:cap] != x)[:5])
        assert (g[cap:] == PV).all(), "%s: %s plane written behind the capacity" % (what, name)
    assert gi[:4].tolist() == [und, cands, 0, 0] and (gi[4:] == PV).all(), "%s: info %s, model %s" % (what, gi[:6], (und, cands))
    assert (ws.to_numpy(np.uint8, 256, offset_bytes=nb) == 0xA5).all(), "%s: written behind the workspace" % what
    for x in (pat, off, dst, ln, info, ws, d_st, tbuf, bbuf):
        if x is not None:
            x.free()
    return expect


FORMS = [em.STATE, em.HEAD]


def both_forms(env, check=True, **kw):
    """the whole text of env through both input forms; the three properties of the records; returns the records"""
    recs = None
    for report in FORMS:
        cells, offs = env.planes(report)
        planes = upload(cells, offs)
        got = run_pass(env, planes, cells, offs, report, env.text, open_end=env.text.size, **kw)
        for x in planes:
            x.free()
        assert got[4] == 0
        assert recs is None or recs == env.recs(got)
        recs = env.recs(got)
    if check:
        em.check(env.pats, [bytes(env.text)], recs)
    return recs


def planted_found(env, where, recs):
    """every planted copy within its budget has a record near its end; the exact ones at it, with n bytes"""
    D, _ = em.brute_force(env.pats, [bytes(env.text)])
    by = {(x, e + 1): (d, ln) for x, e, d, ln in recs}
    seen = set()
    for x, name, at, v in where:
        p, e = env.pats[x], at + len(v)
        if name == "over budget":
            continue
        assert D[x][e] <= p.k, (x, name)
        hit = [by[(x, f)] for f in range(e - 2 * p.k, e + 2 * p.k + 1) if (x, f) in by]
        assert hit and min(hit)[0] <= D[x][e], (x, name, at)
        if name == "exact":
            assert by[(x, e)] == (0, p.n)
        seen |= {(name.split()[0], np.sign(ln - p.n)) for _, ln in hit}
    return seen


# ------------------------------------------------------------------ 1. k, n and the planted occurrences


@pytest.fixture(scope="module")
def short(gpu):
    pats = short_set()
    text, where = em.planted(pats, seed=5)
    e = Env(pats, text)
    e.where = where
    yield e
    e.close()


def test_short_patterns_planted(short):
    """pieces of one byte and of three: every kind of planted copy, both forms, the text at every address modulo 4"""
    recs = both_forms(short)
    seen = planted_found(short, short.where, recs)
    assert {s for _, s in seen} == {-1, 0, 1}
    cells, offs = short.planes(em.HEAD)
    planes = upload(cells, offs)
    expect = short.model.records(cells, offs, em.HEAD, short.text, open_end=short.text.size)
    for align in (1, 2, 3):
        run_pass(short, planes, cells, offs, em.HEAD, short.text, open_end=short.text.size, align=align, expect=expect)
    for x in planes:
        x.free()


def test_long_patterns_planted(gpu):
    """n = 63, 64, 67 and 300: the band walks long spans; indels in front of, behind and around the exact piece"""
    pats = long_set()
    text, where = em.planted(pats, seed=6)
    e = Env(pats, text)
    try:
        recs = both_forms(e)
        seen = planted_found(e, where, recs)
        assert {s for _, s in seen} == {-1, 0, 1} and {"only", "borders", "front", "end"} <= {n for n, _ in seen}
        by = {(x, o): (d, ln) for x, o, d, ln in recs}
        for x, name, at, v in where:                # the copies are far apart: each kind has its own record
            p = e.pats[x]
            if name == "front deleted":
                assert by[(x, at + len(v) - 1)][0] <= p.k and by[(x, at + len(v) - 1)][1] <= p.n
            if name == "over budget":
                assert not any((x, o) in by for o in range(at + len(v) - 1 - p.k, at + len(v) + p.k))
    finally:
        e.close()


def test_4096_bytes_one_occurrence(gpu):
    rng = np.random.default_rng(8)
    A = rnd(rng, 4096)
    b = am.piece_bounds(4096, 4)
    v = bytearray(A)
    v[b[4] + 9] = ord("#")                          # piece 4 substituted, piece 3 a byte longer, piece 1 a byte shorter,
    v[b[3] + 400:b[3] + 400] = b"#"                 # piece 0 substituted: piece 2 is the only exact one
    del v[b[1] + 77]
    v[5] = ord("#")
    text = rnd(rng, 41) + bytes(v) + rnd(rng, 23)
    e = Env([Edit(A, 4)], text)
    try:
        assert e.a.approx_reach == (4096 + 8, 4096 - b[1] + 4)
        recs = both_forms(e)
        assert recs == [(0, 41 + 4096 - 1, 4, 4096)]
    finally:
        e.close()


# ------------------------------------------------------------------ 2. ties and duplicates


def test_ties_in_runs_of_one_letter(gpu):
    pats = [Edit(b"aaaaaa", 2), Edit(b"ababab", 2), Edit(b"aaaaaa", 1)]
    text = b"b" + b"a" * 40 + b"cc" + b"ab" * 17 + b"c" + b"a" * 5 + b"c" + b"a" * 7 + b"b" + b"ab" * 3 + b"a"
    e = Env(pats, text)
    try:
        for report in FORMS:
            cells, offs = e.planes(report)
            planes = upload(cells, offs)
            gp, go, gd, gl, und, cands = run_pass(e, planes, cells, offs, report, e.text, open_end=e.text.size, what="ties")
            for x in planes:
                x.free()
            assert cands > gp.size, "several pieces choose the same end"
        recs = e.recs((gp, go, gd, gl))
        em.check(pats, [text], recs)
        D, _ = em.brute_force(pats, [text])
        for x in range(3):
            exact = set(np.flatnonzero(D[x] == 0).tolist())
            assert len(exact) > 10 and exact <= {o + 1 for y, o, d, ln in recs if y == x and d == 0 and ln == 6}
    finally:
        e.close()


# ------------------------------------------------------------------ 3. edges


def test_t0_and_tend(gpu):
    """an occurrence whose best start would lie in front of T0, and one whose best end would lie behind Tend"""
    A = b"abcabcab"
    pats = [Edit(A, 2)]
    text = A[2:] + b"cc" + A + b"cc" + A[:-2]          # the front cut at T0, whole, the end cut at Tend
    e = Env(pats, text)
    try:
        recs = both_forms(e)
        by = {o: (d, ln) for _, o, d, ln in recs}
        assert by[5] == (2, 6) and by[15] == (0, 8) and by[len(text) - 1] == (2, 6)
        # the same bytes as one text of a longer stream: with the bytes in front known, the cut front is whole
        cells, offs = e.model.all_entries(e.text, 2)
        planes = upload(cells, offs)
        gp, go, gd, gl, und, _ = run_pass(e, planes, cells, offs, em.HEAD, text, origin=2, before=A[:2], lead_begin=0,
                                          open_end=2 + len(text), what="before")
        assert und == 0 and (7, 0, 8) in set(zip(go.tolist(), gd.tolist(), gl.tolist()))
        # ... and with T0 at the origin the bytes of `before` are another text's: cut again
        gp, go, gd, gl, und, _ = run_pass(e, planes, cells, offs, em.HEAD, text, origin=2, before=A[:2], lead_begin=2,
                                          open_end=2 + len(text), what="before, T0 behind it")
        assert und == 0 and (7, 2, 6) in set(zip(go.tolist(), gd.tolist(), gl.tolist()))
        for x in planes:
            x.free()
    finally:
        e.close()


def test_segments(gpu):
    """an occurrence that needs one byte of the neighbouring text is not found across the border, and is within"""
    A = b"abcabcabc"
    pats = [Edit(A, 1)]
    text = b"cc" + A + b"cc" + A + b"ccc"               # the copies end at 10 and at 21
    cut = 2 + 9 + 2 + 4                                  # a border inside the second copy
    e = Env(pats, text)
    try:
        cells, offs = e.planes(em.HEAD)
        planes = upload(cells, offs)
        whole = {(10, 0, 9), (21, 0, 9)}
        for starts, want in (([0], whole), ([0, cut], {(10, 0, 9)}), ([0, cut - 4], whole), ([0, 2, 11, 13, 22], whole),
                             ([0, 3], {(10, 1, 8), (21, 0, 9)}), ([0, 14], {(10, 0, 9), (21, 1, 8)}), ([0, 21], {(10, 0, 9), (20, 1, 8)})):
            got = run_pass(e, planes, cells, offs, em.HEAD, text, starts=starts, open_end=len(text), what="segments")
            assert got[4] == 0 and set(zip(got[1].tolist(), got[2].tolist(), got[3].tolist())) == want, starts
        # the lead text with its end unknown, behind the starts' last: undecided near text_end only
        got = run_pass(e, planes, cells, offs, em.HEAD, text, starts=[0, 13], open_end=None, what="open")
        assert 10 in got[1].tolist()
        for x in planes:
            x.free()
        texts = [text[:cut], text[cut:]]
        gp, ge, gd, gl, und = e.m.scan_edit(texts=texts)
        mp, mo, md, ml, mu, _ = e.model.scan(texts)
        assert und == mu == 0 and [gp.tolist(), ge.tolist(), gd.tolist(), gl.tolist()] == [mp.tolist(), mo.tolist(), md.tolist(), ml.tolist()]
        assert 10 in ge.tolist() and 21 not in ge.tolist()
    finally:
        e.close()


def test_before_carries_the_front(short):
    text = short.text[:400]
    piece, origin = text[150:], 150
    cells, offs = short.model.all_entries(piece, origin)
    planes = upload(cells, offs)
    unds = []
    for nb in (0, 1, 3, 4, 7, 12, 23):
        got = run_pass(short, planes, cells, offs, em.HEAD, piece, origin=origin, before=bytes(text[150 - nb:150]), lead_begin=0,
                       open_end=400, align=nb % 4, what="before %d" % nb)
        unds.append(got[4])
    assert unds[0] > 0 and unds[-1] == 0 and all(x >= y for x, y in zip(unds, unds[1:]))
    for x in planes:
        x.free()


def test_open_end_reads_nothing_behind_text_end(gpu):
    """the pattern's completion lies in the buffer behind text_end: with the end withheld a piece within post + k of
    text_end is undecided, with the end known the cut copy is found with its missing bytes as errors"""
    A = b"abcabcabcabc"
    pats = [Edit(A, 2)]
    text = b"cc" + A + b"ccb" + A[:10]
    e = Env(pats, text)
    try:
        cells, offs = e.planes(em.HEAD)
        planes = upload(cells, offs)
        T = len(text)
        got = run_pass(e, planes, cells, offs, em.HEAD, text, open_end=None, tail=A[10:] + b"cc" + A, what="open end")
        assert got[4] >= 2 and got[1].tolist() == [12, 13, 14]      # (the periodic pattern's pieces choose three ends)
        got = run_pass(e, planes, cells, offs, em.HEAD, text, open_end=T, tail=A[10:] + b"cc" + A, what="known end")
        assert got[4] == 0 and (T - 1, 2, 10) in set(zip(got[1].tolist(), got[2].tolist(), got[3].tolist()))
        got = run_pass(e, planes, cells, offs, em.HEAD, text, open_end=T + 1, tail=A[10:] + b"cc" + A, what="end behind the bytes")
        assert got[4] >= 2 and got[1].tolist() == [12, 13, 14]
        for x in planes:
            x.free()
    finally:
        e.close()


# ------------------------------------------------------------------ 4. a mixed set


def test_mixed_set(gpu):
    """plain, Hamming and edit patterns, folding and exact: the automaton is mixed, its candidates fold everything"""
    pats = [Edit(b"abcaBc", 1), Edit(b"ABcabC", 2, True), (b"bCaAb", 1, False), (b"cabA", 1, True), b"Ab", (b"ca", 0, True)]
    rng = np.random.default_rng(31)
    text = bytearray(rng.choice(np.frombuffer(b"abcABC", dtype=np.uint8), size=3000, p=[.25, .25, .2, .1, .1, .1]))
    for at, t in ((100, b"abcaBc"), (200, b"abcBc"), (300, b"ABCABC"), (400, b"abc#abc"), (500, b"bCaAb"), (600, b"bCaab"), (700, b"aBcaBc")):
        text[at:at + len(t)] = t
    e = Env(pats, bytes(text))
    try:
        assert e.a.mixed_case and [e.a.approx_mode(x) for x in range(4)] == [1, 1, 0, 0]
        recs = both_forms(e)
        assert {x for x, *_ in recs} == set(range(6))
        ham = am.brute_force(pats[2:4], [bytes(text)])
        assert {(x - 2, o - e.pats[x].n + 1, d) for x, o, d, ln in recs if x in (2, 3)} == ham
        by = {(x, o): (d, ln) for x, o, d, ln in recs}
        assert by[(0, 105)] == (0, 6) and by[(0, 204)] == (1, 5) and by[(0, 705)] == (1, 6) and by[(1, 705)] == (0, 6)
    finally:
        e.close()


# ------------------------------------------------------------------ 5. the contract


def test_capacity_and_optional_planes(short):
    for report in FORMS:
        cells, offs = short.planes(report, 700)
        planes = upload(cells, offs)
        kw = dict(open_end=None, starts=[0, 300, 650])
        expect = short.model.records(cells, offs, report, short.text, **kw)
        n = expect[0].size
        assert n > 8
        for cap in (2, 3, n, n + 1, n + 2, n + 9):
            for dist, length in ((True, True), (False, True), (True, False), (False, False)):
                run_pass(short, planes, cells, offs, report, short.text, cap=cap, dist=dist, length=length, expect=expect, **kw)
        for mr in (0, 1, 699, 705):
            run_pass(short, planes, cells, offs, report, short.text, max_records=mr, **kw)
        for x in planes:
            x.free()


def test_hostile_planes(short):
    """cells that are neither states nor patterns, offsets at the ends of int32 and beyond the text, a count cell
    beyond max_records: nothing is read outside the planes, the text and the tables, and the model's records come out"""
    rng = np.random.default_rng(5)
    m, i32 = 900, 0x7FFFFFFF
    text = short.text[:500]
    edge = np.array([-(2 ** 31), -(2 ** 31) + 3, -5, -1, 0, 1, 8, 490, 498, 499, 500, 501, 509, 5000, i32 - 9, i32 - 1, i32], dtype=np.int64)
    for report in FORMS:
        good = np.unique(short.states) if report == em.STATE else np.arange(short.model.num_patterns)
        bad = np.array([-1, -(2 ** 31), i32, 0x7FFFFF00, short.model.num_patterns, short.model.num_states], dtype=np.int64)
        cells = np.concatenate([good, bad])[rng.integers(0, good.size + bad.size, m)]
        offs = np.sort(np.concatenate([edge[rng.integers(0, edge.size, m // 2)], rng.integers(0, 500, m - m // 2)]))
        for count in (m, i32, -1):
            planes = upload(cells, offs, count=count)
            for kw in (dict(open_end=None, lead_begin=-(2 ** 40)), dict(open_end=500, starts=[0, 250, 499, 500, i32]),
                       dict(open_end=2 ** 40, lead_begin=-(2 ** 31) - 50, before=b"abcabcabcabc")):
                got = run_pass(short, planes, cells, offs, report, text, what="hostile count=%d" % count, **kw)
            for x in planes:
                x.free()
        assert got[0].size > 20 and got[4] > 0


def test_scale_across_blocks_and_digits(gpu):
    """about 40 k candidates from 200 KiB: several record-pass tiles and blocks, two radix digits of patterns, three of offsets"""
    rng = np.random.default_rng(17)
    al = np.frombuffer(b"abcdefghijkl", dtype=np.uint8)
    pats = [Edit(rnd(rng, 9, al), 2) for _ in range(120)]
    text = bytearray(rng.choice(al, size=200 * 1024))
    for i in range(3000):                             # near-copies: a byte dropped, a byte added, exact
        v = bytearray(pats[i % 120].bytes)
        if i % 3 == 0:
            del v[1 + i % 7]
        elif i % 3 == 1:
            v[1 + i % 7:1 + i % 7] = b"#"
        at = 50 + 65 * i
        text[at:at + len(v)] = v
    e = Env(pats, bytes(text), max_text=1 << 18)
    try:
        assert e.a.num_patterns == 360 and e.ent_p.size > 30000
        cells, offs = e.planes(em.HEAD)
        planes = upload(cells, offs)
        got = run_pass(e, planes, cells, offs, em.HEAD, e.text, open_end=e.text.size, what="scale")
        for x in planes:
            x.free()
        recs = e.recs(got)
        assert got[5] > 3000 and len(recs) > 1000 and max(p for p in got[0].tolist()) > 256 and got[1].max() > 1 << 16
        sub = [0, 7, 119]                             # brute force for three of the patterns
        em.check([pats[x] for x in sub], [bytes(text)], [(sub.index(x), o, d, ln) for x, o, d, ln in recs if x in sub])
        gp, ge, gd, gl, und = e.m.scan_edit(bytes(text))   # the same through a STATE scan
        assert und == 0 and np.array_equal(gp, got[0]) and np.array_equal(ge, got[1]) and np.array_equal(gd, got[2]) \
            and np.array_equal(gl, got[3])
    finally:
        e.close()


def test_the_hamming_pass_refuses_edit_patterns(short):
    m = short.m
    buf, out = DeviceArray(4096), DeviceArray(4096)
    buf.fill(0)
    out.fill(P)
    ws = m.lib.acm_approx_workspace_bytes(100)
    rc = m.lib.acm_approx_matches_async(m.dfa, buf.ptr, buf.ptr, 100, 1, buf.ptr, 0, 100, None, 0, None, 0, 0, 100, out.ptr,
                                        out.ptr + 1024, None, 100, out.ptr + 2048, buf.ptr, ws, None)
    assert rc == -1 and b"acm_edit_matches_async" in m.lib.acm_last_error()
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()           # nothing was enqueued
    with pytest.raises(AcmError):
        m.scan_approx(b"abcabc")
    # the edit pass's own argument errors
    nb = m.lib.acm_edit_workspace_bytes(m.dfa, 100)
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20):
        b = m.lib.acm_edit_workspace_bytes(m.dfa, r)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    big = DeviceArray(nb)
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, mr=100, report=1, text=buf.ptr, end=100, st=buf.ptr, S=4, open=100, po=out.ptr,
                oo=out.ptr + 1024, cap=100, info=out.ptr + 2048, ws=big.ptr, nb=nb)
    for args in (dict(dfa=None), dict(sp=None), dict(so=None), dict(po=None), dict(oo=None), dict(info=None), dict(cap=1),
                 dict(nb=nb - 1), dict(ws=None), dict(report=2), dict(open=99), dict(open=-2), dict(st=None), dict(mr=0x7FFFFFFF),
                 dict(text=None)):
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_edit_matches_async(x["dfa"], x["sp"], x["so"], x["mr"], x["report"], x["text"], 0, x["end"], None, 0,
                                          x["st"], x["S"], 0, x["open"], x["po"], x["oo"], None, None, x["cap"], x["info"],
                                          x["ws"], x["nb"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()
    m.edit_async(buf, buf, 100, buf, 0, 100, out.ptr, out.ptr + 1024, 100, out.ptr + 2048, report=1, open_end=100,
                 workspace=(big.ptr, nb))                        # an empty plane: no records
    assert out.to_numpy(np.int32, 2).tolist() == [0, 0] and out.to_numpy(np.int32, 4, offset_bytes=2048).tolist() == [0, 0, 0, 0]
    for x in (buf, out, big):
        x.free()


def test_without_edit_patterns_the_normalised_hamming_pass(gpu):
    """a set of plain and Hamming patterns: the records of scan_approx, ordered by (end, pattern), with lengths"""
    pats = [(b"abcabc", 1), (b"bcabcaabc", 2), b"cab", (b"ca", 0), (b"abcab", 1, True)]
    rng = np.random.default_rng(4)
    text = bytes(rng.choice(np.frombuffer(b"abcAB", dtype=np.uint8), size=3000, p=[.3, .3, .3, .05, .05]))
    e = Env(pats, text)
    try:
        assert e.a.num_approx == 3 and [e.a.approx_mode(x) for x in range(3)] == [0, 0, 0]
        hp, he, hd, und = e.m.scan_approx(text)
        want = sorted(set(zip(he.tolist(), hp.tolist(), hd.tolist())))
        assert und == 0 and len(want) == hp.size > 300
        gp, ge, gd, gl, und = e.m.scan_edit(text)
        assert und == 0 and list(zip(ge.tolist(), gp.tolist(), gd.tolist())) == want
        assert gl.tolist() == [e.pats[e.model.owner[p]].n for p in gp.tolist()]
        both_forms(e, check=False)
    finally:
        e.close()
    # and a set with no approximate pattern at all: no table of the pass is uploaded
    a = Automaton()
    for i, p in enumerate([b"abc", b"bc", b"c"]):
        assert a.add_edit(p, 0, i) == i
    a.compile()
    m = Matcher(a, 0, max_text=4096)
    plain = Matcher(pm.build([b"abc", b"bc", b"c"], {}), 0, max_text=4096)
    assert m.device_bytes == plain.device_bytes
    gp, ge, gd, gl, und = m.scan_edit(text)
    every = m.scan_all(text)
    assert und == 0 and gp.size == every[0].size and set(gd.tolist()) == {0}
    assert sorted(zip(every[0].tolist(), every[1].tolist())) == list(zip(ge.tolist(), gp.tolist()))
    assert gl.tolist() == [[3, 2, 1][p] for p in gp.tolist()]
    for x in (m, plain, a):
        x.close()


# ------------------------------------------------------------------ 6. what -k alone misses


def test_indels_are_what_scan_approx_misses(gpu):
    A, k = b"thequickbrownfox", 2
    copies = [A, A[:5] + A[6:], A[:9] + b"w" + A[9:], A[1:], A[:3] + b"#" + A[3:12] + A[13:], A[:7] + b"#" + A[8:], A.upper()]
    text = b"....".join(copies) + b"...."
    ends, at = [], 0
    for c in copies:
        ends.append(at + len(c) - 1)
        at += len(c) + 4
    ham = Automaton()
    ham.add_approx(A, k)
    ham.compile()
    hm = Matcher(ham, 0, max_text=4096)
    hp, he, hd, und = hm.scan_approx(text)
    assert und == 0 and he.tolist() == [ends[0], ends[3], ends[5]]
    for nocase, last in ((False, []), (True, [(0, 16)])):
        ed = Automaton()
        ed.add_edit(A, k, nocase=nocase)
        ed.compile()
        m = Matcher(ed, 0, max_text=4096)
        gp, ge, gd, gl, und = m.scan_edit(text)
        got = dict(zip(ge.tolist(), zip(gd.tolist(), gl.tolist())))
        assert und == 0 and set(gp.tolist()) == {0}
        assert [got.get(e) for e in ends[:6]] == [(0, 16), (1, 15), (1, 17), (1, 15), (2, 16), (1, 16)]
        assert ([got[ends[6]]] if ends[6] in got else []) == last
        em.check([Edit(A, k, nocase)], [text], [(0, e) + got[e] for e in got])
        m.close()
        ed.close()
    hm.close()
    ham.close()
