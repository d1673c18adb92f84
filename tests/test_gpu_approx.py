"""Approximate patterns on the device (acm_approx_matches_async, Matcher.scan_approx), cell for cell against the
model of tests/approx_model.py: the records of a random text over three letters at the record counts where the
record-pass core can go wrong, both input forms, the text at every address modulo 4; pieces of one byte, lengths
around the word compare, uneven pieces; one pattern of 4096 bytes with mismatches on both sides of its piece
borders; folding patterns; a mixed set; spans at the borders of the text, of `before`, of segments and of an open
end; no distance plane, capped planes, hostile cells, the identities of a set without approximate patterns,
determinism, a created stream, argument errors; and end to end against brute force."""
import numpy as np
import pytest

import approx_model as am
import poison
import position_model as pm
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib
from streams import Rig

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16                                   # guard cells behind every output plane
NO_CELL = 0x7FFFFF00                         # neither a state nor a pattern index
INT32_MAX = 0x7FFFFFFF
COUNTS = [1, 1023, 1024, 1025, 2049]         # the tile and block-share cuts of record_pass.h, kTile = 1024
LETTERS = np.frombuffer(b"abc", dtype=np.uint8)

# (bytes, k): n = k + 1 (every piece one byte), n = 2 .. 9 around the word compare, uneven pieces (n % (k + 1) != 0),
# longer ones, and a plain pattern
SWEEP = [(b"ab", 1), (b"cab", 2), (b"bca", 1), (b"abca", 1), (b"cabab", 1), (b"bcabca", 2), (b"abcabca", 2),
         (b"cabcabab", 3), (b"abcacbabc", 3), (b"ca", 0), (b"abcabcabcabc", 2), (b"bcabcaabcbcabcab", 3),
         (b"abcabcaabcabbcabcabc", 4), (b"cabcabcabcabcabcabcabcab", 6)]


def substituted(p, d, rng, letters=LETTERS):
    """a copy of p with exactly d bytes replaced by another letter"""
    c = np.frombuffer(bytes(p), dtype=np.uint8).copy()
    for i in rng.choice(c.size, size=d, replace=False).tolist():
        c[i] = letters[(int(np.flatnonzero(letters == c[i])[0]) + 1) % letters.size]
    return c


def sweep_text(size=2400, seed=1, at=1300):
    """random letters, and from `at` on a copy of every approximate pattern of the sweep at every distance 0 .. k"""
    rng = np.random.default_rng(seed)
    text = rng.choice(LETTERS, size=size).copy()
    for p, k in SWEEP:
        for d in range(k + 1 if k else 0):
            c = substituted(p, d, rng)
            text[at:at + c.size] = c
            at += c.size + 1
    assert at < size
    return text


def build(pats):
    a = Automaton()
    for x, p in enumerate(pats):
        p = am.as_approx([p])[0]
        a.add_approx(p.bytes, p.k, iid=x, nocase=p.nocase)
    a.compile()
    return a


class Env:
    def __init__(self, pats=SWEEP, text=None):
        self.model = am.ApproxModel(pats)
        self.a = build(pats)
        assert self.a.num_patterns == self.model.num_patterns and self.a.num_states == self.model.num_states
        self.m = Matcher(self.a, 0, max_text=16384)
        self.text = sweep_text() if text is None else pm.as_u8(text)
        self.states, self.offs, self.last = self.model.walk(self.text)
        self.ent_p, self.ent_o = self.model.all_entries(self.text)

    def planes(self, m, report):
        if report == am.STATE:
            return self.states[:m], self.offs[:m]
        return self.ent_p[:m], self.ent_o[:m]

    def close(self):
        self.m.close()
        self.a.close()


@pytest.fixture(scope="module")
def env(gpu):
    e = Env()
    assert e.states.size >= 2049
    yield e
    e.close()


def upload(cells, offs, count=None, trailer=77):
    m = len(cells) if count is None else count
    sp = np.concatenate([[m], cells, [trailer]]).astype(np.int64).astype(np.int32)
    so = np.concatenate([[m], offs, [trailer]]).astype(np.int64).astype(np.int32)
    return DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(so, pad_to=0)


def text_at(text, align):
    """(buffer, pointer): the text on the device at an address that is `align` modulo 4, letters around it"""
    buf = DeviceArray(len(text) + 64)
    buf.fill(0x62)                            # 'b' all around: a read outside the text finds a letter, not a zero
    host = np.ascontiguousarray(pm.as_u8(text))
    if host.size:
        _lib.check(buf.lib.acm_rt_memcpy_h2d(buf.ptr + 16 + align, host.ctypes.data, host.size, None), "h2d")
    _lib.check(buf.lib.acm_rt_stream_sync(None), "sync")
    return buf, buf.ptr + 16 + align


def run_pass(matcher, model, planes, cells, offs, report, text, origin=0, before=b"", starts=(), lead_begin=0, open_end=None,
             cap=None, max_records=None, trailer=77, align=0, stream=None, dist=True, expect=None, what=""):
    """one call from poisoned outputs and a poisoned workspace, compared whole with the model; returns the
    model's (patterns, offsets, distances, undecided) and the planes as read"""
    d_sp, d_so = planes
    m = len(cells)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    if expect is None:
        expect = model.filter(cells[:mm], offs[:mm], report, text, origin, before, starts, lead_begin, open_end)
    ep, eo, ed, und = expect
    last = trailer if mm == m else int(cells[mm])
    cap = ep.size + 9 if cap is None else cap
    pat, off, dst = (DeviceArray((cap + SLACK) * 4) for _ in range(3))
    info = DeviceArray((4 + SLACK) * 4)
    poison.fill([pat, off, dst, info], P)
    nb = matcher.lib.acm_approx_workspace_bytes(mr)
    ws = DeviceArray(nb + 256)
    ws.fill(0xA5)
    _lib.check(matcher.lib.acm_rt_stream_sync(None), "sync")
    S = len(starts)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int64).astype(np.int32), pad_to=0) if S else None
    tbuf, tptr = text_at(text, align)
    bbuf, bptr = text_at(before, (align + 1) % 4) if len(before) else (None, None)
    matcher.approx_async(d_sp, d_so, mr, tptr, origin, origin + len(text), pat, off, cap, info, dist_out=dst if dist else None,
                         report=report, before=bptr, before_len=len(before), seg_start=d_st, segments=S,
                         lead_begin=lead_begin, open_end=-1 if open_end is None else open_end, workspace=(ws.ptr, nb),
                         stream=stream)
    what = "%s m=%d max_records=%d report=%d cap=%d S=%d align=%d" % (what, m, mr, report, cap, S, align)
    xp, xo = pm.planes(ep, eo, cap, PV, last)
    xd = pm.planes(ed, ed, cap, PV, last)[0] if dist else np.full(cap, PV, dtype=np.int32)
    gp, go, gd = (x.to_numpy(np.int32, cap + SLACK, stream=stream) for x in (pat, off, dst))
    gi = info.to_numpy(np.int32, 4 + SLACK, stream=stream)
    assert int(gp[0]) == ep.size and int(go[0]) == ep.size, "%s: count %d/%d, model %d" % (what, gp[0], go[0], ep.size)
    assert np.array_equal(gp[:cap], xp), "%s: pattern plane differs at %s" % (what, np.flatnonzero(gp[:cap] != xp)[:5])
    assert np.array_equal(go[:cap], xo), "%s: offset plane differs at %s" % (what, np.flatnonzero(go[:cap] != xo)[:5])
    assert np.array_equal(gd[:cap], xd), "%s: distance plane differs at %s" % (what, np.flatnonzero(gd[:cap] != xd)[:5])
    assert (gp[cap:] == PV).all() and (go[cap:] == PV).all() and (gd[cap:] == PV).all(), "%s: written behind the capacity" % what
    assert gi[:4].tolist() == [und, 0, 0, 0] and (gi[4:] == PV).all(), "%s: info %s, undecided %d" % (what, gi[:6], und)
    assert (ws.to_numpy(np.uint8, 256, offset_bytes=nb, stream=stream) == 0xA5).all(), "%s: written behind the workspace" % what
    for x in (pat, off, dst, info, ws, d_st, tbuf, bbuf):
        if x is not None:
            x.free()
    return ep, eo, ed, und, (gp, go, gd, gi)


FORMS = [am.STATE, am.HEAD]


# ------------------------------------------------------------------ 1. the pass against the model


@pytest.mark.parametrize("m", COUNTS)
def test_records_against_model(env, m):
    for report in FORMS:
        cells, offs = env.planes(m, report)
        planes = upload(cells, offs)
        expect = env.model.filter(cells, offs, report, env.text, open_end=env.text.size)
        assert expect[3] == 0
        for align in range(4):
            run_pass(env.m, env.model, planes, cells, offs, report, env.text, open_end=env.text.size, align=align, expect=expect)
        for x in planes:
            x.free()


def test_every_length_kept_and_dropped(env):
    """over the whole text: every pattern of the sweep has candidates, the pass keeps some and drops some of each
    approximate one, every distance 0 .. k of the short ones occurs, and what it keeps is what brute force finds"""
    cells, offs = env.ent_p, env.ent_o
    planes = upload(cells, offs)
    ep, eo, ed, und, _ = run_pass(env.m, env.model, planes, cells, offs, am.HEAD, env.text, open_end=env.text.size, what="whole")
    for x in planes:
        x.free()
    got = {env.model.span(p, o) + (d,) for p, o, d in zip(ep.tolist(), eo.tolist(), ed.tolist())}
    assert und == 0 and len(got) == ep.size and got == am.brute_force(SWEEP, [bytes(env.text)])
    owner = np.array(env.model.owner)
    for x, (p, k) in enumerate(SWEEP):
        had, has = int((owner[cells] == x).sum()), int((owner[ep] == x).sum())
        assert has > 0 and (k == 0 or had > has), (x, had, has)
        if 0 < k <= 3:
            assert {d for y, _, d in got if y == x} == set(range(k + 1)), x


def test_long_pattern_mismatches_at_piece_borders(gpu):
    """4096 bytes, k = 15: pieces of 256 bytes; copies with substitutions on both sides of piece borders"""
    rng = np.random.default_rng(9)
    pat = rng.choice(LETTERS, size=4096)
    b = am.piece_bounds(4096, 15)

    def copy(at):
        c = pat.copy()
        for i in at:
            c[i] = LETTERS[(int(np.flatnonzero(LETTERS == c[i])[0]) + 1) % 3]
        return c

    def noise(n):
        return rng.choice(LETTERS, size=n)
    variants = [[],                                                         # exact: reported by piece 0 alone
                [b[1] - 1, b[1], b[2] - 1, b[3]],                           # both sides of borders: pieces 0 .. 3 are hit
                [0, b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8] - 1, b[9] - 1, b[10], b[11], b[12], b[13], b[14] + 255],
                [b[i] for i in range(16)],                                  # 16: every piece hit, no candidate at all
                [b[i] for i in range(15)] + [b[14] + 1],                    # 16 with piece 15 exact: over the budget
                [4095], [0], [b[8] - 1, b[8]]]
    parts = [noise(37)]
    for v in variants:
        parts += [copy(v), noise(int(rng.integers(1, 9)))]
    text = np.concatenate(parts)
    last_at = text.size - parts[-1].size - 4096      # where the last copy begins
    e = Env([(bytes(pat), 15), (b"abcab", 1)], text=text)
    try:
        assert e.a.approx_reach == (4096, 3840)
        brute = am.brute_force(e.model.pats, [bytes(text)])
        assert sorted(d for x, _, d in brute if x == 0) == [0, 1, 1, 2, 4, 15]
        for report in FORMS:
            cells, offs = e.planes(len(e.states) if report == am.STATE else len(e.ent_p), report)
            planes = upload(cells, offs)
            for align in (0, 3):
                ep, eo, ed, und, _ = run_pass(e.m, e.model, planes, cells, offs, report, text, open_end=text.size, align=align,
                                              what="long")
            assert und == 0 and {e.model.span(p, o) + (d,) for p, o, d in zip(ep.tolist(), eo.tolist(), ed.tolist())} == brute
            # the last copy cut off by the bytes given: the candidates of its pieces 1 .. 15 (7 and 8 are not exact) are
            # undecided; with `before` in front they are decided: piece 0 is exact, so none of them reports it
            cut = last_at + 100
            tail = text[cut:]
            tp, to = e.model.all_entries(tail, cut)
            tpl = upload(tp, to)
            *_, und0, _ = run_pass(e.m, e.model, tpl, tp, to, am.HEAD, tail, origin=cut, open_end=text.size, what="cut")
            *_, und1, _ = run_pass(e.m, e.model, tpl, tp, to, am.HEAD, tail, origin=cut, before=bytes(text[cut - 300:cut]),
                                   open_end=text.size, align=1, what="cut+before")
            assert und0 >= 13 and und1 == 0
            for x in planes + tpl:
                x.free()
    finally:
        e.close()


def test_folding_patterns(gpu):
    """the fold is a..z only: '@' and '`', '[' and '{' stay different bytes"""
    pats = [(b"a@[z`A{a", 1, True), (b"A`{Za@[Z", 2, True), (b"Aa@[{`", 1, True), (b"@[{`aA@[{`aAz", 3, True)]
    alphabet = np.frombuffer(b"Aa@[{`zZ", dtype=np.uint8)
    rng = np.random.default_rng(12)
    text = rng.choice(alphabet, size=3000).copy()
    at = 5
    for p, k, _ in pats:                       # near-copies in the other case, with 0 .. k + 1 substitutions
        for d in range(k + 2):
            c = np.frombuffer(p.swapcase(), dtype=np.uint8).copy()
            for i in rng.choice(c.size, size=d, replace=False).tolist():
                c[i] = 0x40 if c[i] != 0x40 else 0x60
            text[at:at + c.size] = c
            at += c.size + 2
    e = Env(pats, text=text)
    try:
        assert e.a.nocase
        brute = am.brute_force(e.model.pats, [bytes(text)])
        assert all({d for x, _, d in brute if x == y} == set(range(k + 1)) for y, (_, k, _) in enumerate(pats))
        for report in FORMS:
            cells, offs = e.planes(1 << 30, report)
            planes = upload(cells, offs)
            for align in range(4):
                ep, eo, ed, und, _ = run_pass(e.m, e.model, planes, cells, offs, report, text, open_end=text.size, align=align,
                                              before=b"", what="fold")
            assert {e.model.span(p, o) + (d,) for p, o, d in zip(ep.tolist(), eo.tolist(), ed.tolist())} == brute
            for x in planes:
                x.free()
        # a piece of the stream with folded bytes in `before`
        cells, offs = e.model.all_entries(text[1000:], 1000)
        planes = upload(cells, offs)
        run_pass(e.m, e.model, planes, cells, offs, am.HEAD, text[1000:], origin=1000, before=bytes(text[989:1000]), open_end=3000,
                 align=2, what="fold before")
        for x in planes:
            x.free()
    finally:
        e.close()


def test_mixed_set(gpu):
    """an exact and a folding approximate pattern: the automaton is mixed, its candidates fold everything, and the
    rule alone makes the exact pattern's pieces exact again"""
    pats = [(b"abcaBc", 1, False), (b"ABcabC", 1, True), (b"bCa", 2, False)]
    rng = np.random.default_rng(31)
    text = rng.choice(np.frombuffer(b"abcABC", dtype=np.uint8), size=4000, p=[.25, .25, .2, .1, .1, .1]).copy()
    for at, t in ((100, b"abcaBc"), (200, b"abcaBa"), (300, b"ABCABC"), (400, b"abcabc"), (500, b"bCa"), (600, b"xCa")):
        text[at:at + len(t)] = np.frombuffer(t, dtype=np.uint8)
    e = Env(pats, text=text)
    try:
        assert e.a.mixed_case
        brute = am.brute_force(e.model.pats, [bytes(text)])
        assert {x for x, _, _ in brute} == {0, 1, 2}
        for report in FORMS:
            cells, offs = e.planes(1 << 30, report)
            planes = upload(cells, offs)
            ep, eo, ed, und, _ = run_pass(e.m, e.model, planes, cells, offs, report, text, open_end=text.size, what="mixed")
            assert {e.model.span(p, o) + (d,) for p, o, d in zip(ep.tolist(), eo.tolist(), ed.tolist())} == brute
            assert ep.size < (cells.size if report == am.HEAD else 10 ** 9)
            for x in planes:
                x.free()
        # candidates of the exact pattern that only match folded are dropped
        owner = np.array(e.model.owner)
        ep, *_ = e.model.filter(e.ent_p, e.ent_o, am.HEAD, text, open_end=text.size)
        assert (owner[e.ent_p] == 0).sum() > 3 * (owner[ep] == 0).sum() > 0
    finally:
        e.close()


# ------------------------------------------------------------------ 2. spans at the borders


def test_borders_by_hand(gpu):
    """the rule's steps on a text small enough to read: pattern "abcd" with k = 1, pieces "ab" and "cd" """
    e = Env([(b"abcd", 1), (b"cd", 0)], text=b"cdxabxdabcdab")
    try:
        text = bytes(e.text)
        cells, offs = e.ent_p, e.ent_o           # piece 0 = pattern 0 ("ab"), piece 1 = pattern 1 ("cd"), plain "cd" = 2
        planes = upload(cells, offs)

        def got(**kw):
            ep, eo, ed, und, _ = run_pass(e.m, e.model, planes, cells, offs, am.HEAD, text, **kw)
            return sorted(zip(eo.tolist(), ep.tolist(), ed.tolist())), und
        # one text, its end known.  "cd" at 0..1: piece 1 would begin at -2: dropped.  "ab" at 3..4 + "xd": 1 mismatch;
        # "ab" 7..8 + "cd": exact, reported by piece 0 only; "ab" at 11..12: the span leaves the text: dropped
        recs, und = got(open_end=13)
        assert und == 0 and recs == [(1, 2, 0), (4, 0, 1), (8, 0, 0), (10, 2, 0)]
        # the end withheld, or beyond the bytes given: the last "ab" is undecided
        for open_end in (None, 20):
            recs, und = got(open_end=open_end)
            assert und == 1 and recs == [(1, 2, 0), (4, 0, 1), (8, 0, 0), (10, 2, 0)]
        # a text that ends at 6: "ab" at 3..4 would need [3, 7): dropped, not undecided; and one that starts at 8
        recs, und = got(open_end=13, starts=[0, 6])
        assert und == 0 and recs == [(1, 2, 0), (8, 0, 0), (10, 2, 0)]
        recs, und = got(open_end=13, starts=[0, 8])
        assert und == 0 and recs == [(1, 2, 0), (4, 0, 1), (10, 2, 0)]
        # the same texts with the first one as the lead text
        recs, und = got(open_end=13, starts=[8], lead_begin=0)
        assert (10, 1, 1) not in recs and (8, 0, 0) not in recs and (4, 0, 1) in recs
        # the piece [9, 13) = "cdab" alone: "cd" at 9..10 is piece 1 of a span from 7, in front of the bytes given
        c2, o2 = e.model.all_entries(text[9:], 9)
        p2 = upload(c2, o2)
        ep, eo, ed, und, _ = run_pass(e.m, e.model, p2, c2, o2, am.HEAD, text[9:], origin=9, open_end=13)
        assert und == 1 and (10, 2, 0) in set(zip(eo.tolist(), ep.tolist(), ed.tolist()))     # piece 1 at 9..10 needs [7, 11)
        ep, eo, ed, und, _ = run_pass(e.m, e.model, p2, c2, o2, am.HEAD, text[9:], origin=9, before=b"b", open_end=13)
        assert und == 1
        ep, eo, ed, und, _ = run_pass(e.m, e.model, p2, c2, o2, am.HEAD, text[9:], origin=9, before=b"xb", open_end=13)
        assert und == 0 and (10, 1, 1) in set(zip(eo.tolist(), ep.tolist(), ed.tolist()))     # "xbcd": one mismatch, piece 0 not exact
        ep, eo, ed, und, _ = run_pass(e.m, e.model, p2, c2, o2, am.HEAD, text[9:], origin=9, before=b"ab", open_end=13)
        assert und == 0 and (10, 1, 0) not in set(zip(eo.tolist(), ep.tolist(), ed.tolist()))  # "abcd": piece 0 reports it
        ep, eo, ed, und, _ = run_pass(e.m, e.model, p2, c2, o2, am.HEAD, text[9:], origin=9, before=b"xb", open_end=13,
                                      lead_begin=8)
        assert und == 0 and (10, 1, 1) not in set(zip(eo.tolist(), ep.tolist(), ed.tolist()))  # the text begins at 8: dropped
        for x in planes + p2:
            x.free()
    finally:
        e.close()


def test_borders_swept(env):
    """the sweep set over a short text with every kind of border; the undecided count is the model's"""
    text = env.text[:300]
    T = text.size
    seen = set()
    for report in FORMS:
        states, offs, _ = env.model.walk(text)
        cells, offs = (states, offs) if report == am.STATE else env.model.all_entries(text)
        planes = upload(cells, offs)
        for kw in (dict(open_end=T), dict(open_end=T + 5), dict(open_end=None), dict(open_end=2 ** 40, lead_begin=-(2 ** 40)),
                   dict(open_end=T, lead_begin=4), dict(open_end=None, starts=[0, 50, 50, 50, 120, T - 3]),
                   dict(open_end=T, starts=[30, 31, 33, T, T, T + 7, INT32_MAX], lead_begin=-3),
                   dict(open_end=None, starts=[T + 1]), dict(open_end=T + 9, starts=[0] + [4] * 2100 + [4096])):
            *_, und, _ = run_pass(env.m, env.model, planes, cells, offs, report, text, what="sweep", **kw)
            seen.add((report, und > 0))
        # a piece in the middle of a stream: `before` of 0 .. 24 bytes in front of it
        piece, origin = text[100:], 100
        st2, of2, _ = env.model.walk(piece)
        c2, o2 = (st2, of2 + origin) if report == am.STATE else env.model.all_entries(piece, origin)
        planes2 = upload(c2, o2)
        unds = []
        for nb in (0, 1, 3, 4, 5, 9, 12, 24):
            before = bytes(text[100 - nb:100])
            *_, und, _ = run_pass(env.m, env.model, planes2, c2, o2, report, piece, origin=origin, before=before, lead_begin=0,
                                  open_end=T, align=nb % 4, what="before %d" % nb)
            unds.append(und)
        assert unds[0] > 0 and unds[-1] == 0 and all(x >= y for x, y in zip(unds, unds[1:]))
        for x in planes + planes2:
            x.free()
    assert len(seen) == 4


# ------------------------------------------------------------------ 3. the contract


def test_capped_planes_max_records_and_no_distance_plane(env):
    m = 1025
    for report in FORMS:
        cells, offs = env.planes(m, report)
        planes = upload(cells, offs)
        kw = dict(open_end=None, starts=[0, 700, 1100])
        expect = env.model.filter(cells, offs, report, env.text, **kw)
        assert expect[0].size > 8
        for cap in (None, 2, expect[0].size + 1, expect[0].size, expect[0].size + 2):
            for dist in (True, False):
                run_pass(env.m, env.model, planes, cells, offs, report, env.text, cap=cap, dist=dist, expect=expect, **kw)
        for mr in (0, 1, 1023, 1024, m + 5):
            run_pass(env.m, env.model, planes, cells, offs, report, env.text, max_records=mr, **kw)
        for x in planes:
            x.free()


def test_hostile_planes(env):
    """cells that are neither states nor patterns, pieces named where none matched, offsets at the ends of int32
    and beyond the text, a count cell beyond max_records: nothing is read outside the planes, the text and the
    tables, and the model's records come out"""
    rng = np.random.default_rng(5)
    m = 1500
    text = env.text[:1200]
    edge = np.array([-(2 ** 31), -(2 ** 31) + 3, -5, -1, 0, 1, 8, 9, 10, 1190, 1198, 1199, 1200, 1201, 1209, 5000, INT32_MAX - 9,
                     INT32_MAX - 1, INT32_MAX], dtype=np.int64)
    for report in FORMS:
        good = np.unique(env.states) if report == am.STATE else np.arange(env.model.num_patterns)
        bad = np.array([-1, -(2 ** 31), INT32_MAX, NO_CELL, env.model.num_patterns, env.model.num_states], dtype=np.int64)
        cells = np.concatenate([good, bad])[rng.integers(0, good.size + bad.size, m)]
        offs = np.sort(np.concatenate([edge[rng.integers(0, edge.size, m // 2)], rng.integers(0, 1200, m - m // 2)]))
        for count in (m, INT32_MAX, -1):
            planes = upload(cells, offs, count=count)
            for kw in (dict(open_end=None, lead_begin=-(2 ** 40)), dict(open_end=1200, starts=[0, 600, 1199, 1200, INT32_MAX]),
                       dict(open_end=2 ** 40, lead_begin=-(2 ** 31) - 50, before=b"abcabcabcabc")):
                ep, eo, ed, und, _ = run_pass(env.m, env.model, planes, cells, offs, report, text, what="hostile count=%d" % count,
                                              **kw)
            for x in planes:
                x.free()
        assert ep.size > 20 and und > 0


def test_identities_without_approximate_patterns(gpu):
    pats = [b"abc", b"bc", b"c", b"abcabc", b"cab", b"ab"]
    a = Automaton()
    for i, p in enumerate(pats):
        assert a.add_approx(p, 0, i) == i                # k = 0: plain patterns
    a.compile()
    assert a.num_approx == 0
    rng = np.random.default_rng(4)
    text = rng.choice(np.frombuffer(b"abc.", dtype=np.uint8), size=3000)
    m = Matcher(a, 0, max_text=text.size)
    plain = Matcher(pm.build(pats, {}), 0, max_text=text.size)
    assert m.device_bytes == plain.device_bytes          # no table of the pass is uploaded
    plain.close()
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)
    every = m.scan_all(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    n = every[0].size
    ocap = n + 2 + 5
    assert n > 500

    def poisoned():
        x = DeviceArray((ocap + SLACK) * 4)
        x.fill(P)
        return x
    ws = m.lib.acm_expand_workspace_bytes(cap - 2)
    xw, xp, xo = DeviceArray(ws), poisoned(), poisoned()
    _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, ocap,
                                              xw.ptr, ws, None), "acm_expand_matches_async")
    ex_p, ex_o = xp.to_numpy(np.int32, ocap + SLACK), xo.to_numpy(np.int32, ocap + SLACK)
    ex_d = ex_p.copy()
    ex_d[1:1 + n] = 0                                    # header and trailer as in the other planes, distances 0
    starts = DeviceArray.from_numpy(np.array([0, 100, 2000], dtype=np.int32), pad_to=0)

    def approx(sp, so, max_records, report, **kw):
        pat, off, dst, info = poisoned(), poisoned(), poisoned(), DeviceArray(16)
        m.approx_async(sp, so, max_records, d, 0, text.size, pat, off, ocap, info, dist_out=dst, report=report, **kw)
        out = tuple(x.to_numpy(np.int32, ocap + SLACK) for x in (pat, off, dst)) + (info.to_numpy(np.int32, 4),)
        for x in (pat, off, dst, info):
            x.free()
        return out
    for kw in (dict(), dict(seg_start=starts, segments=3, lead_begin=-5, open_end=-1)):
        gp, go, gd, gi = approx(m.pat_plane, m.off_plane, cap - 2, _lib.REPORT_STATE, **kw)
        assert np.array_equal(gp, ex_p) and np.array_equal(go, ex_o) and gi.tolist() == [0, 0, 0, 0]   # the expansion
        assert np.array_equal(gd, ex_d)
        gp, go, gd, gi = approx(xp, xo, ocap - 2, _lib.REPORT_HEAD, **kw)
        assert np.array_equal(gp, ex_p) and np.array_equal(go, ex_o) and gi.tolist() == [0, 0, 0, 0]   # the input
        assert np.array_equal(gd, ex_d)
    for x in (d, xw, xp, xo, starts):
        x.free()
    m.close()
    a.close()


def test_two_runs_and_a_created_stream(env):
    rig = Rig()
    s = rig.stream()
    for report in FORMS:
        cells, offs = env.planes(2049, report)
        planes = upload(cells, offs)
        kw = dict(open_end=None, starts=[0, 1000, 1001, 2200], what="stream")
        expect = env.model.filter(cells, offs, report, env.text, open_end=None, starts=[0, 1000, 1001, 2200])
        one = run_pass(env.m, env.model, planes, cells, offs, report, env.text, stream=s, expect=expect, **kw)[4]
        two = run_pass(env.m, env.model, planes, cells, offs, report, env.text, stream=s, expect=expect, **kw)[4]
        null = run_pass(env.m, env.model, planes, cells, offs, report, env.text, expect=expect, **kw)[4]
        for x, y, z in zip(one, two, null):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        for x in planes:
            x.free()
    rig.close()


def test_argument_errors(env):
    m = env.m
    buf, out = DeviceArray(4096), DeviceArray(1024 * 4)
    buf.fill(0)
    out.fill(P)
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20, 1 << 22, 0x7FFFFFFE):
        b = m.lib.acm_approx_workspace_bytes(r)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    ws = m.lib.acm_approx_workspace_bytes(100)
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, max_records=100, report=1, text=buf.ptr, origin=0, end=100, before=None,
                blen=0, st=buf.ptr, S=4, lead=0, open=100, po=out.ptr, oo=out.ptr + 2048, do=None, cap=100, info=out.ptr + 1024,
                ws=buf.ptr, ws_bytes=ws)
    bad = [dict(dfa=None), dict(sp=None), dict(so=None), dict(po=None), dict(oo=None), dict(info=None), dict(cap=1),
           dict(cap=0), dict(ws_bytes=ws - 1), dict(ws=None), dict(report=2), dict(report=-1),
           dict(open=99), dict(open=-2), dict(open=0), dict(st=None), dict(max_records=0x7FFFFFFF), dict(S=0x80000000),
           dict(text=None), dict(origin=101), dict(blen=4), dict(before=buf.ptr, blen=0x80000000)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_approx_matches_async(x["dfa"], x["sp"], x["so"], x["max_records"], x["report"], x["text"], x["origin"],
                                            x["end"], x["before"], x["blen"], x["st"], x["S"], x["lead"], x["open"], x["po"],
                                            x["oo"], x["do"], x["cap"], x["info"], x["ws"], x["ws_bytes"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()           # nothing was enqueued
    with pytest.raises(AcmError):
        m.approx_async(buf, buf, 100, buf, 0, 100, out, out, 1, out)
    # the same call with good arguments is accepted (an empty plane: no records), in every legal form
    for report, open_end, dist in ((1, 100, None), (1, -1, out.ptr + 3072), (0, 1 << 40, None)):
        m.approx_async(buf, buf, 100, buf, 0, 100, out.ptr, out.ptr + 2048, 100, out.ptr + 1024, dist_out=dist, report=report,
                       seg_start=buf, segments=4, open_end=open_end)
        assert out.to_numpy(np.int32, 2).tolist() == [0, 0]
        assert out.to_numpy(np.int32, 4, offset_bytes=1024).tolist() == [0, 0, 0, 0]
        if dist:
            assert out.to_numpy(np.int32, 2, offset_bytes=3072).tolist() == [0, 0]
    buf.free()
    out.free()


# ------------------------------------------------------------------ 4. end to end


def random_texts(seed, count=12, longest=120, alphabet=b"abc"):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=int(rng.integers(0, longest)))) for _ in range(count)] + [b""]


def as_results(model, brute):
    """brute force's (x, start, distance) as scan_approx reports them: (first piece, last byte, distance)"""
    return {(model.first[x], s + model.pats[x].n - 1, d) for x, s, d in brute}


def test_scan_approx(env):
    texts = random_texts(8)
    want = as_results(env.model, am.brute_force(SWEEP, texts))
    gp, ge, gd, und = env.m.scan_approx(texts=texts)
    got = set(zip(gp.tolist(), ge.tolist(), gd.tolist()))
    assert und == 0 and len(got) == gp.size and got == want and len(want) > 100
    one = b"".join(texts)
    want = as_results(env.model, am.brute_force(SWEEP, [one]))
    gp, ge, gd, und = env.m.scan_approx(one)
    assert und == 0 and set(zip(gp.tolist(), ge.tolist(), gd.tolist())) == want and gp.size == len(want)
    # a piece with the bytes in front of it: what begins inside `before` and ends in the piece is found by the
    # pieces that lie in the piece; what a cut piece would have reported is the caller's to carry (init_state)
    gp2, ge2, gd2, und = env.m.scan_approx(one[200:], before=one[:200])
    assert und == 0
    got2 = {(p, e + 200, d) for p, e, d in zip(gp2.tolist(), ge2.tolist(), gd2.tolist())}
    assert got2 <= want and {r for r in want if r[1] - env.model.pats[env.model.owner[r[0]]].n + 1 >= 200} <= got2


def test_scan_approx_mixed_and_folding(gpu):
    pats = [(b"abcaBc", 1, False), (b"ABcabC", 1, True), (b"bCaAb", 2, False), (b"cab", 0, True)]
    e = Env(pats, text=b"abc")
    try:
        assert e.a.mixed_case
        texts = random_texts(3, count=20, alphabet=b"abcABC", longest=300)
        texts += [b"..abcaBc..abcabc..abcaBC", b"abCABc.ABcabC", b"bCaAb.bcaAb.BCaAb.bCa"]
        want = as_results(e.model, am.brute_force(e.model.pats[:3], texts))
        gp, ge, gd, und = e.m.scan_approx(texts=texts)
        got = {r for r in zip(gp.tolist(), ge.tolist(), gd.tolist()) if r[0] != e.model.first[3]}
        assert und == 0 and got == want and len(want) > 40 and {r[0] for r in want} == set(e.model.first[:3])
        # the plain pattern is a candidate of the mixed automaton: kept as it stands (rule 1)
        folded = am.brute_force([e.model.pats[3]], texts)
        assert {(e.model.first[3], s + 2, 0) for _, s, _ in folded} == set(zip(gp.tolist(), ge.tolist(), gd.tolist())) - got
    finally:
        e.close()


def test_lists_longer_than_a_row_remembers(gpu):
    """36 patterns that share their last piece: one state lists them all, more entries than the 32 answers the
    count walk hands to the write walk"""
    heads = [bytes([x, y, z]) for x in b"abc" for y in b"abc" for z in b"abc"] + [bytes([x, y]) for x in b"abc" for y in b"abc"]
    pats = [(h + b"ab", 1) for h in heads]
    text = np.random.default_rng(41).choice(LETTERS, size=1500)
    e = Env(pats, text=text)
    try:
        assert e.model.list_len.max() >= 36
        for report in FORMS:
            cells, offs = e.planes(1 << 30, report)
            planes = upload(cells, offs)
            for dist in (True, False):
                ep, eo, ed, und, _ = run_pass(e.m, e.model, planes, cells, offs, report, text, open_end=text.size, dist=dist,
                                              what="long lists")
            assert {e.model.span(p, o) + (d,) for p, o, d in zip(ep.tolist(), eo.tolist(), ed.tolist())} == \
                am.brute_force(pats, [bytes(text)])
            for x in planes:
                x.free()
    finally:
        e.close()
