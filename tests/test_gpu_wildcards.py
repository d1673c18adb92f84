"""Wildcard patterns on the device (acm_wildcard_matches_async, Matcher.scan_wildcards, Matcher.scan_sequences
over extended signatures), cell for cell against the model of tests/wildcard_model.py: the records of random
texts over three letters at the record counts where the record-pass core can go wrong, both input forms and
both output forms, contexts of 0 to 9 positions on either side of exact bytes, nibble sets, ??, complements and
256 interned sets, every alignment of the text; spans at the borders of the text, of `before`, of segments and
of an open end; capped planes, hostile cells, the identities of a set without contexts, determinism, a created
stream, argument errors; and end to end against brute force."""
import numpy as np
import pytest

import poison
import position_model as pm
import wildcard_model as wm
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib
from streams import Rig

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16                                   # guard cells behind every output plane
NO_CELL = 0x7FFFFF00                         # neither a state nor a pattern index
INT32_MAX = 0x7FFFFFFF
COUNTS = [1, 1023, 1024, 1025, 2049]         # the tile and block-share cuts of record_pass.h, kTile = 1024
a_, b_, c_ = 0x61, 0x62, 0x63
ANY = wm.FULL
NIB6 = frozenset(0x60 | x for x in range(16))            # 6?: every letter of the texts
NIB_1 = frozenset(x << 4 | 1 for x in range(16))         # ?1: 'a' of the letters
NIB_2 = frozenset(x << 4 | 2 for x in range(16))         # ?2: 'b'
NOT_A = ANY - {a_}
NOT_BC = ANY - {b_, c_}
MENU = [a_, b_, c_, {a_, b_}, {b_, c_}, {a_, c_}, NIB6, NIB_1, NIB_2, ANY, ANY, NOT_A, NOT_BC, NIB6, ANY]


def wild_set():
    """20 patterns with pre = k, post = 9 - k and post = k, pre = 9 - k for k = 0 .. 9 around anchors of one to
    three letters, context positions drawn from MENU; two plain patterns; then patterns whose contexts are two-byte
    sets {letter, x}, one per byte x outside the letters, until 256 sets are interned"""
    rng = np.random.default_rng(77)
    pats = []
    for k in range(10):
        for pre, post in ((k, 9 - k), (9 - k, k)):
            anchor = [int(x) for x in rng.choice([a_, b_, c_], size=int(rng.integers(1, 4)))]
            ctx = [MENU[int(rng.integers(len(MENU)))] for _ in range(pre + post)]
            # (a context that runs into the anchor would move it: its neighbours are never exact bytes)
            if pre:
                ctx[pre - 1] = {a_, b_} if isinstance(ctx[pre - 1], int) else ctx[pre - 1]
            if post:
                ctx[pre] = {b_, c_} if isinstance(ctx[pre], int) else ctx[pre]
            run = 0
            for i, s in enumerate(ctx):                      # no run of exact bytes as long as the anchor
                run = run + 1 if isinstance(s, int) else 0
                if run >= len(anchor):
                    ctx[i] = NIB6
                    run = 0
            pats.append(ctx[:pre] + anchor + ctx[pre:])
    pats += [[a_, b_], [c_]]
    used = {wm.as_set(s) for p in pats for s in p if len(wm.as_set(s)) > 1}
    extra = [frozenset((int(rng.choice([a_, b_, c_])), x)) for x in range(256) if x not in (a_, b_, c_)]
    extra = extra[:256 - len(used)]
    for k in range(0, len(extra), 4):
        grp = extra[k:k + 4]
        pats.append(grp[:2] + [[a_, b_, c_][(k // 4) % 3], [b_, c_, a_][(k // 4) % 3]] + grp[2:])
    return pats


class Env:
    def __init__(self):
        self.pats = wild_set()
        self.model = wm.WildcardModel(self.pats)
        a = Automaton()
        for i, p in enumerate(self.pats):
            assert a.add_wildcard(p, i) == i
            w = self.model.pats[i]
            assert a.pattern(i)[0] == w.anchor and a.wildcard_lengths(i) == (w.pre, w.post)
        a.compile()
        assert a.has_wildcards and a.wildcard_reach[0] >= 10 and a.wildcard_reach[1] == 9
        self.classes = len({s for p in self.model.pats for s in p.positions[:p.pre] + p.positions[p.at + p.L:] if len(s) > 1})
        assert self.classes == 256
        self.a = a
        self.m = Matcher(a, 0, max_text=4096)
        rng = np.random.default_rng(1)
        self.text = rng.choice(np.array([a_, b_, c_], dtype=np.uint8), size=2400)
        self.states, self.offs, self.last = self.model.walk(self.text)
        assert self.states.size >= 2049
        n = self.model.list_len[self.states]
        rec = np.repeat(np.arange(self.states.size), n)
        j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
        self.ent_p, self.ent_o = self.model.list[self.states[rec], j], self.offs[rec]

    def planes(self, m, report):
        if report == wm.STATE:
            return self.states[:m], self.offs[:m]
        return self.ent_p[:m], self.ent_o[:m]


@pytest.fixture(scope="module")
def env(gpu):
    e = Env()
    yield e
    e.m.close()


def upload(cells, offs, count=None, trailer=77):
    m = len(cells) if count is None else count
    sp = np.concatenate([[m], cells, [trailer]]).astype(np.int64).astype(np.int32)
    so = np.concatenate([[m], offs, [trailer]]).astype(np.int64).astype(np.int32)
    return DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(so, pad_to=0)


def text_at(text, align):
    """(buffer, pointer): the text on the device at an address that is `align` modulo 4, poison around it"""
    buf = DeviceArray(len(text) + 64)
    buf.fill(0x62)                            # 'b' all around: a read outside the text finds a letter, not a zero
    host = np.ascontiguousarray(pm.as_u8(text))
    if host.size:
        _lib.check(buf.lib.acm_rt_memcpy_h2d(buf.ptr + 16 + align, host.ctypes.data, host.size, None), "h2d")
    _lib.check(buf.lib.acm_rt_stream_sync(None), "sync")
    return buf, buf.ptr + 16 + align


def run_pass(matcher, model, planes, cells, offs, report, all_patterns, text, origin=0, before=b"", starts=(), lead_begin=0,
             open_end=None, cap=None, max_records=None, trailer=77, align=0, stream=None, what=""):
    """one call from poisoned outputs and a poisoned workspace, compared whole with the model; returns the
    model's (patterns, offsets, undecided) and the planes as read"""
    d_sp, d_so = planes
    m = len(cells)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    ep, eo, und = model.filter(cells[:mm], offs[:mm], report, all_patterns, text, origin, before, starts, lead_begin, open_end)
    last = trailer if mm == m else int(cells[mm])
    cap = ep.size + 9 if cap is None else cap
    pat, off, info = DeviceArray((cap + SLACK) * 4), DeviceArray((cap + SLACK) * 4), DeviceArray((4 + SLACK) * 4)
    poison.fill([pat, off, info], P)
    nb = matcher.lib.acm_wildcard_workspace_bytes(mr)
    ws = DeviceArray(nb + 256)
    ws.fill(0xA5)
    _lib.check(matcher.lib.acm_rt_stream_sync(None), "sync")
    S = len(starts)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int64).astype(np.int32), pad_to=0) if S else None
    tbuf, tptr = text_at(text, align)
    bbuf, bptr = text_at(before, (align + 1) % 4) if len(before) else (None, None)
    matcher.wildcard_async(d_sp, d_so, mr, tptr, origin, origin + len(text), pat, off, cap, info, report=report, before=bptr,
                           before_len=len(before), seg_start=d_st, segments=S, lead_begin=lead_begin,
                           open_end=-1 if open_end is None else open_end, all_patterns=all_patterns, workspace=(ws.ptr, nb),
                           stream=stream)
    what = "%s m=%d max_records=%d report=%d all=%d cap=%d S=%d align=%d" % (what, m, mr, report, all_patterns, cap, S, align)
    xp, xo = pm.planes(ep, eo, cap, PV, last)
    gp, go = pat.to_numpy(np.int32, cap + SLACK, stream=stream), off.to_numpy(np.int32, cap + SLACK, stream=stream)
    gi = info.to_numpy(np.int32, 4 + SLACK, stream=stream)
    assert int(gp[0]) == ep.size and int(go[0]) == ep.size, "%s: count %d/%d, model %d" % (what, gp[0], go[0], ep.size)
    assert np.array_equal(gp[:cap], xp), "%s: pattern plane differs at %s" % (what, np.flatnonzero(gp[:cap] != xp)[:5])
    assert np.array_equal(go[:cap], xo), "%s: offset plane differs at %s" % (what, np.flatnonzero(go[:cap] != xo)[:5])
    assert (gp[cap:] == PV).all() and (go[cap:] == PV).all(), "%s: written behind the capacity" % what
    assert gi[:4].tolist() == [und, 0, 0, 0] and (gi[4:] == PV).all(), "%s: info %s, undecided %d" % (what, gi[:6], und)
    assert (ws.to_numpy(np.uint8, 256, offset_bytes=nb, stream=stream) == 0xA5).all(), "%s: written behind the workspace" % what
    for x in (pat, off, info, ws, d_st, tbuf, bbuf):
        if x is not None:
            x.free()
    return ep, eo, und, (gp, go, gi)


FORMS = [(wm.STATE, True), (wm.STATE, False), (wm.HEAD, True)]


# ------------------------------------------------------------------ 1. the pass against the model


@pytest.mark.parametrize("m", COUNTS)
def test_records_against_model(env, m):
    text = env.text
    kept = 0
    for report, all_patterns in FORMS:
        cells, offs = env.planes(m, report)
        planes = upload(cells, offs)
        for align in range(4):
            ep, eo, und, _ = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, text, open_end=text.size,
                                      align=align)
            assert und == 0
        if m > 1000:
            seen = set(ep.tolist())
            assert {i for i in range(20) if i in seen} and any(i >= 22 for i in seen), "contexts of every kind are kept somewhere"
            kept += ep.size
        for x in planes:
            x.free()
    assert m < 1000 or kept > 100


def test_every_pattern_kept_and_dropped(env):
    """over the whole text: every pattern of the set has entries, the pass keeps some and drops some of almost all
    of them, and what it keeps is what a brute force over the positions finds"""
    cells, offs = env.ent_p, env.ent_o
    ep, eo, und = env.model.filter(cells, offs, wm.HEAD, True, env.text, open_end=env.text.size)
    assert set(zip(eo.tolist(), ep.tolist())) == wm.brute_force(env.model.pats, [bytes(env.text)])
    lens = [(p.pre, p.post) for p in env.model.pats[:20]]
    assert sorted(lens) == sorted([(k, 9 - k) for k in range(10)] * 2)
    had, has = set(cells.tolist()), set(ep.tolist())
    assert len(has) > 30 and len(had - has) > 3
    planes = upload(cells, offs)
    run_pass(env.m, env.model, planes, cells, offs, wm.HEAD, True, env.text, open_end=env.text.size, what="whole")
    for x in planes:
        x.free()


# ------------------------------------------------------------------ 2. spans at the borders

BORDER = [[ANY, b_, b_],                      # 0: one byte in front
          [b_, b_, NOT_A],                    # 1: one byte behind
          [{a_, c_}, ANY, b_, b_, ANY, ANY],  # 2: two in front, two behind
          [b_, b_]]                           # 3: plain


def border_env():
    a = Automaton()
    for i, p in enumerate(BORDER):
        a.add_wildcard(p, i)
    a.compile()
    return wm.WildcardModel(BORDER), Matcher(a, 0, max_text=4096)


def entries_of(model, text, origin=0):
    states, offs, _ = model.walk(text)
    n = model.list_len[states]
    rec = np.repeat(np.arange(states.size), n)
    j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
    return model.list[states[rec], j], offs[rec] + origin


def test_borders_by_hand(gpu):
    """the rule's four steps on a text small enough to read: "cxbbcbbbb" """
    model, m = border_env()
    text = b"cxbbcbbbb"
    cells, offs = entries_of(model, text)
    planes = upload(cells, offs)

    def got(**kw):
        ep, eo, und, _ = run_pass(m, model, planes, cells, offs, wm.HEAD, True, text, **kw)
        return sorted(zip(eo.tolist(), ep.tolist())), und
    # one text, its end known: bb ends at 3, 6, 7, 8
    recs, und = got(open_end=9)
    assert und == 0 and recs == [(3, 0), (3, 1), (3, 2), (3, 3), (6, 0), (6, 1), (6, 3), (7, 0), (7, 1), (7, 3), (8, 0), (8, 3)]
    # the end withheld, or beyond the bytes given: what reaches past them is undecided, whatever is there
    for open_end in (None, 12):
        recs, und = got(open_end=open_end)
        assert und == 3 and (8, 1) not in recs and (7, 2) not in recs and (8, 2) not in recs and (7, 1) in recs
    # a text that starts at 2: the byte in front of "bb" at 2 is another text's -- dropped, not undecided
    recs, und = got(open_end=9, starts=[0, 2])
    assert und == 0 and (3, 0) not in recs and (3, 2) not in recs and (3, 1) in recs and (6, 0) in recs
    # texts [0, 5) and [5, 9): "bb" + 1 behind at 3 sees 'c' inside its text; + 2 behind leaves it
    recs, und = got(open_end=9, starts=[0, 5, 5, 5, 9, 9, 40, INT32_MAX])
    assert und == 0 and (3, 1) in recs and (3, 2) not in recs and (6, 0) not in recs and (7, 0) in recs and (8, 1) not in recs
    # the piece [2, 9) alone with its lead text begun at 0: in front of it nothing is given -- undecided;
    # with `before` the bytes are there
    cells2, offs2 = entries_of(model, text[2:], 2)
    planes2 = upload(cells2, offs2)
    ep, eo, und, _ = run_pass(m, model, planes2, cells2, offs2, wm.HEAD, True, text[2:], origin=2, open_end=9)
    assert und == 2 and (3, 1) in set(zip(eo.tolist(), ep.tolist()))
    ep, eo, und, _ = run_pass(m, model, planes2, cells2, offs2, wm.HEAD, True, text[2:], origin=2, before=b"x", open_end=9)
    assert und == 1 and (3, 0) in set(zip(eo.tolist(), ep.tolist()))
    ep, eo, und, _ = run_pass(m, model, planes2, cells2, offs2, wm.HEAD, True, text[2:], origin=2, before=b"cx", open_end=9)
    assert und == 0 and {(3, 0), (3, 2)} <= set(zip(eo.tolist(), ep.tolist()))
    ep, eo, und, _ = run_pass(m, model, planes2, cells2, offs2, wm.HEAD, True, text[2:], origin=2, before=b"cx", open_end=9,
                              lead_begin=1)
    assert und == 0 and (3, 0) in set(zip(eo.tolist(), ep.tolist())) and (3, 2) not in set(zip(eo.tolist(), ep.tolist()))
    for x in planes + planes2:
        x.free()
    m.close()


def test_borders_swept(env):
    """the set of 0 .. 9 context positions over a short text with every kind of border"""
    text = env.text[:300]
    T = text.size
    seen = set()
    for report, all_patterns in FORMS:
        states, offs, _ = env.model.walk(text)
        cells, offs = (states, offs) if report == wm.STATE else entries_of(env.model, text)
        planes = upload(cells, offs)
        for kw in (dict(open_end=T), dict(open_end=T + 5), dict(open_end=None), dict(open_end=2 ** 40, lead_begin=-(2 ** 40)),
                   dict(open_end=T, lead_begin=4), dict(open_end=None, starts=[0, 50, 50, 50, 120, T - 3]),
                   dict(open_end=T, starts=[30, 31, 33, T, T, T + 7, INT32_MAX], lead_begin=-3),
                   dict(open_end=None, starts=[T + 1]), dict(open_end=T + 9, starts=[0] + [4] * 2100 + [4096])):
            ep, eo, und, _ = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, text, what="sweep", **kw)
            seen.add((report, all_patterns, und > 0))
        # a piece in the middle of a stream: `before` of 0 .. 12 bytes in front of it
        piece, origin = text[100:], 100
        st2, of2, _ = env.model.walk(piece)
        c2, o2 = (st2, of2 + origin) if report == wm.STATE else entries_of(env.model, piece, origin)
        planes2 = upload(c2, o2)
        unds = []
        for nb in (0, 1, 3, 4, 5, 9, 12):
            before = bytes(text[100 - nb:100])
            *_, und, _ = run_pass(env.m, env.model, planes2, c2, o2, report, all_patterns, piece, origin=origin, before=before,
                                  lead_begin=0, open_end=T, align=nb % 4, what="before %d" % nb)
            unds.append(und)
        assert unds[0] > 0 and unds[-1] == 0 and all(x >= y for x, y in zip(unds, unds[1:]))
        for x in planes + planes2:
            x.free()
    assert len(seen) == 6


# ------------------------------------------------------------------ 3. the contract


def test_capped_planes_and_max_records(env):
    m = 1025
    for report, all_patterns in FORMS:
        cells, offs = env.planes(m, report)
        planes = upload(cells, offs)
        kw = dict(open_end=None, starts=[0, 700, 1100])
        ep, *_ = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, env.text, **kw)
        assert ep.size > 8
        for cap in (2, ep.size + 1, ep.size, ep.size + 2):
            run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, env.text, cap=cap, **kw)
        for mr in (0, 1, 1023, 1024, m + 5):
            run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, env.text, max_records=mr, **kw)
        for x in planes:
            x.free()


def test_hostile_planes(env):
    """cells that are neither states nor patterns, offsets at the ends of int32 and beyond the text, a count cell
    beyond max_records: nothing is read outside the planes, the text and the tables, and the model's records come
    out"""
    rng = np.random.default_rng(5)
    m = 1500
    text = env.text[:1200]
    edge = np.array([-(2 ** 31), -(2 ** 31) + 3, -5, -1, 0, 1, 8, 9, 10, 1190, 1198, 1199, 1200, 1201, 1209, 5000, INT32_MAX - 9,
                     INT32_MAX - 1, INT32_MAX], dtype=np.int64)
    for report, all_patterns in FORMS:
        good = np.unique(env.states) if report == wm.STATE else np.arange(len(env.pats))
        bad = np.array([-1, -(2 ** 31), INT32_MAX, NO_CELL, len(env.pats), env.model.num_states], dtype=np.int64)
        cells = np.concatenate([good, bad])[rng.integers(0, good.size + bad.size, m)]
        offs = np.sort(np.concatenate([edge[rng.integers(0, edge.size, m // 2)], rng.integers(0, 1200, m - m // 2)]))
        for count in (m, INT32_MAX, -1):
            planes = upload(cells, offs, count=count)
            for kw in (dict(open_end=None, lead_begin=-(2 ** 40)), dict(open_end=1200, starts=[0, 600, 1199, 1200, INT32_MAX]),
                       dict(open_end=2 ** 40, lead_begin=-(2 ** 31) - 50, before=b"abcabcabcabc")):
                ep, eo, und, _ = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, text,
                                          what="hostile count=%d" % count, **kw)
            for x in planes:
                x.free()
        assert ep.size > 20 and und > 0


def test_identities_without_contexts(gpu):
    pats = [b"abc", b"bc", b"c", b"abcabc", b"cab", b"ab"]
    a = Automaton()
    for i, p in enumerate(pats):
        a.add_wildcard(list(p), i)                       # all exact: plain patterns
    a.compile()
    assert not a.has_wildcards
    rng = np.random.default_rng(4)
    text = rng.choice(np.frombuffer(b"abc.", dtype=np.uint8), size=3000)
    m = Matcher(a, 0, max_text=text.size)
    plain = Matcher(pm.build(pats, {}), 0, max_text=text.size)
    assert m.device_bytes == plain.device_bytes          # no table of the pass is uploaded
    plain.close()
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)
    head = m.scan(text)
    every = m.scan_all(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    ocap = every[0].size + 2 + 5
    k = head[0].size
    assert every[0].size > k > 500

    def poisoned():
        x = DeviceArray((ocap + SLACK) * 4)
        x.fill(P)
        return x
    ws = m.lib.acm_expand_workspace_bytes(cap - 2)
    xw, xp, xo = DeviceArray(ws), poisoned(), poisoned()
    _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, ocap,
                                              xw.ptr, ws, None), "acm_expand_matches_async")
    ex_p, ex_o = xp.to_numpy(np.int32, ocap + SLACK), xo.to_numpy(np.int32, ocap + SLACK)
    starts = DeviceArray.from_numpy(np.array([0, 100, 2000], dtype=np.int32), pad_to=0)

    def wildcard(sp, so, max_records, report, all_patterns, **kw):
        pat, off, info = poisoned(), poisoned(), DeviceArray(16)
        m.wildcard_async(sp, so, max_records, d, 0, text.size, pat, off, ocap, info, report=report, all_patterns=all_patterns, **kw)
        out = pat.to_numpy(np.int32, ocap + SLACK), off.to_numpy(np.int32, ocap + SLACK), info.to_numpy(np.int32, 4)
        for x in (pat, off, info):
            x.free()
        return out
    for kw in (dict(), dict(seg_start=starts, segments=3, lead_begin=-5, open_end=-1)):
        gp, go, gi = wildcard(m.pat_plane, m.off_plane, cap - 2, _lib.REPORT_STATE, True, **kw)
        assert np.array_equal(gp, ex_p) and np.array_equal(go, ex_o) and gi.tolist() == [0, 0, 0, 0]   # the expansion
        gp, go, gi = wildcard(xp, xo, ocap - 2, _lib.REPORT_HEAD, True, **kw)
        assert np.array_equal(gp, ex_p) and np.array_equal(go, ex_o) and gi.tolist() == [0, 0, 0, 0]   # the input
        gp, go, gi = wildcard(m.pat_plane, m.off_plane, cap - 2, _lib.REPORT_STATE, False, **kw)
        assert int(gp[0]) == k and int(go[0]) == k and gi.tolist() == [0, 0, 0, 0] and (gp[2 + k:] == PV).all()
    m.scan_async(d, text.size)                            # bit for bit, against the planes of a HEAD scan
    hp, ho = m.pat_plane.to_numpy(np.int32, k + 2), m.off_plane.to_numpy(np.int32, k + 2)
    assert np.array_equal(gp[:k + 2], hp) and np.array_equal(go[:k + 2], ho)
    for x in (d, xw, xp, xo, starts):
        x.free()
    m.close()


def test_two_runs_and_a_created_stream(env):
    rig = Rig()
    s = rig.stream()
    for report, all_patterns in FORMS:
        cells, offs = env.planes(2049, report)
        planes = upload(cells, offs)
        kw = dict(open_end=None, starts=[0, 1000, 1001, 2200], before=b"", what="stream")
        one = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, env.text, stream=s, **kw)[3]
        two = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, env.text, stream=s, **kw)[3]
        null = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, env.text, **kw)[3]
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
        b = m.lib.acm_wildcard_workspace_bytes(r)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    ws = m.lib.acm_wildcard_workspace_bytes(100)
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, max_records=100, report=1, text=buf.ptr, origin=0, end=100, before=None,
                blen=0, st=buf.ptr, S=4, lead=0, open=100, all=1, po=out.ptr, oo=out.ptr + 2048, cap=100, info=out.ptr + 1024,
                ws=buf.ptr, ws_bytes=ws)
    bad = [dict(dfa=None), dict(sp=None), dict(so=None), dict(po=None), dict(oo=None), dict(info=None), dict(cap=1),
           dict(cap=0), dict(ws_bytes=ws - 1), dict(ws=None), dict(report=2), dict(report=-1), dict(report=0, all=0),
           dict(open=99), dict(open=-2), dict(open=0), dict(st=None), dict(max_records=0x7FFFFFFF), dict(S=0x80000000),
           dict(text=None), dict(origin=101), dict(blen=4), dict(before=buf.ptr, blen=0x80000000)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_wildcard_matches_async(x["dfa"], x["sp"], x["so"], x["max_records"], x["report"], x["text"], x["origin"],
                                              x["end"], x["before"], x["blen"], x["st"], x["S"], x["lead"], x["open"], x["all"],
                                              x["po"], x["oo"], x["cap"], x["info"], x["ws"], x["ws_bytes"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()           # nothing was enqueued
    with pytest.raises(AcmError):
        m.wildcard_async(buf, buf, 100, buf, 0, 100, out, out, 1, out)
    # the same call with good arguments is accepted (an empty plane: no records), in every legal form
    for report, all_patterns, open_end in ((1, True, 100), (1, False, -1), (0, True, 1 << 40)):
        m.wildcard_async(buf, buf, 100, buf, 0, 100, out.ptr, out.ptr + 2048, 100, out.ptr + 1024, report=report,
                         seg_start=buf, segments=4, open_end=open_end, all_patterns=all_patterns)
        assert out.to_numpy(np.int32, 2).tolist() == [0, 0]
        assert out.to_numpy(np.int32, 4, offset_bytes=1024).tolist() == [0, 0, 0, 0]
    buf.free()
    out.free()


# ------------------------------------------------------------------ 4. end to end


def random_texts(seed, count=12, longest=120, alphabet=(a_, b_, c_)):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.array(alphabet, dtype=np.uint8), size=int(rng.integers(0, longest)))) for _ in range(count)] + [b""]


def test_scan_wildcards(env):
    texts = random_texts(8)
    brute = wm.brute_force(env.model.pats, texts)
    for all_patterns in (True, False):
        exp = env.model.records(texts, all_patterns)
        go, gp, last, info = env.m.scan_wildcards(texts=texts, all_patterns=all_patterns)
        assert np.array_equal(go, exp[0]) and np.array_equal(gp, exp[1]) and last == exp[2] and info.tolist() == [0, 0, 0, 0]
        if all_patterns:
            assert set(zip(go.tolist(), gp.tolist())) == brute and len(brute) > 100
    one = b"".join(texts)
    go, gp, last, info = env.m.scan_wildcards(one, all_patterns=True)
    assert set(zip(go.tolist(), gp.tolist())) == wm.brute_force(env.model.pats, [one]) and info[0] == 0
    # a piece with the bytes in front of it
    go2, gp2, _, info = env.m.scan_wildcards(one[200:], all_patterns=True, before=one[:200])
    assert info[0] == 0
    assert set(zip((go2 + 200).tolist(), gp2.tolist())) == {(o, p) for o, p in zip(go.tolist(), gp.tolist())
                                                            if o - env.model.pats[p].L + 1 >= 200}


def test_scan_wildcards_mixed_case(gpu):
    A, B = 0x41, 0x42
    pats = [([{a_, b_}, A, B, ANY], True), ([A, B, NOT_A], False), ([B, A], True), ([ANY, ANY, B, A], False)]
    model = wm.WildcardModel(pats)
    a = Automaton()
    for i, (p, nc) in enumerate(pats):
        a.add_wildcard(p, i, nocase=nc)
    a.compile()
    assert a.mixed_case and a.has_wildcards
    m = Matcher(a, 0, max_text=4096)
    texts = random_texts(3, alphabet=(a_, b_, A, B), longest=200)
    brute = wm.brute_force(model.pats, texts)
    go, gp, _, info = m.scan_wildcards(texts=texts, all_patterns=True)
    assert set(zip(go.tolist(), gp.tolist())) == brute and len(brute) > 40 and go.size == len(brute)
    assert (np.diff(go.astype(np.int64)) >= 0).all()
    fo, fp, _, _ = m.scan_wildcards(texts=texts)
    assert np.array_equal(fo, np.unique(go)) and all((o, p) in brute for o, p in zip(fo.tolist(), fp.tolist()))
    m.close()


SIGS = ["61?2*(61|62)63{1-3}6?61",            # 0: a[\x02\x12..b..]  *  [ab]c  {1-3}  [`a-o]a
        "6162??63",                            # 1: ab.c in one part
        "!(61)6263{2}61!(62|63)",              # 2: [^a]bc {2} a[^bc]
        "63??????61{-4}62(61|63)",             # 3: c...a {-4} b[ac]
        "6261"]                                # 4: plain


def sig_automaton(bodies, windows=None, nocase=()):
    a = Automaton()
    pats, seqs = [], []
    for q, body in enumerate(bodies):
        parts, gaps = wm.parse_body_ex(body)
        assert a.add_signature(body, iid=q, nocase=q in nocase, extended=True) == q
        seqs.append((list(range(len(pats), len(pats) + len(parts))), gaps))
        pats += [wm.Pattern(p, q in nocase) for p in parts]
    a.compile()
    for i, (lo, hi, fe) in (windows or {}).items():
        a.set_position(i, lo, hi, fe)
    return a, pats, seqs


@pytest.mark.parametrize("kind", ["plain", "mixed", "window"])
def test_scan_sequences_extended(gpu, kind):
    nocase = (0, 3) if kind == "mixed" else ()
    # the window on a first part counts from the part's FIRST POSITION: "[^a]bc" begins 2 .. 30 bytes into its text
    windows = {3: (2, 30, False), 5: (0, 12, True)} if kind == "window" else None
    a, pats, seqs = sig_automaton(SIGS, windows, nocase)
    assert a.has_wildcards and a.mixed_case == (kind == "mixed") and a.positioned == (kind == "window")
    m = Matcher(a, 0, max_text=4096)
    letters = (a_, b_, c_, 0x41, 0x43) if kind == "mixed" else (a_, b_, c_)
    texts = random_texts(11, count=20, longest=90, alphabet=letters)
    want = wm.span_sequences(pats, seqs, texts, windows)
    go, gq, _, _ = m.scan_sequences(texts=texts)
    got = set(zip(go.tolist(), gq.tolist()))
    assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    assert {q for _, q in want} == set(range(len(SIGS)))           # every signature matches somewhere
    if kind != "plain":
        assert want != wm.span_sequences([wm.Pattern(p.positions) for p in pats], seqs, texts)   # ... and the rule matters
    m.close()


def test_extended_and_syntax0_agree_on_gap_wildcards(gpu, tmp_path):
    """bodies whose only wildcard is ??: as positions checked by the wildcard pass and as gaps joined by the
    sequence pass they report the same (id, end offset) pairs"""
    bodies = ["6162??63", "61??62????6361", "6263*61??62", "63??61{1-2}62??61", "6162"]
    f = tmp_path / "q.sig"
    f.write_text("".join("%d:%s\n" % (10 + q, b) for q, b in enumerate(bodies)))
    texts = random_texts(13, count=25, longest=80)
    out = []
    for extended in (False, True):
        a = Automaton()
        assert a.load_signature_file(f, extended=extended) == len(bodies)
        a.compile()
        assert a.has_wildcards == extended
        iid = [a.sequence(q)[2] for q in range(a.num_sequences)]
        m = Matcher(a, 0, max_text=4096)
        go, gq, _, _ = m.scan_sequences(texts=texts)
        out.append(sorted((iid[q], o) for o, q in zip(go.tolist(), gq.tolist())))
        m.close()
    assert out[0] == out[1] and len(out[0]) > 60 and {i for i, _ in out[0]} == {10, 11, 12, 13, 14}
