"""Position constraints on the device (acm_position_matches_async, Matcher.scan_positions), cell for cell
against the model of tests/position_model.py: synthetic planes at the record counts where the record-pass
core can go wrong, both input forms (states, pattern indices) and both output forms; runs of equal offsets
across tile and block cuts; window edges on scanned text; segments, the lead text and open ends; a stream
cut at every position; composition with the case and word passes; the identities of an automaton without
constraints; argument errors."""
import functools

import numpy as np
import pytest

import poison
import position_model as pm
from gpu_pattern_matching_amd import AcmError, DeviceArray, Matcher, _lib

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16                                   # guard cells behind every output plane
NO_CELL = 0x7FFFFF00                         # neither a state nor a pattern index
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049]
BIG = 1024 * 1024 + 1025                     # 1026 tiles on 1024 blocks: a block owns two tiles, block cuts at 2048 k
INT32_MAX = 0x7FFFFFFF

# the state of "dcba" lists four patterns, of "cba" three, ...: "a" never matches (lo > hi), "ba" is counted from
# the end, "cba" from the start, "dcba" is free
SYN = [b"a", b"ba", b"cba", b"dcba"]
SYN_W = {0: (5, 2, False), 1: (8, 40, True), 2: (2, 33, False)}


class Env:
    def __init__(self):
        self.model = pm.PositionModel(SYN, SYN_W)
        self.m = Matcher(pm.build(SYN, SYN_W), 0, max_text=4096)
        self.state = [NO_CELL] + [int(self.model.walk(p)[2]) for p in SYN]          # kind -> state
        assert [int(self.model.list_len[s]) for s in self.state[1:]] == [1, 2, 3, 4]
        self.cache = {}

    def planes(self, m, report):
        """(cells int64[m], offsets int64[m]) of m records: states of random kind at offsets 4 i + 3 (a fifth
        of the cells no state), or pattern indices (a third of them none) in runs of equal offsets"""
        key = (m, report)
        if key not in self.cache:
            if m >= BIG:
                self.cache = {k: v for k, v in self.cache.items() if k[0] < BIG}
            rng = np.random.default_rng(2000 + m)
            if report == pm.STATE:
                cells = np.array(self.state, dtype=np.int64)[rng.integers(0, 5, m)]
                offs = np.arange(m, dtype=np.int64) * 4 + 3
            else:
                cells = np.array([-1, 0, 1, 2, 3, NO_CELL], dtype=np.int64)[rng.integers(0, 6, m)]
                offs = 4 * np.cumsum(rng.random(m) < 0.5) + 3
            self.cache[key] = (cells, offs)
        return self.cache[key]


@pytest.fixture(scope="module")
def env(gpu):
    e = Env()
    yield e
    e.m.close()


def caps_of(total):
    """total + 2 == cap, total + 1 == cap, total >= cap; and room to spare"""
    return sorted({max(total + 2, 2), max(total + 1, 2), max(total, 2), total + 9})


def upload(cells, offs, count=None, trailer=77):
    m = len(cells) if count is None else count
    sp = np.concatenate([[m], cells, [trailer]]).astype(np.int64).astype(np.int32)
    so = np.concatenate([[m], offs, [trailer]]).astype(np.int64).astype(np.int32)
    return DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(so, pad_to=0)


def run_pass(matcher, model, planes, cells, offs, report, all_patterns, starts=(), lead_begin=0, text_end=0, open_end=None,
             cap=None, max_records=None, trailer=77, what=""):
    """one call from poisoned outputs and a poisoned workspace, compared whole with the model; returns the
    model's (patterns, offsets, undecided)"""
    d_sp, d_so = planes
    m = len(cells)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    ep, eo, und = model.filter(cells[:mm], offs[:mm], report, all_patterns, starts, lead_begin, text_end, open_end)
    last = trailer if mm == m else int(cells[mm])
    cap = ep.size + 9 if cap is None else cap
    pat, off, info = DeviceArray((cap + SLACK) * 4), DeviceArray((cap + SLACK) * 4), DeviceArray((4 + SLACK) * 4)
    poison.fill([pat, off, info], P)
    nb = matcher.lib.acm_position_workspace_bytes(mr)
    ws = DeviceArray(max(nb, 16))
    ws.fill(0xA5)
    S = len(starts)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int64).astype(np.int32), pad_to=0) if S else None
    matcher.position_async(d_sp, d_so, mr, pat, off, cap, info, report=report, seg_start=d_st, segments=S,
                           lead_begin=lead_begin, text_end=text_end, open_end=-1 if open_end is None else open_end,
                           all_patterns=all_patterns, workspace=(ws.ptr, nb))
    what = "%s m=%d max_records=%d report=%d all=%d cap=%d S=%d" % (what, m, mr, report, all_patterns, cap, S)
    xp, xo = pm.planes(ep, eo, cap, PV, last)
    gp, go = pat.to_numpy(np.int32, cap + SLACK), off.to_numpy(np.int32, cap + SLACK)
    gi = info.to_numpy(np.int32, 4 + SLACK)
    assert int(gp[0]) == ep.size and int(go[0]) == ep.size, "%s: count %d/%d, model %d" % (what, gp[0], go[0], ep.size)
    assert np.array_equal(gp[:cap], xp), "%s: pattern plane differs at %s" % (what, np.flatnonzero(gp[:cap] != xp)[:5])
    assert np.array_equal(go[:cap], xo), "%s: offset plane differs at %s" % (what, np.flatnonzero(go[:cap] != xo)[:5])
    assert (gp[cap:] == PV).all() and (go[cap:] == PV).all(), "%s: written behind the capacity" % what
    assert gi[:4].tolist() == [und, 0, 0, 0] and (gi[4:] == PV).all(), "%s: info %s, undecided %d" % (what, gi[:6], und)
    for x in (pat, off, info, ws, d_st):
        if x is not None:
            x.free()
    return ep, eo, und


def syn_starts(text_end):
    """a text every 48 bytes from 48 on (the records in front are the lead's) over three quarters of the stream,
    the last text open, and two sentinels beyond the end"""
    return list(range(48, 3 * text_end // 4, 48)) + [text_end + 100, INT32_MAX]


def end_of(offs):
    return int(offs[-1]) + 1 if len(offs) else 4


# ------------------------------------------------------------------ 1. synthetic planes


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_synthetic_planes(env, m):
    for report in (pm.STATE, pm.HEAD):
        cells, offs = env.planes(m, report)
        planes = upload(cells, offs)
        text_end = end_of(offs)
        for all_patterns in (False, True):
            kw = dict(starts=syn_starts(text_end), lead_begin=-20, text_end=text_end, open_end=None)
            ep, _, und = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, **kw)
            if m >= 257:
                assert 0 < ep.size and und > 0
            if m == BIG:
                continue
            for cap in caps_of(ep.size):
                run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, cap=cap, **kw)
            for mr in sorted({max(m - 1, 0), m + 5}):
                run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, max_records=mr, **kw)
        for x in planes:
            x.free()


def test_list_across_the_cut(env):
    """a STATE record whose list writes entries on both sides of the cap - 2 cut"""
    m = 257
    cells, offs = env.planes(m, pm.STATE)
    kw = dict(starts=syn_starts(4 * m), lead_begin=-20, text_end=4 * m, open_end=4 * m)
    _, eo, _ = env.model.filter(cells, offs, pm.STATE, True, **kw)
    i = int(np.flatnonzero(eo[1:] == eo[:-1])[-1])      # entries i and i + 1 are one record's
    planes = upload(cells, offs)
    run_pass(env.m, env.model, planes, cells, offs, pm.STATE, True, cap=i + 1 + 2, **kw)
    for x in planes:
        x.free()


def test_hostile_planes(env):
    """cells that are neither states nor patterns, offsets at the ends of int32, a count cell beyond
    max_records: nothing is read outside the planes and the tables and the model's records come out.  Offsets
    out of order are outside the contract: nothing may be written outside the planes, whatever comes out."""
    rng = np.random.default_rng(5)
    m = 1500
    edge = np.array([-(2 ** 31), -5, 0, 1, 47, 48, 49, 3000, 6003, 6004, INT32_MAX], dtype=np.int64)
    many = [0] + [4] * 2100 + [4096]
    for report in (pm.STATE, pm.HEAD):
        good = env.state[1:] if report == pm.STATE else [0, 1, 2, 3]
        cells = np.array(good + [-1, -(2 ** 31), INT32_MAX, NO_CELL, 4, 5], dtype=np.int64)[rng.integers(0, 10, m)]
        offs = np.sort(np.concatenate([edge[rng.integers(0, 11, m // 2)], rng.integers(0, 6004, m - m // 2)]))
        for count in (m, INT32_MAX, -1):
            planes = upload(cells, offs, count=count)
            for all_patterns in (False, True):
                for starts in ([], syn_starts(6004), many):
                    run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, starts=starts, lead_begin=-7,
                             text_end=4 * m + 4, open_end=None, what="hostile count=%d" % count)
            for x in planes:
                x.free()
        wild = rng.permutation(offs)
        planes = upload(cells, wild)
        d_st = DeviceArray.from_numpy(np.array(many, dtype=np.int32), pad_to=0)
        nb = env.m.lib.acm_position_workspace_bytes(m)
        for all_patterns in (False, True):
            for cap in (2, 700, 8 * m):
                bufs = [DeviceArray((cap + SLACK) * 4), DeviceArray((cap + SLACK) * 4), DeviceArray((4 + SLACK) * 4),
                        DeviceArray(nb)]
                poison.fill(bufs, P)
                env.m.position_async(planes[0], planes[1], m, bufs[0], bufs[1], cap, bufs[2], report=report, seg_start=d_st,
                                     segments=len(many), lead_begin=-7, text_end=4 * m + 4, open_end=-1,
                                     all_patterns=all_patterns, workspace=(bufs[3].ptr, nb))
                gp, go = bufs[0].to_numpy(np.int32, cap + SLACK), bufs[1].to_numpy(np.int32, cap + SLACK)
                gi = bufs[2].to_numpy(np.int32, 4 + SLACK)
                assert 0 <= gp[0] == go[0] <= 4 * m and (gp[cap:] == PV).all() and (go[cap:] == PV).all()
                assert (gp[min(int(gp[0]) + 2, cap):cap] == PV).all() and gp[min(int(gp[0]) + 1, cap - 1)] == 77
                assert gi[0] >= 0 and gi[1:4].tolist() == [0, 0, 0] and (gi[4:] == PV).all()
                for x in bufs:
                    x.free()
        for x in planes + (d_st,):
            x.free()


# ------------------------------------------------------------------ 2. runs of HEAD input across the cuts


FIRST_KEPT_BEFORE = [0, 0, 3, 3, 0, 3]          # laid from cut - 3: dropped, dropped, kept | kept, dropped, kept
FIRST_KEPT_BEHIND = [0, 0, 0, 0, 0, 3, 3]       # laid from cut - 5: every entry in front of the cut is dropped


def plant(cells, offs, at, pats):
    """records at .. at + len(pats) - 1 become one run of their own, with these patterns"""
    k = len(pats)
    offs[at:] += 4
    cells[at:at + k] = pats
    offs[at:at + k] = offs[at]
    offs[at + k:] = np.maximum(offs[at + k:], offs[at] + 4)


@pytest.mark.parametrize("m,cuts", [(2060, [(1024, 0), (2048, 1)]),
                                    (BIG, [(1024, 0), (2048 * 100, 0), (2048 * 300 + 1024, 1), (2048 * 512, 1)])],
                         ids=["tiles", "blocks"])
def test_head_runs_across_cuts(env, m, cuts):
    """a run of equal offsets laid across a tile cut (1024 k) or a block cut (2048 k of the big count): its first
    entries are dropped ("a" never matches), "dcba" (free) is kept; the first form writes one record of the run"""
    cells, offs = (x.copy() for x in env.planes(m, pm.HEAD))
    where = []
    for c, kind in cuts:
        pats = FIRST_KEPT_BEHIND if kind else FIRST_KEPT_BEFORE
        at = c - (5 if kind else 3)
        plant(cells, offs, at, pats)
        where.append((at, pats.count(3)))
    assert (np.diff(offs) >= 0).all()
    planes = upload(cells, offs)
    kw = dict(starts=syn_starts(end_of(offs)), lead_begin=0, text_end=end_of(offs), open_end=end_of(offs))
    for all_patterns in (False, True):
        ep, eo, _ = run_pass(env.m, env.model, planes, cells, offs, pm.HEAD, all_patterns, what="runs", **kw)
        for at, kept in where:
            sel = eo == offs[at]
            assert int(sel.sum()) == (kept if all_patterns else 1) and (ep[sel] == 3).all(), (at, int(sel.sum()))
    for x in planes:
        x.free()


# ------------------------------------------------------------------ 3. window edges on scanned text

EDGE = [b"abc", b"abc", b"abc", b"abc", b"xyz", b"longpattern", b"abc", b"c"]
EDGE_W = {0: (2, 4, False),        # a - T0 in [2, 4]
          1: (0, 0, False),        # ^
          2: (3, 3, True),         # $: ends on the text's last byte
          3: (4, 4, True),         # one byte in front of that
          4: (5, 2, False),        # lo > hi: never
          6: (6, 9, False)}        # the same bytes as 0, a disjoint window
EDGE_TEXTS = [b"abc", b".abc", b"..abc", b"....abc", b".....abc", b"abc.", b"ab", b"", b"", b"xyz", b"longpatter",
              b"longpattern", b"......abc", b"", b"..abc..abc", b"c", b"abcabcabcabc"]


def test_window_edges(gpu):
    model = pm.PositionModel(EDGE, EDGE_W)
    m = Matcher(pm.build(EDGE, EDGE_W), 0, max_text=4096)
    base = np.cumsum([0] + [len(t) for t in EDGE_TEXTS])
    brute = pm.brute_force(EDGE, EDGE_W, EDGE_TEXTS)
    for all_patterns in (False, True):
        exp = model.records(EDGE_TEXTS, all_patterns)
        go, gp, last, und = m.scan_positions(texts=EDGE_TEXTS, all_patterns=all_patterns)
        assert np.array_equal(go, exp[0]) and np.array_equal(gp, exp[1]) and (last, und) == (exp[2], 0), all_patterns
    got = set(zip(go.tolist(), gp.tolist()))
    assert got == brute
    end = lambda k: int(base[k]) + len(EDGE_TEXTS[k]) - 1
    at = lambda k: {p for o, p in got if o == end(k)}
    assert at(0) == {1, 2, 7}                  # "abc": ^ and $ (and "c")
    assert at(1) == {2, 7}                     # a - T0 = lo - 1
    assert at(2) == {0, 2, 7}                  # = lo
    assert at(3) == {0, 2, 7}                  # = hi
    assert at(4) == {2, 7}                     # = hi + 1
    assert {p for o, p in got if o == end(5) - 1} == {1, 3, 7}     # Tend - a = L + 1
    assert at(9) == set() and at(10) == set() and at(11) == {5}
    assert at(12) == {6, 2, 7}                 # the duplicate with the other window
    assert {p for o, p in got if o == int(base[14]) + 4} == {0, 7} and at(14) == {2, 6, 7}   # both duplicates, all form
    m.close()


# ------------------------------------------------------------------ 4. segments, the lead text, open ends


@pytest.mark.parametrize("slice_len", [0, 2048, 2049])
def test_segment_slices(env, slice_len):
    """the starts tile 0 spans: none (one start beyond the records, a sentinel), exactly the LDS budget, one
    more (searched in global memory): many empty texts, a record belongs to the last start <= its offset"""
    m = 1025
    starts = [4 * m + 100] if slice_len == 0 else [0] + [4] * (slice_len - 1) + [4096]
    for report in (pm.STATE, pm.HEAD):
        cells, offs = env.planes(m, report)
        planes = upload(cells, offs)
        for all_patterns in (False, True):
            for open_end in (None, 4 * m + 4, 4 * m + 4 + 1000):
                ep, _, und = run_pass(env.m, env.model, planes, cells, offs, report, all_patterns, starts=starts,
                                      lead_begin=-30, text_end=4 * m + 4, open_end=open_end, what="slice")
                assert und == 0 or open_end is None
                assert und > 0 or open_end is not None or slice_len
        for x in planes:
            x.free()


def test_lead_and_open_end(env):
    m = 300
    text_end = 4 * m + 4
    cells, offs = env.planes(m, pm.STATE)
    planes = upload(cells, offs)
    seen = set()
    for lead_begin in (-(2 ** 40), -25, 0, 40):
        for open_end in (None, text_end, text_end + 17, 2 ** 40):
            for starts in ([], [600], [600, text_end], [600, text_end + 1], [600, INT32_MAX, INT32_MAX]):
                ep, eo, und = run_pass(env.m, env.model, planes, cells, offs, pm.STATE, True, starts=starts,
                                       lead_begin=lead_begin, text_end=text_end, open_end=open_end, what="lead")
                seen.add((ep.size, und))
                # a start at text_end closes the text in front of it: its end is known whatever open_end is
                assert (und > 0) == (open_end is None and starts != [600, text_end])
    assert len(seen) > 6                      # the arguments matter
    for x in planes:
        x.free()


# ------------------------------------------------------------------ 5. a stream cut at every position

STREAM = [b"a", b"ab", b"bab", b"abba", b"aab", b"b", b"baab", b"ab"]
STREAM_W = {1: (0, 3, False), 2: (3, 12, True), 3: (4, None, False), 4: (4, 4, True), 5: (0, 2, True), 7: (2, 2, True)}


def test_streaming(gpu):
    rng = np.random.default_rng(3)
    texts = [bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=n)) for n in (70, 60, 70)]
    stream = np.frombuffer(b"".join(texts), dtype=np.uint8)
    G = [0, 70, 130]
    model = pm.PositionModel(STREAM, STREAM_W)
    m = Matcher(pm.build(STREAM, STREAM_W), 0, max_text=4096)
    for all_patterns in (True, False):
        exp = model.records(texts, all_patterns)
        whole = m.scan_positions(texts=(stream, np.array(G, dtype=np.int32)), all_patterns=all_patterns)
        assert np.array_equal(whole[0], exp[0]) and np.array_equal(whole[1], exp[1]) and whole[2:] == exp[2:]
        assert exp[0].size > 80 and exp[3] == 0
        lost = 0
        for c in range(1, 200):
            s1 = np.array([s for s in G if s < c], dtype=np.int32)
            s2 = np.array([s - c for s in G if s >= c], dtype=np.int32)
            end1 = min([s for s in G if s >= c] + [200])
            o1, p1, last, u1 = m.scan_positions(texts=(stream[:c], s1), all_patterns=all_patterns, open_end=end1)
            o2, p2, last, u2 = m.scan_positions(texts=(stream[c:], s2), all_patterns=all_patterns, init_state=last,
                                                lead_begin=int(s1[-1]) - c)
            assert u1 == 0 and u2 == 0
            assert np.array_equal(np.concatenate([o1, o2 + c]), whole[0]), "cut at %d" % c
            assert np.array_equal(np.concatenate([p1, p2]), whole[1]) and last == whole[2], "cut at %d" % c
            if c % 20 == 7:                     # the end withheld: the first call counts what it cannot decide
                w1, q1, _, u1 = m.scan_positions(texts=(stream[:c], s1), all_patterns=all_patterns, open_end=None)
                assert u1 > 0 and w1.size <= o1.size
                if all_patterns:                # what is left is what was kept with the end known, in order
                    known = list(zip(o1.tolist(), p1.tolist()))
                    left = list(zip(w1.tolist(), q1.tolist()))
                    assert [x for x in known if x in set(left)] == left
                    assert all(STREAM_W.get(p, (0, 0, False))[2] for _, p in set(known) - set(left))
                lost += u1
        assert lost > 0
    m.close()


# ------------------------------------------------------------------ 6. composition with the case and word passes

LONG3 = [(b"abc", False), (b"ABC", True), (b"bcd", False), (b"Bcd", True), (b"abcd", False), (b"cdab", True), (b"abc", False)]
WITH1 = LONG3 + [(b"d", False), (b"A", True)]
COMP_W = {0: (0, 0, False), 1: (1, None, False), 2: (3, 3, True), 3: (0, 6, True), 5: (2, 9, False), 6: (4, 9, True),
          7: (1, 1, True)}


@functools.lru_cache(maxsize=None)
def comp_texts():
    """texts of up to 6 patterns in random case, glued by nothing, a word byte or another byte; and the edges"""
    rng = np.random.default_rng(9)
    glue = [b"", b"", b" ", b".", b"_", b"x", b"  "]
    texts = []
    for _ in range(80):
        t = bytearray(glue[int(rng.integers(len(glue)))])
        for _ in range(int(rng.integers(0, 7))):
            p = bytearray(WITH1[int(rng.integers(len(WITH1)))][0])
            if rng.random() < 0.4:
                k = int(rng.integers(len(p)))
                p[k] ^= 0x20
            t += p + glue[int(rng.integers(len(glue)))]
        texts.append(bytes(t))
    return texts + [b"abc", b"ABC", b"abcd", b"aBcd", b" abc ", b"xabc", b"abc_", b"bcd", b"", b"d", b"Abcd abcd"]


@pytest.mark.parametrize("then", ["case", "words"])
@pytest.mark.parametrize("name", ["sparse", "chain"])
def test_composition(gpu, name, then):
    pats = LONG3 if name == "sparse" else WITH1
    windows = {i: w for i, w in COMP_W.items() if i < len(pats)}
    if then == "words":                       # (the word pass reads raw bytes: an automaton that is not mixed)
        pats = [p for p, _ in pats]
    a = pm.build(pats, windows)
    assert a.mixed_case == (then == "case") and a.positioned
    model = pm.PositionModel(pats, windows)
    texts = comp_texts()
    n = sum(len(t) for t in texts)
    m = Matcher(a, 0, max_text=n)
    assert m.sparse_eligible() == (name == "sparse")
    if name == "sparse":
        assert m.set_mode("sparse") == "sparse"
    plain = pm.PositionModel(pats, windows).records(texts, True)[0].size
    for all_patterns in (False, True):
        exp = model.records(texts, all_patterns, then=then)
        go, gp, last, und = m.scan_positions(texts=texts, all_patterns=all_patterns, then=then)
        assert np.array_equal(go, exp[0]) and np.array_equal(gp, exp[1]) and (last, und) == (exp[2], 0), all_patterns
        assert 15 < exp[0].size < plain       # the pass in between drops entries, and so do the windows
        assert exp[0].size < pm.PositionModel(pats, {}).records(texts, all_patterns, then=then)[0].size
    assert m.path_taken(n) == name
    m.close()


def single(model, t, all_patterns, then, before=b""):
    """what scan_positions(t, then=then, before=before) returns: one text that starts at offset 0 and ends with
    its bytes, no segment pass; the pass in between sees `before` in front of it"""
    states, offs, last = model.walk(t)
    whole, k = bytes(before) + bytes(t), len(before)
    ent = [(p, o) for s, o in zip(states.tolist(), offs.tolist()) for p in model.list[s, :model.list_len[s]].tolist()
           if model.then_keeps(then, p, o + k, whole)]
    p, o, und = model.entries([e[0] for e in ent], [e[1] for e in ent], all_patterns, (), 0, len(t), len(t))
    return o.astype(np.uint32), p, last, und


@pytest.mark.parametrize("then", [None, "case", "words"])
def test_single_text(gpu, then):
    """text instead of texts, with and without before: only the word pass looks at the byte in front of the text"""
    pats = WITH1 if then == "case" else [p for p, _ in WITH1]
    model = pm.PositionModel(pats, COMP_W)
    t = b"abcd " + b" ".join(comp_texts())       # "abcd" at the text start: a word unless a word byte is in front
    assert len(t) < 4096
    m = Matcher(pm.build(pats, COMP_W), 0, max_text=len(t))
    for all_patterns in (False, True):
        alone = model.records([t], all_patterns, then=then)
        assert alone[0].size > 15 and alone[3] == 0
        for before in (b"", b".", b"x_"):
            exp = single(model, t, all_patterns, then, before)
            go, gp, last, und = m.scan_positions(t, all_patterns=all_patterns, then=then, before=before)
            assert np.array_equal(go, exp[0]) and np.array_equal(gp, exp[1]) and (last, und) == exp[2:], (all_patterns, before)
            as_alone = np.array_equal(exp[0], alone[0]) and np.array_equal(exp[1], alone[1])
            assert as_alone == (then != "words" or before != b"x_"), (all_patterns, before)
    m.close()


# ------------------------------------------------------------------ 7. an automaton without constraints


def test_identities(gpu):
    pats = [b"abc", b"bc", b"c", b"abcabc", b"cab", b"ab"]
    a = pm.build(pats, {})
    assert not a.positioned
    rng = np.random.default_rng(4)
    text = rng.choice(np.frombuffer(b"abc.", dtype=np.uint8), size=3000)
    m = Matcher(a, 0, max_text=text.size)
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)
    head = m.scan(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    every = m.scan_all(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    ocap = every[0].size + 2 + 5
    assert every[0].size > head[0].size > 500

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

    def position(sp, so, max_records, report, all_patterns, **kw):
        pat, off, info = poisoned(), poisoned(), DeviceArray(16)
        m.position_async(sp, so, max_records, pat, off, ocap, info, report=report, all_patterns=all_patterns, **kw)
        out = pat.to_numpy(np.int32, ocap + SLACK), off.to_numpy(np.int32, ocap + SLACK), info.to_numpy(np.int32, 4)
        for x in (pat, off, info):
            x.free()
        return out
    # whatever the texts are said to be: no entry has a window
    for kw in (dict(), dict(seg_start=starts, segments=3, lead_begin=-5, text_end=text.size, open_end=-1)):
        gp, go, gi = position(m.pat_plane, m.off_plane, cap - 2, _lib.REPORT_STATE, True, **kw)
        assert np.array_equal(gp, ex_p) and np.array_equal(go, ex_o) and gi.tolist() == [0, 0, 0, 0]   # STATE + all: the expansion
        gp, go, gi = position(xp, xo, ocap - 2, _lib.REPORT_HEAD, True, **kw)
        assert np.array_equal(gp, ex_p) and np.array_equal(go, ex_o) and gi.tolist() == [0, 0, 0, 0]   # HEAD + all: the input
        gp, go, gi = position(m.pat_plane, m.off_plane, cap - 2, _lib.REPORT_STATE, False, **kw)
        k = head[0].size
        assert int(gp[0]) == k and int(go[0]) == k and gi.tolist() == [0, 0, 0, 0]                  # STATE + first: the HEAD scan
        assert np.array_equal(go[1:1 + k].astype(np.uint32), head[0]) and np.array_equal(gp[1:1 + k], head[1])
        assert int(gp[1 + k]) == head[2] and int(go[1 + k]) == head[2] and (gp[2 + k:] == PV).all()
    # bit for bit, against the planes of a HEAD scan
    m.scan_async(d, text.size)
    hp, ho = m.pat_plane.to_numpy(np.int32, k + 2), m.off_plane.to_numpy(np.int32, k + 2)
    assert np.array_equal(gp[:k + 2], hp) and np.array_equal(go[:k + 2], ho)
    for x in (d, xw, xp, xo, starts):
        x.free()
    m.close()


def test_argument_errors(env):
    m = env.m
    buf, out = DeviceArray(4096), DeviceArray(1024 * 4)
    buf.fill(0)
    out.fill(P)
    ws = m.lib.acm_position_workspace_bytes(100)
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20, 1 << 22, 0x7FFFFFFE):
        b = m.lib.acm_position_workspace_bytes(r)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, max_records=100, report=0, st=buf.ptr, S=4, lead=0, end=100, open=100,
                po=out.ptr, oo=out.ptr + 2048, cap=100, info=out.ptr + 1024, ws=buf.ptr, ws_bytes=ws)
    bad = [dict(dfa=None), dict(sp=None), dict(so=None), dict(po=None), dict(oo=None), dict(info=None), dict(cap=1),
           dict(cap=0), dict(ws_bytes=ws - 1), dict(ws=None), dict(report=2), dict(report=-1), dict(open=99), dict(open=-2),
           dict(open=0), dict(st=None), dict(max_records=0x7FFFFFFF), dict(S=0x80000000)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_position_matches_async(x["dfa"], x["sp"], x["so"], x["max_records"], x["report"], x["st"], x["S"],
                                              x["lead"], x["end"], x["open"], 0, x["po"], x["oo"], x["cap"], x["info"],
                                              x["ws"], x["ws_bytes"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()           # nothing was enqueued
    with pytest.raises(AcmError):
        m.position_async(buf, buf, 100, out, out, 1, out)
    # the same call with good arguments is accepted (an empty plane: no records), open_end -1 and text_end as well
    for open_end in (100, -1, 1 << 40):
        m.position_async(buf, buf, 100, out.ptr, out.ptr + 2048, 100, out.ptr + 1024, report=0, seg_start=buf, segments=4,
                         text_end=100, open_end=open_end)
        assert out.to_numpy(np.int32, 2).tolist() == [0, 0]
        assert out.to_numpy(np.int32, 4, offset_bytes=1024).tolist() == [0, 0, 0, 0]
    buf.free()
    out.free()
