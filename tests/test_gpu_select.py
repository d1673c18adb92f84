"""Leftmost-longest non-overlapping selection on the device (acm_select_matches_async, Matcher.scan_select), cell
for cell against the model of tests/select_model.py: synthetic planes at the record counts where the record-pass
core and the radix passes can go wrong; chains of every length the doubling rounds depend on; ties inside a run of
equal starts, across tile and block cuts; wildcard contexts; cells that take no part; min_start; capacities;
determinism and argument errors; Matcher.scan_select against the model over the occurrences bytes.find gives.
Outputs and the workspace are poisoned before every call and guard cells behind every output are checked."""
import numpy as np
import pytest

import poison
import select_model as sel
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16                                   # guard cells behind every output plane
NO_CELL = 0x7FFFFF00                         # no pattern index
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049]
BIG = 1024 * 1024 + 1025                     # 1026 tiles on 1024 blocks: a block owns two tiles; 21 rounds of doubling
INT32_MAX = 0x7FFFFFFF
INT32_MIN = -(2 ** 31)

#       0     1      2       3        4      5      6        7    8      9
SYN = [b"a", b"ab", b"abc", b"abcd", b"bc", b"cd", b"dddd", b"", b"ab", b"xxxxxxxxx"]
A, AB, ABC, ABCD, BC, CD, DDDD, EMPTY, AB2, LONG = range(10)
SYN_CELLS = [-1, NO_CELL, EMPTY, A, AB, ABC, ABCD, BC, CD, DDDD, AB2, LONG, A, A, BC]


def syn_planes(m):
    """(cells, offsets) of m records: random cells (a pattern of 0 to 9 bytes, -1 or no pattern) in runs of equal
    offsets, a new offset one or two bytes on with probability 0.7: the order by start is far from the input's"""
    rng = np.random.default_rng(4000 + m)
    cells = np.array(SYN_CELLS, dtype=np.int64)[rng.integers(0, len(SYN_CELLS), m)]
    offs = np.cumsum((rng.random(m) < 0.7) * rng.integers(1, 3, m)) + 3
    return cells, offs.astype(np.int64)


def build(pats):
    a = Automaton()
    for i, p in enumerate(pats):
        a.add(p, i)
    a.compile()
    return a


class Env:
    def __init__(self):
        self.model = sel.SelectModel([len(p) for p in SYN])
        self.m = Matcher(build(SYN), 0, max_text=4096)
        self.cache = {}

    def planes(self, m):
        if m not in self.cache:
            self.cache[m] = syn_planes(m)
        return self.cache[m]


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


def call(matcher, planes, mr, cap, min_start=0, fill=0xA5, with_start=True):
    """one call from poisoned outputs and a poisoned workspace; (pattern plane, offset plane, start plane, info),
    each with its guard cells; without with_start the start plane is not passed and must stay poisoned"""
    pat, off, start = (DeviceArray((cap + SLACK) * 4) for _ in range(3))
    info = DeviceArray((4 + SLACK) * 4)
    poison.fill([pat, off, start, info], P)
    nb = matcher.lib.acm_select_workspace_bytes(mr)
    ws = DeviceArray(max(nb, 16))
    ws.fill(fill)
    matcher.select_async(planes[0], planes[1], mr, pat, off, cap, info, start_out=start if with_start else None,
                         min_start=min_start, workspace=(ws.ptr, nb))
    out = tuple(x.to_numpy(np.int32, cap + SLACK) for x in (pat, off, start)) + (info.to_numpy(np.int32, 4 + SLACK),)
    for x in (pat, off, start, info, ws):
        x.free()
    return out


def run_pass(matcher, model, planes, cells, offs, min_start=0, cap=None, max_records=None, trailer=77, with_start=True,
             what=""):
    """one call compared whole with the model; returns the model's (patterns, offsets, starts, info)"""
    m = len(cells)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    ep, eo, es, einfo = model.run(cells[:mm], offs[:mm], min_start)
    last = trailer if mm == m else int(cells[mm])
    cap = ep.size + 9 if cap is None else cap
    gp, go, gs, gi = call(matcher, planes, mr, cap, min_start, with_start=with_start)
    what = "%s m=%d max_records=%d cap=%d min_start=%d" % (what, m, mr, cap, min_start)
    xp, xo, xs = sel.planes(ep, eo, es, cap, PV, last)
    assert int(gp[0]) == ep.size and int(go[0]) == ep.size, "%s: count %d/%d, model %d" % (what, gp[0], go[0], ep.size)
    assert np.array_equal(gp[:cap], xp), "%s: pattern plane differs at %s" % (what, np.flatnonzero(gp[:cap] != xp)[:5])
    assert np.array_equal(go[:cap], xo), "%s: offset plane differs at %s" % (what, np.flatnonzero(go[:cap] != xo)[:5])
    if with_start:
        assert np.array_equal(gs[:cap], xs), "%s: start plane differs at %s" % (what, np.flatnonzero(gs[:cap] != xs)[:5])
    else:
        assert (gs == PV).all(), "%s: a start plane that was not passed was written" % what
    assert (gp[cap:] == PV).all() and (go[cap:] == PV).all() and (gs[cap:] == PV).all(), "%s: written behind the capacity" % what
    assert gi[:4].tolist() == einfo and (gi[4:] == PV).all(), "%s: info %s, model %s" % (what, gi[:6], einfo)
    return ep, eo, es, einfo


def free(planes):
    for x in planes:
        x.free()


# ------------------------------------------------------------------ 1. synthetic planes


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_synthetic_planes(env, m):
    cells, offs = env.planes(m)
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs)
    if m >= 1023:
        # neither empty nor everything; the empty pattern is never chosen; the order by start is not the input's
        real = int(np.isin(cells, [A, AB, ABC, ABCD, BC, CD, DDDD, AB2, LONG]).sum())
        assert 0.05 * real < ep.size < 0.6 * real, (ep.size, real)
        assert set(ep.tolist()) >= {A, ABCD, DDDD, LONG} and EMPTY not in ep.tolist()
        assert einfo[0] + einfo[1] == real
        s = env.model.spans(cells, offs)[0]
        assert (np.diff(s[np.isin(cells, [A, LONG])]) < 0).sum() > m // 50
        assert (np.diff(es) > 0).all() and (np.diff(eo) > 0).all()
    if m != BIG:
        for cap in sorted({max(ep.size + 2, 2), max(ep.size + 1, 2), max(ep.size, 2), 3, 2}):
            run_pass(env.m, env.model, planes, cells, offs, cap=cap)
        run_pass(env.m, env.model, planes, cells, offs, cap=max(ep.size + 1, 2), with_start=False)
        for mr in sorted({max(m - 1, 0), m // 2, m + 5}):
            run_pass(env.m, env.model, planes, cells, offs, max_records=mr)
        for ms in (-20, int(offs[m // 2]) if m else 7):
            dropped = run_pass(env.m, env.model, planes, cells, offs, min_start=ms)[3][1]
            assert dropped > m // 4 if ms > 0 and m >= 63 else dropped == 0 or ms > 0
    free(planes)


def test_hostile_planes(env):
    """cells that are no pattern, offsets at the ends of int32, a count cell beyond max_records, min_start at the ends
    of its range: nothing is read outside the planes and the tables and the model's records come out.  Offsets out of
    order are outside the contract: nothing may be written outside the planes, whatever comes out."""
    rng = np.random.default_rng(5)
    m = 1500
    edge = np.array([INT32_MIN, INT32_MIN + 1, INT32_MIN + 9, -5, 0, 1, 8, 9, 3000, INT32_MAX - 1, INT32_MAX], dtype=np.int64)
    cells = np.array(list(range(10)) + [-1, INT32_MIN, INT32_MAX, NO_CELL, 10, 11], dtype=np.int64)[rng.integers(0, 16, m)]
    offs = np.sort(np.concatenate([edge[rng.integers(0, 11, m // 2)], rng.integers(0, 6004, m - m // 2)]))
    for count in (m, INT32_MAX, -1):
        planes = upload(cells, offs, count=count)
        for ms in (0, -7, INT32_MIN + 1, INT32_MAX, INT32_MAX - 3, 2999):
            run_pass(env.m, env.model, planes, cells, offs, min_start=ms, what="hostile count=%d" % count)
        free(planes)
    mixed = rng.permutation(offs)
    planes = upload(cells, mixed)
    for cap in (2, 300, 2 * m):
        gp, go, gs, gi = call(env.m, planes, m, cap, -7)
        assert 0 <= gp[0] == go[0] == gs[0] <= m
        assert (gp[cap:] == PV).all() and (go[cap:] == PV).all() and (gs[cap:] == PV).all()
        assert (gp[min(int(gp[0]) + 2, cap):cap] == PV).all() and gp[min(int(gp[0]) + 1, cap - 1)] == 77
        assert gi[:2].tolist() == env.model.run(cells, mixed, -7)[3][:2] and (gi[4:] == PV).all()   # (counts: no order in them)
    free(planes)


# ------------------------------------------------------------------ 2. the length of the chain


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025])
def test_disjoint_chain(env, m):
    """m disjoint one-byte matches: all are selected, the path has m cells; with max_records far above m (more
    rounds than needed) and below it (only the first max_records are looked at)"""
    cells, offs = np.full(m, A, dtype=np.int64), 2 * np.arange(m, dtype=np.int64)
    planes = upload(cells, offs)
    for mr in sorted({m, m + 1, m + 70000, m - 1, m // 2}):
        ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, max_records=mr, what="chain")
        k = min(m, mr)
        assert ep.size == k and einfo == [k, 0, 2 * k - 1 if k else 0, 0]
    free(planes)


@pytest.mark.parametrize("m", [2, 9, 10, 1025, 2049])
def test_one_long_over_short(env, m):
    """the other extreme: m - 1 one-byte matches under one nine-byte match that starts with the first of them"""
    offs = np.concatenate([92 + (np.arange(m - 1, dtype=np.int64) * 9) // max(m - 1, 1), [100]])
    cells = np.concatenate([np.full(m - 1, A, dtype=np.int64), [LONG]])
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, what="long")
    assert ep.tolist() == [LONG] and eo.tolist() == [100] and es.tolist() == [92] and einfo == [m, 0, 101, 0]
    free(planes)


# ------------------------------------------------------------------ 3. ties


def test_hand_cases(env):
    # "abcd" with {ab, abc, bc, cd}: four records, one match
    cells, offs = np.array([AB, ABC, BC, CD], dtype=np.int64), np.array([1, 2, 2, 3], dtype=np.int64)
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs)
    assert (ep.tolist(), eo.tolist(), es.tolist(), einfo) == ([ABC], [2], [0], [4, 0, 3, 0])
    free(planes)
    # nested prefixes at one start: the longest wins; then the next start behind it
    cells, offs = np.array([A, AB, ABC, BC, ABCD, CD, A], dtype=np.int64), np.array([10, 11, 12, 12, 13, 13, 14], dtype=np.int64)
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs)
    assert (ep.tolist(), eo.tolist(), es.tolist(), einfo) == ([ABCD, A], [13, 14], [10, 14], [7, 0, 15, 0])
    free(planes)
    # the same bytes added twice: the first in the input wins, whichever it is
    for pair in ([AB2, AB], [AB, AB2]):
        cells, offs = np.array([A] + pair + [BC], dtype=np.int64), np.array([10, 11, 11, 12], dtype=np.int64)
        planes = upload(cells, offs)
        ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs)
        assert (ep.tolist(), eo.tolist(), es.tolist()) == ([pair[0]], [11], [10])
        free(planes)


def cut_planes(m, cuts):
    """m disjoint one-byte matches ten bytes apart; at every cut c the six records [c - 3, c + 3) begin at one byte:
    a, ab, ab again, abc, abcd, abcd again: the fifth is chosen"""
    cells, offs = np.full(m, A, dtype=np.int64), 10 * np.arange(m, dtype=np.int64)
    for c in cuts:
        cells[c - 3:c + 3] = [A, AB, AB2, ABC, ABCD, ABCD]
        offs[c - 3:c + 3] = offs[c - 3] + np.array([0, 1, 1, 2, 3, 3])
    assert (np.diff(offs) >= 0).all()
    return cells, offs


@pytest.mark.parametrize("m,cuts", [(2060, [1024, 2048]), (BIG, [1024, 2048 * 100, 2048 * 300 + 1024, 2048 * 512])],
                         ids=["tiles", "blocks"])
def test_runs_across_cuts(env, m, cuts):
    """a run of equal starts laid across a tile cut (1024 k) or a block cut (2048 k of the big count: every cell is
    eligible, so the order by start is the input's); the big count is also the longest chain: m - 5 * cuts cells"""
    cells, offs = cut_planes(m, cuts)
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, what="runs")
    assert ep.size == m - 5 * len(cuts) and einfo[:2] == [m, 0]
    for c in cuts:
        k = int(np.searchsorted(es, offs[c - 3]))
        assert (int(ep[k]), int(eo[k]), int(es[k])) == (ABCD, int(offs[c + 1]), int(offs[c - 3])), c
    free(planes)


def test_long_run_of_equal_starts(env):
    """2100 entries that begin at one byte (a run over two tile cuts), the longest in the middle of them"""
    k = 2100
    cells = np.concatenate([[A], np.full(k, AB, dtype=np.int64), [BC, A]])
    cells[1 + k // 2] = ABC
    offs = np.concatenate([[5], np.full(k, 11, dtype=np.int64), [12, 20]])
    offs[1 + k // 2:1 + k] = 12                                  # (ab at 12 starts one byte on: a second run)
    offs[1 + k // 2] = 12
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, what="run")
    assert (ep.tolist(), eo.tolist(), es.tolist()) == ([A, ABC, A], [5, 12, 20], [5, 10, 20])
    free(planes)


# ------------------------------------------------------------------ 4. contexts

ANY = range(256)


def wild_env():
    a = Automaton()
    a.add_wildcard([ANY, b"k", b"e", b"y", ANY, ANY], 0)         # 0: pre 1, anchor 3, post 2
    a.add(b"key", 1)                                             # 1: plain
    a.add_wildcard([ANY, ANY, b"k", b"e"], 2)                    # 2: pre 2, anchor 2
    a.add_wildcard([b"e", b"y", ANY, ANY, ANY, ANY, ANY], 3)     # 3: anchor 2, post 5
    a.add(b"z", 4)
    a.compile()
    lens = [len(a.pattern(i)[0]) for i in range(5)]
    ctx = [a.wildcard_lengths(i) for i in range(5)]
    assert lens == [3, 3, 2, 2, 1] and ctx == [(1, 2), (0, 0), (2, 0), (0, 5), (0, 0)]
    return a, sel.SelectModel(lens, [c[0] for c in ctx], [c[1] for c in ctx])


def test_contexts(gpu):
    a, model = wild_env()
    m = Matcher(a, 0, max_text=4096)
    # ".key.." at 9..14: the anchor "key" ends at 12.  Entries 0, 2 and (one byte on) 1 and 3:
    #   0 @12: [9, 14]    2 @11: [8, 11]    1 @12: [10, 12]    3 @12: [11, 17]
    cells = np.array([4, 2, 0, 2, 1, 3, 4, 4, 4, 4], dtype=np.int64)
    offs = np.array([3, 11, 12, 12, 12, 12, 13, 15, 17, 18], dtype=np.int64)
    #  starts:       3,  8,  9,  9, 10, 11, 13, 15, 17, 18;  ends: 3, 11, 14, 12, 12, 17, ...
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(m, model, planes, cells, offs, what="contexts")
    # z; then 2 @11 (start 8); then the first start >= 12: z @13, 15, 17, 18
    assert (ep.tolist(), eo.tolist(), es.tolist()) == ([4, 2, 4, 4, 4, 4], [3, 11, 13, 15, 17, 18], [3, 8, 13, 15, 17, 18])
    # from 9 on: the run of start 9 is (0 @12, e 14) and (2 @12, e 12): the largest e is not the last cell, and it
    # reaches over z @13, whose offset is the next record's; the offset stays the anchor's end
    ep, eo, es, einfo = run_pass(m, model, planes, cells, offs, min_start=9, what="contexts")
    assert (ep.tolist(), eo.tolist(), es.tolist()) == ([0, 4, 4, 4], [12, 15, 17, 18], [9, 15, 17, 18])
    assert einfo == [8, 2, 19, 0]
    # from 11 on: 3 @12 spans [11, 17] and hides z @13, 15 and 17
    ep, eo, es, einfo = run_pass(m, model, planes, cells, offs, min_start=11, what="contexts")
    assert (ep.tolist(), eo.tolist(), es.tolist()) == ([3, 4], [12, 18], [11, 18])
    free(planes)
    # random planes over the set
    for n in (257, 2049):
        rng = np.random.default_rng(n)
        cells = np.array([-1, 0, 1, 2, 3, 4, 4, NO_CELL], dtype=np.int64)[rng.integers(0, 8, n)]
        offs = (np.cumsum((rng.random(n) < 0.7) * rng.integers(1, 4, n)) + 2).astype(np.int64)
        planes = upload(cells, offs)
        for ms in (0, -3, 40):
            ep, eo, es, einfo = run_pass(m, model, planes, cells, offs, min_start=ms, what="contexts")
        assert set(ep.tolist()) == {0, 1, 2, 3, 4}
        free(planes)
    m.close()


# ------------------------------------------------------------------ 5. cells that take no part, min_start


def test_cells_that_take_no_part(env):
    for n in (1, 300, 1030):
        cells = np.array([-1, NO_CELL, EMPTY], dtype=np.int64)[np.arange(n) % 3]
        offs = np.arange(n, dtype=np.int64) + 4
        planes = upload(cells, offs)
        for ms in (0, -9, 2 ** 31 - 1):
            ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, min_start=ms)
            assert ep.size == 0 and einfo == [0, 0, ms, 0 if ms >= 0 else -1]
        free(planes)


def test_min_start(env):
    cells = np.array([LONG, A, AB, ABC, BC, ABCD, CD, A], dtype=np.int64)
    offs = np.array([3, 10, 11, 12, 12, 13, 13, 14], dtype=np.int64)
    planes = upload(cells, offs)
    # the long pattern starts at -5
    want = {-5: ([LONG, ABCD, A], [3, 13, 14], [-5, 10, 14], [8, 0, 15, 0]),
            -4: ([ABCD, A], [13, 14], [10, 14], [7, 1, 15, 0]),
            10: ([ABCD, A], [13, 14], [10, 14], [7, 1, 15, 0]),
            11: ([BC, A], [12, 14], [11, 14], [3, 5, 15, 0]),            # abcd would have won: it is no candidate
            13: ([A], [14], [14], [1, 7, 15, 0]),
            15: ([], [], [], [0, 8, 15, 0]),
            -(2 ** 31) + 1: ([LONG, ABCD, A], [3, 13, 14], [-5, 10, 14], [8, 0, 15, 0])}
    for ms, (xp, xo, xs, xi) in want.items():
        ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, min_start=ms, what="min_start")
        assert (ep.tolist(), eo.tolist(), es.tolist(), einfo) == (xp, xo, xs, xi), ms
    free(planes)
    # a negative cursor: the only match ends in front of 0
    cells, offs = np.array([AB], dtype=np.int64), np.array([-3], dtype=np.int64)
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, min_start=-100)
    assert (ep.tolist(), eo.tolist(), es.tolist(), einfo) == ([AB], [-3], [-4], [1, 0, -2, -1])
    free(planes)
    # a cursor beyond int32: a match that ends at the last offset
    cells, offs = np.array([A], dtype=np.int64), np.array([INT32_MAX], dtype=np.int64)
    planes = upload(cells, offs)
    ep, eo, es, einfo = run_pass(env.m, env.model, planes, cells, offs, min_start=INT32_MAX)
    assert einfo == [1, 0, INT32_MIN, 0] and ep.tolist() == [A]
    free(planes)


# ------------------------------------------------------------------ 6. determinism, argument errors


def test_determinism_and_stale_workspaces(env):
    m = 2049
    cells, offs = env.planes(m)
    planes = upload(cells, offs)
    runs = [call(env.m, planes, m, m + 2, fill=f) for f in (0xA5, 0xA5, 0x00, 0xFF)]
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))
    assert runs[0][0][0] > 100
    free(planes)


def test_argument_errors(env):
    m = env.m
    buf, out = DeviceArray(1 << 16), DeviceArray(1024 * 4)
    buf.fill(0)
    out.fill(P)
    ws = m.lib.acm_select_workspace_bytes(100)
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20, 1 << 22, 0x7FFFFFFE):
        b = m.lib.acm_select_workspace_bytes(r)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    assert ws <= buf.nbytes
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, max_records=100, ms=0, flags=0, po=out.ptr, oo=out.ptr + 2048,
                st=out.ptr + 3072, cap=100, info=out.ptr + 1024, ws=buf.ptr, ws_bytes=ws)
    bad = [dict(dfa=None), dict(sp=None), dict(so=None), dict(po=None), dict(oo=None), dict(info=None), dict(cap=1),
           dict(cap=0), dict(ws_bytes=ws - 1), dict(ws=None), dict(max_records=0x7FFFFFFF), dict(flags=1), dict(flags=0x80000000),
           dict(ms=-(2 ** 31)), dict(ms=2 ** 31), dict(ms=-(2 ** 40)), dict(ms=2 ** 40)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_select_matches_async(x["dfa"], x["sp"], x["so"], x["max_records"], x["ms"], x["flags"], x["po"], x["oo"],
                                            x["st"], x["cap"], x["info"], x["ws"], x["ws_bytes"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()           # nothing was enqueued
    with pytest.raises(AcmError):
        m.select_async(buf, buf, 100, out, out, 1, out)
    # the same call with good arguments is accepted (an empty plane: no records; its own workspace), with and
    # without a start plane
    w = DeviceArray(ws)
    for st in (out.ptr + 3072, None):
        m.select_async(buf, buf, 100, out.ptr, out.ptr + 2048, 100, out.ptr + 1024, start_out=st, min_start=-6,
                       workspace=(w.ptr, ws))
        assert out.to_numpy(np.int32, 2).tolist() == [0, 0]
        assert out.to_numpy(np.int32, 4, offset_bytes=1024).tolist() == [0, 0, -6, -1]
    for x in (buf, out, w):
        x.free()


# ------------------------------------------------------------------ 7. end to end


def occurrences(pats, texts, windows=None):
    """(cells, offsets) of every occurrence of every pattern in every text, each text alone, in offset order: found
    with bytes.find.  pats: bytes or (bytes, nocase); windows {pattern: (lo, hi or None, from_end)}"""
    windows = windows or {}
    out, base = [], 0
    for t in texts:
        t = bytes(t)
        for i, p in enumerate(pats):
            pat, nc = p if isinstance(p, tuple) else (p, False)
            hay, needle = (t.upper(), pat.upper()) if nc else (t, pat)
            lo, hi, fe = windows.get(i, (0, None, False))
            k = hay.find(needle)
            while k >= 0 and needle:
                v = len(t) - k if fe else k
                if lo <= v and (hi is None or v <= hi):
                    out.append((base + k + len(pat) - 1, i))
                k = hay.find(needle, k + 1)
        base += len(t)
    out.sort()
    return np.array([c for _, c in out], dtype=np.int64), np.array([o for o, _ in out], dtype=np.int64)


def check_scan(got, model, cells, offs, min_start=0):
    go, gp, gs, info = got
    ep, eo, es, einfo = model.run(cells, offs, min_start)
    assert go.tolist() == eo.tolist() and gp.tolist() == ep.tolist() and gs.tolist() == es.tolist()
    assert info.tolist() == einfo
    assert (es[1:] > eo[:-1]).all()                              # no two overlap
    return ep


E2E = [b"a", b"ab", b"abc", b"bc", b"bcd", b"cd", b"dddd"]


def test_scan_select(gpu):
    """64 KiB of random text over abcd, whole and as texts (one of them empty)"""
    rng = np.random.default_rng(21)
    text = bytes(np.frombuffer(b"abcd", dtype=np.uint8)[rng.integers(0, 4, 64 * 1024)])
    model = sel.SelectModel([len(p) for p in E2E])
    m = Matcher(build(E2E), 0, max_text=len(text))
    cells, offs = occurrences(E2E, [text])
    ep = check_scan(m.scan_select(text), model, cells, offs)
    assert set(ep.tolist()) == set(range(7)) and 20000 < ep.size < cells.size - 5000
    cuts = np.sort(rng.integers(0, 20000, 30))
    texts = [text[a:b] for a, b in zip(np.r_[0, cuts], np.r_[cuts, 20000])]
    texts = texts[:12] + [b""] + texts[12:]
    cells_t, offs_t = occurrences(E2E, texts)
    ep_t = check_scan(m.scan_select(texts=texts), model, cells_t, offs_t)
    whole = model.run(*occurrences(E2E, [text[:20000]]))[0]
    assert ep_t.tolist() != whole.tolist()                       # a cut inside a match changes the selection
    with pytest.raises(AcmError) as e:
        m.scan_select(text, out_capacity=ep.size + 1)
    assert e.value.code == _lib.ACM_ERR_CAPACITY
    # before: a match may start in the bytes in front ("bc" lies across the cut), when the scan goes on from their state
    assert text[:5] == b"bdbcb"
    keep = offs >= 3
    got = m.scan_select(text[3:3000], before=text[:3], init_state=m.scan_all(text[:3])[2])
    sub = keep & (offs < 3000)
    ep_b = check_scan(got, model, cells[sub], offs[sub] - 3, min_start=-3)
    assert got[2][0] == -1 and got[1][0] == E2E.index(b"bc") and ep_b.size > 1000
    # without them it starts in front of what the call has: dropped and counted
    got = m.scan_select(text[3:3000], init_state=m.scan_all(text[:3])[2])
    check_scan(got, model, cells[sub], offs[sub] - 3)
    assert got[3][1] == 1 and got[2][0] >= 0
    m.close()


def test_scan_select_mixed_and_positioned(gpu):
    pats = [(b"Ab", True), (b"abc", False), (b"BC", False), (b"cD", True), (b"d", False)]
    rng = np.random.default_rng(22)
    text = bytes(np.frombuffer(b"abcdABCD", dtype=np.uint8)[rng.integers(0, 8, 16 * 1024)])
    model = sel.SelectModel([len(p[0]) for p in pats])
    a = Automaton()
    for i, (p, nc) in enumerate(pats):
        a.add(p, i, nocase=nc)
    a.compile()
    assert a.mixed_case
    m = Matcher(a, 0, max_text=len(text))
    ep = check_scan(m.scan_select(text), model, *occurrences(pats, [text]))
    assert set(ep.tolist()) == set(range(5))
    m.close()
    # a positioned set: windows from the start and from the end of every text
    plain = [b"ab", b"abc", b"bc", b"c", b"dd"]
    windows = {0: (0, 0, False), 1: (2, None, False), 3: (1, 4, True)}
    a = build(plain)
    for i, (lo, hi, fe) in windows.items():
        a.set_position(i, lo, hi, fe)
    assert a.positioned
    m = Matcher(a, 0, max_text=4096)
    texts = [b"abcabc", b"ab", b"", b"cabcddabc", b"ddd", b"abcc", b"xxabcxx", b"abab"]
    model = sel.SelectModel([len(p) for p in plain])
    cells, offs = occurrences(plain, texts, windows)
    ep = check_scan(m.scan_select(texts=texts), model, cells, offs)
    free_cells = occurrences(plain, texts)[0]
    assert cells.size < free_cells.size and set(ep.tolist()) == set(range(5))
    m.close()
