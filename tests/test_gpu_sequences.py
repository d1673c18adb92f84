"""Ordered multi-part signatures on the device (acm_sequence_matches_async, Matcher.scan_sequences), cell for
cell against the model of tests/sequence_model.py: synthetic planes at the record counts where the record-pass
core and the radix passes can go wrong, runs of equal offsets across tile and block cuts; the edges of a gap;
4 and 32 levels; texts, the lead text and empty segments; capacities; the identity of 1-part sequences;
determinism and argument errors; Matcher.scan_sequences against a brute force.  Outputs and the workspace are
poisoned before every call and guard cells behind every output are checked.

The synthetic set has nine patterns: the four sequences asked for take eight parts (a pattern is a part of at
most one sequence), and one pattern is in none."""
import numpy as np
import pytest

import poison
import sequence_model as sm
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16                                   # guard cells behind every output plane
NO_CELL = 0x7FFFFF00                         # no pattern index
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049]
BIG = 1024 * 1024 + 1025                     # 1026 tiles on 1024 blocks: a block owns two tiles; the sort spans every block
INT32_MAX = 0x7FFFFFFF

SYN = [b"a", b"bb", b"ccc", b"dd", b"e", b"ffff", b"gg", b"hhh", b"zz"]
SYN_SEQS = [([0], []), ([1, 2], [(0, 3)]), ([3, 4, 5], [(1, None), (0, 0)]), ([6, 7], [(4, 2)])]   # "zz" is in none
SYN_CELLS = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, NO_CELL, 1, 2, 4, 5]


def syn_planes(m):
    """(cells, offsets) of m records: random cells (a pattern, -1 or no pattern) in runs of equal offsets, a new
    offset one or two bytes on with probability 0.7"""
    rng = np.random.default_rng(3000 + m)
    cells = np.array(SYN_CELLS, dtype=np.int64)[rng.integers(0, len(SYN_CELLS), m)]
    offs = np.cumsum((rng.random(m) < 0.7) * rng.integers(1, 3, m)) + 3
    return cells, offs.astype(np.int64)


def syn_starts(text_end):
    """a text every 40 bytes from 40 on (the records in front are the lead's) over three quarters of the stream,
    and two sentinels beyond the end"""
    return list(range(40, 3 * text_end // 4, 40)) + [text_end + 100, INT32_MAX]


class Env:
    def __init__(self):
        self.model = sm.SequenceModel([len(p) for p in SYN], SYN_SEQS)
        self.m = Matcher(sm.build(SYN, SYN_SEQS), 0, max_text=4096)
        self.cache = {}

    def planes(self, m):
        if m not in self.cache:
            if m >= BIG:
                self.cache = {k: v for k, v in self.cache.items() if k < BIG}
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


def call(matcher, planes, mr, cap, starts=(), lead_begin=0, text_end=0, fill=0xA5):
    """one call from poisoned outputs and a poisoned workspace; (sequence plane, offset plane, info), each with
    its guard cells"""
    seq, off, info = DeviceArray((cap + SLACK) * 4), DeviceArray((cap + SLACK) * 4), DeviceArray((4 + SLACK) * 4)
    poison.fill([seq, off, info], P)
    nb = matcher.lib.acm_sequence_workspace_bytes(matcher.dfa, mr)
    ws = DeviceArray(max(nb, 16))
    ws.fill(fill)
    S = len(starts)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int64).astype(np.int32), pad_to=0) if S else None
    matcher.sequence_async(planes[0], planes[1], mr, seq, off, cap, info, seg_start=d_st, segments=S,
                           lead_begin=lead_begin, text_end=text_end, workspace=(ws.ptr, nb))
    out = seq.to_numpy(np.int32, cap + SLACK), off.to_numpy(np.int32, cap + SLACK), info.to_numpy(np.int32, 4 + SLACK)
    for x in (seq, off, info, ws, d_st):
        if x is not None:
            x.free()
    return out


def run_pass(matcher, model, planes, cells, offs, starts=(), lead_begin=0, text_end=0, cap=None, max_records=None,
             trailer=77, what=""):
    """one call compared whole with the model; returns the model's (sequences, offsets, info)"""
    m = len(cells)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    eq, eo, einfo = model.run(cells[:mm], offs[:mm], starts, lead_begin)
    last = trailer if mm == m else int(cells[mm])
    cap = eq.size + 9 if cap is None else cap
    gq, go, gi = call(matcher, planes, mr, cap, starts, lead_begin, text_end)
    what = "%s m=%d max_records=%d cap=%d S=%d" % (what, m, mr, cap, len(starts))
    xq, xo = sm.planes(eq, eo, cap, PV, last)
    assert int(gq[0]) == eq.size and int(go[0]) == eq.size, "%s: count %d/%d, model %d" % (what, gq[0], go[0], eq.size)
    assert np.array_equal(gq[:cap], xq), "%s: sequence plane differs at %s" % (what, np.flatnonzero(gq[:cap] != xq)[:5])
    assert np.array_equal(go[:cap], xo), "%s: offset plane differs at %s" % (what, np.flatnonzero(go[:cap] != xo)[:5])
    assert (gq[cap:] == PV).all() and (go[cap:] == PV).all(), "%s: written behind the capacity" % what
    assert gi[:4].tolist() == einfo and (gi[4:] == PV).all(), "%s: info %s, model %s" % (what, gi[:6], einfo)
    return eq, eo, einfo


def end_of(offs):
    return int(offs[-1]) + 1 if len(offs) else 4


# ------------------------------------------------------------------ 1. synthetic planes


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_synthetic_planes(env, m):
    cells, offs = env.planes(m)
    planes = upload(cells, offs)
    text_end = end_of(offs)
    kw = dict(starts=syn_starts(text_end), lead_begin=-20, text_end=text_end)
    eq, eo, einfo = run_pass(env.m, env.model, planes, cells, offs, **kw)
    if m >= 1023:
        # neither empty nor everything: roughly a third of the last-part records are alive, every sequence
        # but the one with lo > hi matches, and the texts matter
        last = int(np.isin(cells, [0, 2, 5, 7]).sum())
        assert 0.2 * last < eq.size < 0.5 * last, (eq.size, last)
        assert set(eq.tolist()) == {0, 1, 2}
        assert env.model.run(cells, offs)[0].size > eq.size
    if m != BIG:
        for cap in sorted({max(eq.size + 2, 2), max(eq.size + 1, 2), max(eq.size, 2), 2}):
            run_pass(env.m, env.model, planes, cells, offs, cap=cap, **kw)
        for mr in sorted({max(m - 1, 0), m // 2, m + 5}):
            run_pass(env.m, env.model, planes, cells, offs, max_records=mr, **kw)
        run_pass(env.m, env.model, planes, cells, offs, lead_begin=0, text_end=text_end)       # segments == 0
    for x in planes:
        x.free()


@pytest.mark.parametrize("m,cuts", [(2060, [1024, 2048]), (BIG, [1024, 2048 * 100, 2048 * 300 + 1024, 2048 * 512])],
                         ids=["tiles", "blocks"])
def test_runs_across_cuts(env, m, cuts):
    """a run of equal offsets laid across a tile cut (1024 k) or a block cut (2048 k of the big count): "bb" in front
    of the cut, "ccc" four bytes on behind it; and both parts inside one run on both sides of the cut"""
    cells, offs = (x.copy() for x in env.planes(m))
    for c in cuts:
        offs[c - 3:] += 40
        offs[c - 3:c + 3] = offs[c - 3]                        # one run of six records across the cut
        cells[c - 3:c + 3] = [8, 1, 8, 8, 1, 8]
        offs[c + 3:] = np.maximum(offs[c + 3:], offs[c - 3] + 4)
        offs[c + 3:c + 6] = offs[c - 3] + 4                    # "ccc" starts two bytes behind that "bb"
        cells[c + 3:c + 6] = [8, 2, 2]
        offs[c + 6:] = np.maximum(offs[c + 6:], offs[c - 3] + 30)
    assert (np.diff(offs) >= 0).all()
    planes = upload(cells, offs)
    eq, eo, _ = run_pass(env.m, env.model, planes, cells, offs, text_end=end_of(offs), what="runs")
    for c in cuts:
        sel = eo == offs[c + 3]
        assert int(sel.sum()) == 2 and (eq[sel] == 1).all(), c
    for x in planes:
        x.free()


def test_hostile_planes(env):
    """cells that are no pattern, offsets at the ends of int32, a count cell beyond max_records: nothing is read
    outside the planes and the tables and the model's records come out.  Offsets out of order are outside the
    contract: nothing may be written outside the planes, whatever comes out."""
    rng = np.random.default_rng(5)
    m = 1500
    edge = np.array([-(2 ** 31), -5, 0, 1, 39, 40, 41, 3000, 6003, 6004, INT32_MAX], dtype=np.int64)
    many = [0] + [4] * 2100 + [4096]
    cells = np.array(list(range(9)) + [-1, -(2 ** 31), INT32_MAX, NO_CELL, 9, 10], dtype=np.int64)[rng.integers(0, 15, m)]
    offs = np.sort(np.concatenate([edge[rng.integers(0, 11, m // 2)], rng.integers(0, 6004, m - m // 2)]))
    for count in (m, INT32_MAX, -1):
        planes = upload(cells, offs, count=count)
        for starts in ([], syn_starts(6004), many):
            for lead in (-7, -(2 ** 62), 2 ** 40):
                run_pass(env.m, env.model, planes, cells, offs, starts=starts, lead_begin=lead, text_end=6004,
                         what="hostile count=%d" % count)
        for x in planes:
            x.free()
    planes = upload(cells, rng.permutation(offs))
    for cap in (2, 300, 2 * m):
        gq, go, gi = call(env.m, planes, m, cap, many, -7, 6004)
        assert 0 <= gq[0] == go[0] <= m and (gq[cap:] == PV).all() and (go[cap:] == PV).all()
        assert (gq[min(int(gq[0]) + 2, cap):cap] == PV).all() and gq[min(int(gq[0]) + 1, cap - 1)] == 77
        assert 0 <= gi[1] and gi[0] == env.model.run(cells, offs)[2][0] and gi[2:4].tolist() == [0, 0] and (gi[4:] == PV).all()
    for x in planes:
        x.free()


# ------------------------------------------------------------------ 2. the edges of a gap

EDGE = [b"aaa", b"bb", b"cc", b"dd", b"ee", b"fff"]
EDGE_SEQS = [([0, 1], [(2, 5)]), ([2, 3], [(3, None)]), ([4, 5], [(0, 0)])]


def test_gap_edges(gpu):
    """hand-made planes where exactly one predecessor exists, at the gap lo - 1, lo, hi, hi + 1; the unbounded gap with
    the predecessor at the very first record; the predecessor's end equal to a - 1 - lo"""
    model = sm.SequenceModel([len(p) for p in EDGE], EDGE_SEQS)
    m = Matcher(sm.build(EDGE, EDGE_SEQS), 0, max_text=4096)
    for gap, alive in ((1, False), (2, True), (3, True), (5, True), (6, False), (0, False)):
        # "aaa" ends at 102; "bb" starts at 103 + gap and ends one byte on; strangers around them
        cells = np.array([5, 0, 3, 1, 5], dtype=np.int64)
        offs = np.array([90, 102, 102, 104 + gap, 104 + gap], dtype=np.int64)
        planes = upload(cells, offs)
        eq, eo, info = run_pass(m, model, planes, cells, offs, text_end=200, what="gap %d" % gap)
        assert (eq.tolist(), eo.tolist()) == (([0], [104 + gap]) if alive else ([], [])), gap
        assert info == [5, 1 + alive, 0, 0]
        for x in planes:
            x.free()
    # the unbounded gap: the predecessor is the very first record, far in front; lo - 1 and lo
    for gap, alive in ((2, False), (3, True), (1000000, True)):
        cells = np.array([2] + [1] * 700 + [3], dtype=np.int64)
        offs = np.array([11] + [11] * 700 + [13 + gap], dtype=np.int64)
        planes = upload(cells, offs)
        eq, eo, _ = run_pass(m, model, planes, cells, offs, text_end=13 + gap + 1, what="unbounded %d" % gap)
        assert eq.tolist() == ([1] if alive else []), gap
        # ... and not when a text begins between the two, or when the first part begins in front of its text
        for starts, lead in (([12], 0), ([11], 0), ([], 11)):
            eq, _, _ = run_pass(m, model, planes, cells, offs, starts=starts, lead_begin=lead, text_end=13 + gap + 1)
            assert eq.size == 0
        for x in planes:
            x.free()
    # (0, 0): the predecessor's end equals a - 1 - lo = a - 1; one byte off either way it is not
    for d, alive in ((-1, False), (0, True), (1, False)):
        cells = np.array([4, 4, 5], dtype=np.int64)
        offs = np.array([50, 57 + d, 60], dtype=np.int64)                # "fff" starts at 58
        planes = upload(cells, offs)
        eq, eo, _ = run_pass(m, model, planes, cells, offs, text_end=61, what="adjacent %d" % d)
        assert eq.tolist() == ([2] if alive else []), d
        for x in planes:
            x.free()
    m.close()


# ------------------------------------------------------------------ 3. levels


@pytest.mark.parametrize("k", [4, 32])
def test_levels(gpu, k):
    """a k-part sequence of one-byte gaps on a planted text; the same with one middle part missing gives nothing"""
    pats = [b"<%02d>" % j for j in range(k)] + [b"solo"]
    seqs = [(list(range(k)), [(1, 1)] * (k - 1), 5), ([k], [], 6)]
    a = sm.build(pats, seqs)
    m = Matcher(a, 0, max_text=4096)
    whole = b".".join(pats[:k])
    holed = b".".join(pats[:k // 2] + [b"<xx>"] + pats[k // 2 + 1:k])
    shifted = b".".join(pats[:k // 2]) + b".." + b".".join(pats[k // 2:k])     # one gap of two bytes
    text = b"solo " + whole + b" ... " + holed + b" solo " + shifted + b" " + whole + b"."
    go, gq, last, info = m.scan_sequences(text)
    exp = sorted(sm.brute_force(pats, seqs, [text]))
    assert list(zip(go.tolist(), gq.tolist())) == exp
    ends = [o for o, q in exp if q == 0]
    assert ends == [5 + len(whole) - 1, len(text) - 2] and sum(q == 1 for _, q in exp) == 2
    alive = 2 * k + k // 2 + k // 2 + 2          # two whole chains, the front half of the two broken ones, "solo" twice
    assert info.tolist() == [4 * k - 1 + 2, alive, 0, 0]
    m.close()


# ------------------------------------------------------------------ 4. texts


def test_texts(env):
    """the predecessor in the previous segment, a part that starts in front of its T0, empty segments and starts
    beyond text_end, a lead text with a negative lead_begin"""
    #        "bb" at 11, "ccc" ends 15 (gap 1): alive unless a text begins in 11 .. 13 (12, 13: the first byte of "ccc")
    cells = np.array([0, 1, 2, 3, 4, 5, 0], dtype=np.int64)
    offs = np.array([0, 11, 15, 21, 30, 34, 40], dtype=np.int64)
    planes = upload(cells, offs)
    expect = {(): [(0, 0), (1, 15), (2, 34), (0, 40)],
              (12,): [(0, 0), (2, 34), (0, 40)],               # the predecessor is in the previous segment
              (14,): [(0, 0), (2, 34), (0, 40)],               # "ccc" starts in front of its T0
              (11,): [(0, 0), (2, 34), (0, 40)],               # "bb" starts in front of its T0
              (10, 10, 10): [(0, 0), (1, 15), (2, 34), (0, 40)],
              (16, 16, 20, 41, 41, 500, INT32_MAX): [(0, 0), (1, 15), (2, 34), (0, 40)],
              (21,): [(0, 0), (1, 15), (0, 40)],               # "dd" starts at 20
              (0, 1): [(0, 0), (1, 15), (2, 34), (0, 40)],
              (31,): [(0, 0), (1, 15), (0, 40)]}
    for starts, exp in expect.items():
        eq, eo, _ = run_pass(env.m, env.model, planes, cells, offs, starts=list(starts), lead_begin=0, text_end=41,
                             what="texts %s" % (starts,))
        assert list(zip(eq.tolist(), eo.tolist())) == exp, starts
    for lead, exp in ((-5, 4), (0, 4), (1, 3), (10, 3), (11, 2), (-(2 ** 40), 4), (2 ** 40, 0)):
        eq, _, _ = run_pass(env.m, env.model, planes, cells, offs, lead_begin=lead, text_end=41, what="lead %d" % lead)
        assert eq.size == exp, lead
    for x in planes:
        x.free()


@pytest.mark.parametrize("slice_len", [0, 2048, 2049])
def test_segment_slices(env, slice_len):
    """the starts tile 0 spans: none, exactly the LDS budget, one more (searched in global memory)"""
    m = 1025
    cells, offs = env.planes(m)
    starts = [end_of(offs) + 100] if slice_len == 0 else [0] + [4] * (slice_len - 1) + [700]
    planes = upload(cells, offs)
    run_pass(env.m, env.model, planes, cells, offs, starts=starts, lead_begin=-30, text_end=end_of(offs), what="slice")
    for x in planes:
        x.free()


# ------------------------------------------------------------------ 5. identity, determinism, no sequences, errors


def test_identity(gpu):
    """sequence i = the 1-part of pattern i, for every pattern: the output is the input, bit for bit (length-0
    entries aside: the expansion does not report them either)"""
    pats = [b"abc", b"bc", b"c", b"abcabc", b"cab", b"ab"]
    a = sm.build(pats, [([i], []) for i in range(len(pats))])
    rng = np.random.default_rng(4)
    text = rng.choice(np.frombuffer(b"abc.", dtype=np.uint8), size=3000)
    m = Matcher(a, 0, max_text=text.size)
    every = m.scan_all(text)
    n = every[0].size
    assert n > 1000
    cells, offs = every[1].astype(np.int64), every[0].astype(np.int64)
    planes = upload(cells, offs, trailer=every[2])
    gq, go, gi = call(m, planes, n, n + 2 + 5)
    xp, xo = sm.planes(cells, offs, n + 2 + 5, PV, every[2])
    assert np.array_equal(gq[:n + 7], xp) and np.array_equal(go[:n + 7], xo) and gi[:4].tolist() == [n, n, 0, 0]
    go2, gq2, last, info = m.scan_sequences(bytes(text))
    assert np.array_equal(go2, every[0]) and np.array_equal(gq2, every[1]) and last == every[2]
    for x in planes:
        x.free()
    m.close()


def test_determinism_and_stale_workspaces(env):
    m = 2049
    cells, offs = env.planes(m)
    planes = upload(cells, offs)
    kw = dict(starts=syn_starts(end_of(offs)), lead_begin=-20, text_end=end_of(offs))
    runs = [call(env.m, planes, m, m + 2, fill=f, **kw) for f in (0xA5, 0xA5, 0x00, 0xFF)]
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))
    assert runs[0][0][0] > 100
    for x in planes:
        x.free()


def test_set_without_sequences(gpu):
    a = sm.build(SYN, [])
    m = Matcher(a, 0, max_text=4096)
    cells, offs = syn_planes(300)
    planes = upload(cells, offs)
    for cap in (2, 3, 50):
        gq, go, gi = call(m, planes, 300, cap)
        xq, xo = sm.planes([], [], cap, PV, 77)
        assert np.array_equal(gq[:cap], xq) and np.array_equal(go[:cap], xo) and (gq[cap:] == PV).all()
        assert gi[:4].tolist() == [0, 0, 0, 0] and (gi[4:] == PV).all()
    go, gq, last, info = m.scan_sequences(b"a bb ccc")
    assert go.size == 0 and gq.size == 0 and info.tolist() == [0, 0, 0, 0]
    for x in planes:
        x.free()
    m.close()


def test_argument_errors(env):
    m = env.m
    buf, out = DeviceArray(1 << 16), DeviceArray(1024 * 4)
    buf.fill(0)
    out.fill(P)
    ws = m.lib.acm_sequence_workspace_bytes(m.dfa, 100)
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20, 1 << 22, 0x7FFFFFFE):
        b = m.lib.acm_sequence_workspace_bytes(m.dfa, r)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    assert ws <= buf.nbytes
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, max_records=100, st=buf.ptr, S=4, lead=0, end=100,
                po=out.ptr, oo=out.ptr + 2048, cap=100, info=out.ptr + 1024, ws=buf.ptr, ws_bytes=ws)
    bad = [dict(dfa=None), dict(sp=None), dict(so=None), dict(po=None), dict(oo=None), dict(info=None), dict(cap=1),
           dict(cap=0), dict(ws_bytes=ws - 1), dict(ws=None), dict(st=None), dict(max_records=0x7FFFFFFF), dict(S=0x80000000)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_sequence_matches_async(x["dfa"], x["sp"], x["so"], x["max_records"], x["st"], x["S"], x["lead"],
                                              x["end"], x["po"], x["oo"], x["cap"], x["info"], x["ws"], x["ws_bytes"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()           # nothing was enqueued
    with pytest.raises(AcmError):
        m.sequence_async(buf, buf, 100, out, out, 1, out)
    # the same call with good arguments is accepted (an empty plane: no records; its own workspace)
    w = DeviceArray(ws)
    m.sequence_async(buf, buf, 100, out.ptr, out.ptr + 2048, 100, out.ptr + 1024, seg_start=buf, segments=4, text_end=100,
                     workspace=(w.ptr, ws))
    assert out.to_numpy(np.int32, 2).tolist() == [0, 0]
    assert out.to_numpy(np.int32, 4, offset_bytes=1024).tolist() == [0, 0, 0, 0]
    for x in (buf, out, w):
        x.free()


# ------------------------------------------------------------------ 6. end to end

E2E = [b"MZ\x90\x00sig", b"payload!", b"\xde\xad\xbe\xef", b"tail", b"needle", b"haystack", b"one", b"two", b"three", b"lonely"]
E2E_SEQS = [([0, 1], [(2, 10)], 100), ([2, 3], [(0, None)], 101), ([4], [], 102), ([5, 6, 7, 8], [(0, 4), (1, 1), (0, 300)], 103)]


def planted_text(n, seed):
    rng = np.random.default_rng(seed)
    t = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    at = 100
    bodies = [E2E[0] + b".." + E2E[1], E2E[0] + b"." + E2E[1], E2E[0] + b"x" * 10 + E2E[1], E2E[0] + b"x" * 11 + E2E[1],
              E2E[2] + E2E[3], E2E[3] + b"...." + E2E[2], E2E[4], E2E[5] + E2E[6] + b"-" + E2E[7] + b"." * 300 + E2E[8],
              E2E[5] + b"....." + E2E[6] + b"-" + E2E[7] + E2E[8], E2E[5] + b"...." + E2E[6] + b"--" + E2E[7] + E2E[8],
              E2E[9], E2E[2] + b"!" * 2000 + E2E[3], E2E[5] + E2E[6] + b"+" + E2E[7] + E2E[8]]
    while at + 3000 < n:
        for b in bodies:
            if at + len(b) + 8 >= n:
                break
            t[at:at + len(b)] = b
            at += len(b) + int(rng.integers(1, 700))
    return bytes(t)


@pytest.mark.parametrize("name", ["sparse", "chain"])
def test_scan_sequences(gpu, name):
    """a 64 KiB seeded text with planted signatures, and 50 short texts, under both pipelines"""
    pats = E2E if name == "sparse" else E2E + [b"x"]               # a one-byte pattern: the set is not sparse-eligible
    a = sm.build(pats, E2E_SEQS)
    text = planted_text(64 * 1024, 11)
    m = Matcher(a, 0, max_text=len(text))
    assert m.sparse_eligible() == (name == "sparse")
    if name == "sparse":
        assert m.set_mode("sparse") == "sparse"
    go, gq, last, info = m.scan_sequences(text)
    exp = sorted(sm.brute_force(pats, E2E_SEQS, [text]))
    assert list(zip(go.tolist(), gq.tolist())) == exp
    assert {q for _, q in exp} == {0, 1, 2, 3} and len(exp) > 40
    assert m.path_taken(len(text)) == name
    rng = np.random.default_rng(2)
    cuts = np.sort(rng.integers(0, 12000, 49))
    texts = [text[a:b] for a, b in zip(np.r_[0, cuts], np.r_[cuts, 12000])] + [b""]
    texts = texts[:25] + [b""] + texts[25:50]
    assert len(texts) == 51 and sum(len(t) for t in texts) == 12000
    go, gq, last, info = m.scan_sequences(texts=texts)
    exp_t = sorted(sm.brute_force(pats, E2E_SEQS, texts))
    assert list(zip(go.tolist(), gq.tolist())) == exp_t
    whole = [x for x in exp if x[0] < 12000]
    assert 5 < len(exp_t) < len(whole)                            # a cut inside a signature loses it
    with pytest.raises(AcmError) as e:
        m.scan_sequences(text, out_capacity=len(exp) + 1)
    assert e.value.code == _lib.ACM_ERR_CAPACITY
    m.close()


def test_scan_sequences_mixed_and_anchored(gpu):
    """a mixed-case set (one part ignores case, one is exact), and a positioned first part (0, 0): the signature
    anchored at the start of its text"""
    pats = [(b"Head", True), (b"Body", False), (b"start", False), (b"end", False), (b"start", False), (b"end", False)]
    seqs = [([0, 1], [(1, 3)]), ([2, 3], [(0, None)]), ([4, 5], [(0, None)])]
    windows = {2: (0, 0, False)}
    texts = [b"head Body", b"HEAD body", b"hEAD..Body", b"Head....Body", b"start-end", b".start-end", b"startend start end",
             b"", b"end start", b"START end", b"headBody", b"Head BodyHead  Body"]
    for w in ({}, windows):
        a = sm.build(pats, seqs, windows=w)
        assert a.mixed_case and a.positioned == bool(w)
        m = Matcher(a, 0, max_text=4096)
        go, gq, last, info = m.scan_sequences(texts=texts)
        exp = sorted(sm.brute_force(pats, seqs, texts, windows=w))
        assert list(zip(go.tolist(), gq.tolist())) == exp, w
        got1 = [o for o, q in exp if q == 1]
        got2 = [o for o, q in exp if q == 2]
        assert len(got2) == 4 and len(got1) == (3 if w else 4) and sum(q == 0 for _, q in exp) == 4
        m.close()
