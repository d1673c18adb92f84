"""Rules on the device (acm_rule_matches_async, Matcher.scan_rules), cell for cell against the model of
tests/rule_model.py: synthetic planes at the record counts where the record-pass core and the radix passes can go
wrong, with texts and as one text that spans every tile and block; the edges of a comparison; nesting; a rule of
64 operands and a set of more than 255 slots; triggers; capacities; determinism and argument errors;
Matcher.scan_rules against a brute force.  Outputs and the workspace are poisoned before every call and guard
cells behind every output are checked.

The synthetic set has ten one-pattern sequences: eight are operands of four rules, one is an operand of none,
and the tenth pattern is in no sequence."""
import numpy as np
import pytest

import poison
import rule_model as rm
import sequence_model as sm
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16                                   # guard cells behind every output plane
NO_CELL = 0x7FFFFF00                         # no sequence index
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049]
BIG = 1024 * 1024 + 1025                     # 1026 tiles on 1024 blocks: a block owns two tiles; the sort spans every block
INT32_MAX = 0x7FFFFFFF

SYN_RULES = [([0, 1], "0&1"), ([2, 3, 4], "(0|1)>3|2"), ([5], "0>2"), ([6, 7], "0&1=0")]     # sequence 8 is in none
SYN_CELLS = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, NO_CELL, 9, 1, 4, 7]


def build(nseq, rules, extra=1):
    """a compiled Automaton of nseq one-pattern sequences (and extra patterns in no sequence) with the rules"""
    a = Automaton()
    for i in range(nseq + extra):
        a.add(b"<%04d>" % i, i)
    for i in range(nseq):
        a.add_sequence([i], [], iid=i)
    a.compile()
    for r, (ops, e) in enumerate(rules):
        assert a.add_rule(ops, e, iid=1000 + r) == r
    return a


def syn_planes(m):
    """(cells, offsets) of m records: random cells (a sequence, -1 or no sequence) in runs of equal offsets, a new
    offset one or two bytes on with probability 0.7"""
    rng = np.random.default_rng(4000 + m)
    cells = np.array(SYN_CELLS, dtype=np.int64)[rng.integers(0, len(SYN_CELLS), m)]
    offs = np.cumsum((rng.random(m) < 0.7) * rng.integers(1, 3, m)) + 3
    return cells, offs.astype(np.int64)


def syn_starts(text_end):
    """a text every 40 bytes from 40 on (the records in front are the lead's) over three quarters of the stream, an
    empty segment after every fifth, and two sentinels beyond the end"""
    s = []
    for k, x in enumerate(range(40, 3 * text_end // 4, 40)):
        s += [x, x] if k % 5 == 4 else [x]
    return s + [text_end + 100, INT32_MAX]


class Env:
    def __init__(self):
        self.model = rm.RuleModel(9, SYN_RULES)
        self.m = Matcher(build(9, SYN_RULES), 0, max_text=4096)
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


def call(matcher, planes, mr, cap, starts=(), fill=0xA5):
    """one call from poisoned outputs and a poisoned workspace; (rule plane, text plane, offset plane, info), each
    with its guard cells"""
    outs = [DeviceArray((cap + SLACK) * 4) for _ in range(3)]
    info = DeviceArray((4 + SLACK) * 4)
    poison.fill(outs + [info], P)
    nb = matcher.lib.acm_rule_workspace_bytes(matcher.dfa, mr)
    ws = DeviceArray(max(nb, 16))
    ws.fill(fill)
    S = len(starts)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int64).astype(np.int32), pad_to=0) if S else None
    matcher.rule_async(planes[0], planes[1], mr, outs[0], outs[1], outs[2], cap, info, seg_start=d_st, segments=S,
                       workspace=(ws.ptr, nb))
    out = tuple(x.to_numpy(np.int32, cap + SLACK) for x in outs) + (info.to_numpy(np.int32, 4 + SLACK),)
    for x in outs + [info, ws, d_st]:
        if x is not None:
            x.free()
    return out


def run_pass(matcher, model, planes, cells, offs, starts=(), cap=None, max_records=None, trailer=77, what=""):
    """one call compared whole with the model; returns the model's (rules, texts, offsets, info)"""
    m = len(cells)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    er, et, eo, einfo = model.run(cells[:mm], offs[:mm], starts)
    last = trailer if mm == m else int(cells[mm])
    cap = er.size + 9 if cap is None else cap
    gr, gt, go, gi = call(matcher, planes, mr, cap, starts)
    what = "%s m=%d max_records=%d cap=%d S=%d" % (what, m, mr, cap, len(starts))
    xr, xt, xo = rm.planes(er, et, eo, cap, PV, last)
    assert int(gr[0]) == int(gt[0]) == int(go[0]) == er.size, "%s: count %d/%d/%d, model %d" % (what, gr[0], gt[0], go[0], er.size)
    for name, g, x in (("rule", gr, xr), ("text", gt, xt), ("offset", go, xo)):
        assert np.array_equal(g[:cap], x), "%s: %s plane differs at %s" % (what, name, np.flatnonzero(g[:cap] != x)[:5])
        assert (g[cap:] == PV).all(), "%s: %s plane written behind the capacity" % (what, name)
    assert gi[:4].tolist() == einfo and (gi[4:] == PV).all(), "%s: info %s, model %s" % (what, gi[:6], einfo)
    return er, et, eo, einfo


def end_of(offs):
    return int(offs[-1]) + 1 if len(offs) else 4


# ------------------------------------------------------------------ 1. synthetic planes


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_synthetic_planes(env, m):
    cells, offs = env.planes(m)
    planes = upload(cells, offs)
    starts = syn_starts(end_of(offs))
    er, et, eo, einfo = run_pass(env.m, env.model, planes, cells, offs, starts=starts)
    one = run_pass(env.m, env.model, planes, cells, offs)                     # segments == 0: one text spans every cut
    assert (one[1] == -1).all() and one[0].size <= 4
    if m >= 1023:
        # neither empty nor everything: every rule holds somewhere and fails somewhere, and the texts matter
        assert set(er.tolist()) == ({0, 1, 2, 3} if m == BIG else {0, 1, 2}) and 0.1 * einfo[2] < er.size < 0.9 * einfo[2]
        assert einfo[0] > einfo[1] > einfo[2] > 0 and (np.diff(et) >= 0).all() and et[0] == -1
        assert set(one[0].tolist()) == {0, 1, 2}                             # "0&1=0" fails where both occur
    if m != BIG:
        for cap in sorted({max(er.size + 2, 2), max(er.size + 1, 2), max(er.size, 2), 2}):
            run_pass(env.m, env.model, planes, cells, offs, starts=starts, cap=cap)
        for mr in sorted({max(m - 1, 0), m // 2, m + 5}):
            run_pass(env.m, env.model, planes, cells, offs, starts=starts, max_records=mr)
    for x in planes:
        x.free()


@pytest.mark.parametrize("slice_len", [0, 2048, 2049])
def test_segment_slices(env, slice_len):
    """the starts tile 0 spans: none, exactly the LDS budget, one more (searched in global memory)"""
    m = 1025
    cells, offs = env.planes(m)
    starts = [end_of(offs) + 100] if slice_len == 0 else [0] + [4] * (slice_len - 1) + [700]
    planes = upload(cells, offs)
    run_pass(env.m, env.model, planes, cells, offs, starts=starts, what="slice")
    for x in planes:
        x.free()


def test_hostile_planes(env):
    """cells that are no sequence, offsets at the ends of int32, a count cell beyond max_records: nothing is read
    outside the planes and the tables and the model's records come out.  Offsets out of order are outside the
    contract: nothing may be written outside the planes, whatever comes out."""
    rng = np.random.default_rng(5)
    m = 1500
    edge = np.array([-(2 ** 31), -5, 0, 1, 39, 40, 41, 3000, 6003, 6004, INT32_MAX], dtype=np.int64)
    many = [0] + [4] * 2100 + [4096]
    cells = np.array(list(range(10)) + [-1, -(2 ** 31), INT32_MAX, NO_CELL, 10], dtype=np.int64)[rng.integers(0, 15, m)]
    offs = np.sort(np.concatenate([edge[rng.integers(0, 11, m // 2)], rng.integers(0, 6004, m - m // 2)]))
    for count in (m, INT32_MAX, -1):
        planes = upload(cells, offs, count=count)
        for starts in ([], syn_starts(6004), many, [-(2 ** 31), INT32_MAX]):
            run_pass(env.m, env.model, planes, cells, offs, starts=starts, what="hostile count=%d" % count)
        for x in planes:
            x.free()
    planes = upload(cells, rng.permutation(offs))
    for cap in (2, 300, 2 * m):
        gr, gt, go, gi = call(env.m, planes, m, cap, many)
        assert 0 <= gr[0] == gt[0] == go[0] <= m
        for g in (gr, gt, go):
            assert (g[cap:] == PV).all() and (g[min(int(g[0]) + 2, cap):cap] == PV).all() and g[min(int(g[0]) + 1, cap - 1)] == 77
        stored = min(int(gr[0]), cap - 2)
        assert ((gr[1:1 + stored] >= 0) & (gr[1:1 + stored] < 4)).all()
        assert ((gt[1:1 + stored] >= -1) & (gt[1:1 + stored] < len(many))).all()
        assert gi[0] == env.model.run(cells, offs)[3][0] and gi[0] >= gi[1] >= gi[2] >= gr[0] and gi[3] == 0
        assert (gi[4:] == PV).all()
    for x in planes:
        x.free()


# ------------------------------------------------------------------ 2. expressions

EDGE_RULES = [([0], "0=2"), ([1], "0>2"), ([2, 3], "0<2&1"), ([4, 5], "(0|1)>3"), ([6, 7], "0&1=0"),
              ([8], "(0|0|0)>5"), ([9, 10], "(" * 8 + "0" + ")" * 8 + "&1"), ([11, 12], "0|(1&((0=1|1>2)&0<3))")]


def test_expression_edges(gpu):
    """every text is 100 bytes; the cells of a text are listed as (sequence, how many)"""
    texts = [[(0, 1), (1, 1), (2, 1), (3, 1)],            # 0: counts 1: "0<2&1"
             [(0, 2), (1, 2), (2, 2), (3, 1)],            # 1: counts 2: "0=2"
             [(0, 3), (1, 3), (2, 3), (3, 1)],            # 2: counts 3: "0>2"
             [(3, 2)],                                    # 3: "0<2&1" with operand 0 at 0: 0 < 2 holds, and 1 occurs
             [(4, 2), (5, 2)],                            # 4: (0|1)>3 as 2 + 2
             [(4, 4)],                                    # 5: ... as 4 + 0
             [(4, 3)],                                    # 6: three: no
             [(5, 4)],                                    # 7: ... as 0 + 4: the trigger is an operand-1 record
             [(6, 2)],                                    # 8: 0&1=0: yes
             [(7, 1), (6, 1)],                            # 9: no
             [(7, 3)],                                    # 10: no
             [(8, 2)], [(8, 1)],                          # 11, 12: an operand named three times: 6 > 5, 3 > 5
             [(10, 1), (9, 1)], [(9, 1)],                 # 13, 14: nesting 8
             [(12, 3)], [(12, 2)], [(11, 1), (12, 1)]]    # 15 .. 17: four levels; 1>2 & 0<3; no; 0
    expect = [(2, 0), (0, 1), (1, 2), (2, 3), (3, 4), (3, 5), (3, 7), (4, 8), (5, 11), (6, 13), (7, 15), (7, 17)]
    cells, offs = [], []
    for k, t in enumerate(texts):
        at = 100 * k + 5
        for q, n in t:
            for _ in range(n):
                cells.append(q)
                offs.append(at)
                at += 3
    cells, offs = np.array(cells, dtype=np.int64), np.array(offs, dtype=np.int64)
    starts = [100 * k for k in range(len(texts))]
    model = rm.RuleModel(13, EDGE_RULES)
    m = Matcher(build(13, EDGE_RULES), 0, max_text=4096)
    planes = upload(cells, offs)
    er, et, eo, info = run_pass(m, model, planes, cells, offs, starts=starts, what="edges")
    assert list(zip(er.tolist(), et.tolist())) == expect
    assert eo.tolist()[:4] == [11, 105, 214, 305] and eo.tolist()[6] == 705 and eo.tolist()[9] == 1308
    assert info[:3] == [len(cells), sum(len(t) for t in texts), 24]
    for x in planes:
        x.free()
    m.close()


WIDE_RULES = [(list(range(60 * r, 60 * r + 60)),
               ["&".join("%d" % j for j in range(60)), "(" + "|".join("%d" % j for j in range(59)) + ")>2&59=0",
                "|".join("%d" % j for j in range(60)), "(0&1)|(2&3&4)|(5|6|7)>4|(8&(9|(10&(11|12))))",
                "59&0=0"][r]) for r in range(5)] + [(list(range(300, 364)), "|".join("%d" % j for j in range(64)))]


def test_wide_rules_and_triggers(gpu):
    """5 rules of 60 operands and one of 64: 364 slots, two radix passes.  A text where every operand of the rule of
    64 occurs gives exactly one record, at the first hit of operand 0; a text where only the last operand occurs"""
    model = rm.RuleModel(365, WIDE_RULES)
    m = Matcher(build(365, WIDE_RULES), 0, max_text=4096)
    rng = np.random.default_rng(8)
    cells = [list(rng.integers(0, 366, 400)) for _ in range(30)]
    cells[3] = list(range(363, 299, -1)) * 2                               # every operand, the highest first
    cells[4] = [364, 363, 20, 363]                                         # only the last operand (and strangers)
    cells[5] = list(range(60)) * 3                                         # rule 0 whole
    cells[6] = [59, 58, 57] + [59]                                         # rule 0: no
    cells[7] = list(range(60, 119)) + [100]                                # rule 1: 60 hits, no operand 59
    cells[8] = list(range(60, 120))                                        # ... with it
    flat = np.array([c for t in cells for c in t], dtype=np.int64)
    offs = np.concatenate([2000 * k + 4 * np.arange(len(t)) for k, t in enumerate(cells)]).astype(np.int64)
    starts = [2000 * k for k in range(len(cells))]
    planes = upload(flat, offs)
    er, et, eo, info = run_pass(m, model, planes, flat, offs, starts=starts, what="wide")
    got = {k: [(r, o) for r, t, o in zip(er.tolist(), et.tolist(), eo.tolist()) if t == k] for k in range(len(cells))}
    assert got[3] == [(5, 6000 + 4 * 63)] and got[4] == [(5, 8000 + 4)]
    assert got[5] == [(0, 10000)] and got[6] == [] and got[7] == [(1, 14000)] and got[8] == []
    assert len(set(er.tolist())) == 6
    run_pass(m, model, planes, flat, offs, what="wide, one text")
    for x in planes:
        x.free()
    m.close()


# ------------------------------------------------------------------ 3. determinism, no rules, errors


def test_determinism_and_stale_workspaces(env):
    m = 2049
    cells, offs = env.planes(m)
    planes = upload(cells, offs)
    starts = syn_starts(end_of(offs))
    runs = [call(env.m, planes, m, m + 2, starts, fill=f) for f in (0xA5, 0xA5, 0x00, 0xFF)]
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))
    assert runs[0][0][0] > 30
    for x in planes:
        x.free()


def test_set_without_rules(gpu):
    a = build(9, [])
    m = Matcher(a, 0, max_text=4096)
    cells, offs = syn_planes(300)
    planes = upload(cells, offs)
    for cap in (2, 3, 50):
        gr, gt, go, gi = call(m, planes, 300, cap)
        for g, x in zip((gr, gt, go), rm.planes([], [], [], cap, PV, 77)):
            assert np.array_equal(g[:cap], x) and (g[cap:] == PV).all()
        assert gi[:4].tolist() == [0, 0, 0, 0] and (gi[4:] == PV).all()
    r, t, o, info = m.scan_rules(b"<0001> <0002>")
    assert r.size == t.size == o.size == 0 and info.tolist() == [0, 0, 0, 0]
    for x in planes:
        x.free()
    m.close()


def test_rules_do_not_change_the_scan(gpu):
    """the same patterns and sequences with and without rules: the same scan and the same sequence records; the
    rule tables are the only device bytes added"""
    plain, ruled = Matcher(build(9, []), 0, max_text=4096), Matcher(build(9, SYN_RULES), 0, max_text=4096)
    text = b" ".join(b"<%04d>" % (i % 11) for i in range(300))
    x, y = plain.scan_sequences(text), ruled.scan_sequences(text)
    assert all(np.array_equal(a, b) for a, b in zip(x, y)) and x[0].size == 246
    assert 0 < ruled.device_bytes - plain.device_bytes <= 4096
    plain.close()
    ruled.close()


def test_argument_errors(env):
    m = env.m
    buf, out = DeviceArray(1 << 16), DeviceArray(1024 * 4)
    buf.fill(0)
    out.fill(P)
    ws = m.lib.acm_rule_workspace_bytes(m.dfa, 100)
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20, 1 << 22, 0x7FFFFFFE):
        b = m.lib.acm_rule_workspace_bytes(m.dfa, r)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    assert ws <= buf.nbytes
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, max_records=100, st=buf.ptr, S=4, ro=out.ptr, to=out.ptr + 512,
                oo=out.ptr + 2048, cap=100, info=out.ptr + 1024, ws=buf.ptr, ws_bytes=ws)
    bad = [dict(dfa=None), dict(sp=None), dict(so=None), dict(ro=None), dict(to=None), dict(oo=None), dict(info=None),
           dict(cap=1), dict(cap=0), dict(ws_bytes=ws - 1), dict(ws=None), dict(st=None), dict(max_records=0x7FFFFFFF),
           dict(S=0x80000000)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_rule_matches_async(x["dfa"], x["sp"], x["so"], x["max_records"], x["st"], x["S"], x["ro"], x["to"],
                                          x["oo"], x["cap"], x["info"], x["ws"], x["ws_bytes"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == PV).all()           # nothing was enqueued
    with pytest.raises(AcmError):
        m.rule_async(buf, buf, 100, out, out, out, 1, out)
    # the same call with good arguments is accepted (an empty plane: no records; its own workspace)
    w = DeviceArray(ws)
    m.rule_async(buf, buf, 100, out.ptr, out.ptr + 512, out.ptr + 2048, 100, out.ptr + 1024, seg_start=buf, segments=4,
                 workspace=(w.ptr, ws))
    for at in (0, 512, 2048):
        assert out.to_numpy(np.int32, 2, offset_bytes=at).tolist() == [0, 0]
    assert out.to_numpy(np.int32, 4, offset_bytes=1024).tolist() == [0, 0, 0, 0]
    for x in (buf, out, w):
        x.free()


# ------------------------------------------------------------------ 4. end to end

E2E_PATS = [b"needle", b"ab", b"cd", b"xy", b"hello", b"zz"]                  # as the signatures below add them
E2E_SEQS = [([0], []), ([1, 2], [(1, 3)]), ([3], []), ([4], []), ([5], [])]
E2E_RULES = [([0, 1], "0&1"), ([2, 3], "(0|1)>1"), ([4], "0=2")]


def e2e_automaton():
    """a plain pattern, a gap signature, an extended-syntax signature ([12]xy: a context in front of the anchor)
    and a nocase one; no two of them end in the same byte, so no two records share an offset"""
    a = Automaton()
    assert a.add_signature(b"needle".hex()) == 0
    assert a.add_signature("6162{1-3}6364") == 1
    assert a.add_signature("(31|32)7879", extended=True) == 2
    assert a.add_signature(b"hello".hex(), nocase=True) == 3
    assert a.add_signature(b"zz".hex()) == 4
    for r, (ops, e) in enumerate(E2E_RULES):
        assert a.add_rule(ops, e, iid=r) == r
    a.compile()
    return a


def e2e_records(texts):
    """(cells, offsets, starts) of the sequence records of the texts, by bytes.find"""
    recs, base, starts = [], 0, []
    for t in texts:
        t = bytes(t)
        starts.append(base)
        recs += [(base + k + 5, 0) for k in sm.occurrences(t, b"needle")]
        recs += [(base + e, 1) for e, q in sm.brute_force(E2E_PATS, E2E_SEQS, [t]) if q == 1]
        recs += [(base + k + 2, 2) for c in (b"1xy", b"2xy") for k in sm.occurrences(t, c)]
        recs += [(base + k + 4, 3) for k in sm.occurrences(t, b"hello", nocase=True)]
        recs += [(base + k + 1, 4) for k in sm.occurrences(t, b"zz")]
        base += len(t)
    recs.sort()
    assert len({o for o, _ in recs}) == len(recs)
    return [q for _, q in recs], [o for o, _ in recs], starts


def test_scan_rules(gpu):
    texts = [b"a needle, then ab.cd and abcd", b"needle ab....cd", b"ab..cd", b"needleneedle ab...cd abXcd",
             b"", b"1xy hello", b"1xy 2xy", b"HeLLo hello 3xy", b"hello", b"zz", b"zzz", b"z zz z zz", b"zz" * 150,
             b"1xyHELLOneedleab.cdzz.zz needle" + b"." * 300 + b"hello", b"", b"needle", b"ab.cd"]
    a = e2e_automaton()
    model = rm.RuleModel(5, E2E_RULES)
    m = Matcher(a, 0, max_text=8192)
    cells, offs, starts = e2e_records(texts)
    er, et, eo, einfo = model.run(cells, offs, starts)
    r, t, o, info = m.scan_rules(texts=texts)
    assert (r.tolist(), t.tolist(), o.tolist()) == (er.tolist(), et.tolist(), eo.tolist())
    assert info.tolist() == einfo
    assert [(x, y) for x, y in zip(er.tolist(), et.tolist())] == [(0, 0), (0, 3), (1, 5), (1, 6), (1, 7), (2, 10), (2, 11),
                                                                  (1, 13), (0, 13), (2, 13)]
    whole = b"".join(texts)
    cells, offs, _ = e2e_records([whole])
    er, et, eo, einfo = model.run(cells, offs)
    r, t, o, info = m.scan_rules(whole)
    assert (r.tolist(), t.tolist(), o.tolist()) == (er.tolist(), et.tolist(), eo.tolist()) and info.tolist() == einfo
    assert er.tolist() == [0, 1] and (et == -1).all()                       # 150 + x "zz": "0=2" fails
    with pytest.raises(AcmError) as e:
        m.scan_rules(texts=texts, out_capacity=5)
    assert e.value.code == _lib.ACM_ERR_CAPACITY
    m.close()
