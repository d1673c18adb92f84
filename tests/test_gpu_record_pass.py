"""The record-pass core (csrc/record_pass.h, csrc/entry_pass.h) through every pass that uses it -- segment,
word, tally, line select, expand, case, position -- at the record counts where tile ownership, ordered ranks
and the header / trailer cells can go wrong.  Planes are built by hand in numpy; expected outputs are plain numpy and the models of the
suite, never the library.

The automaton is {a, ba, cba}: the state of "cba" lists three patterns, of "ba" two, of "a" one.  Record i
ends at offset 4 i + 3 and holds one of those states or (a quarter of the records) a value that is no state
and is dropped by segment, word and tally: the kept records are an arbitrary subset, known on the host.
A record's kind is its longest pattern's length; its match list holds that pattern and every shorter one,
in the oracle's order.
Starts are multiples of 4, so every record lies 4 bytes or more into its segment and no state is clamped.

The case pass has a mixed automaton of its own over the same idea, {a, bA, cba (ignoring case), Dcba}: kinds
1..4 with lists of 1..4 entries, the four bytes under a record in a case drawn per byte, so that which of
a record's exact entries hold -- 0 to 3 cells per record in the all form -- is known on the host only.  The
text starts two bytes into record 0, whose longer entries reach into `before`."""
import numpy as np
import pytest

import case_model as cm
import line_model
import orc
import poison
import tally_model
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib

pytestmark = pytest.mark.gpu

PATS = [b"a", b"ba", b"cba"]
NO_STATE = 0x7FFFFF00
WORD = b"x"                                  # the word set: every other byte bounds a word
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049]
BIG = 1024 * 1024 + 1025                     # some blocks own two tiles, the last tile is partial
P = poison.PLANE_POISON
PV = poison.cell(P)


class Env:
    def __init__(self):
        a = Automaton()
        for p in PATS:
            a.add(p)
        a.compile()
        self.m = Matcher(a, 0, max_text=4096)
        self.num_states = a.num_states
        o = orc.Oracle()
        for i, p in enumerate(PATS):
            o.add(p, i)
        o.compile()
        self.state = {k: int(o.scan(PATS[k - 1])[2]) for k in (1, 2, 3)}   # kind -> state
        self.lists = np.full((4, 3), -1, dtype=np.int32)                     # [kind, j] -> pattern
        for k in (1, 2, 3):
            lst = o.match_list(self.state[k])
            assert sorted(lst) == list(range(k))
            self.lists[k, :k] = lst
        self.cache = {}

    def planes(self, m, valid_only=False):
        """(kinds, offsets, host state plane, device state plane, device offset plane, text) of m records"""
        key = (m, valid_only)
        if key not in self.cache:
            if m >= BIG:
                self.cache = {k: v for k, v in self.cache.items() if k[0] < BIG}
            rng = np.random.default_rng(1000 + m)
            kind = rng.integers(1 if valid_only else 0, 4, m)
            off = (np.arange(m, dtype=np.int64) * 4 + 3).astype(np.int32)
            lut = np.array([NO_STATE, self.state[1], self.state[2], self.state[3]], dtype=np.int32)
            sp = np.concatenate([[m], lut[kind], [self.state[1]]]).astype(np.int32)
            op = np.concatenate([[m], off, [self.state[1]]]).astype(np.int32)
            text = rng.choice(np.frombuffer(b" x", dtype=np.uint8), 4 * m + 4)
            for k in (1, 2, 3):   # the bytes of the record's longest pattern end at its offset
                sel = off[kind == k].astype(np.int64)
                for j, c in enumerate(PATS[k - 1][::-1]):
                    text[sel - j] = c
            self.cache[key] = (kind, off, sp, DeviceArray.from_numpy(sp), DeviceArray.from_numpy(op), text)
        return self.cache[key]


@pytest.fixture(scope="module")
def env(gpu):
    e = Env()
    yield e
    e.m.close()


def max_records_of(m):
    return sorted({max(m - 1, 0), m, m + 5})


def caps_of(total):
    """total + 2 == cap, total + 1 == cap, total >= cap; and room to spare"""
    return sorted({max(total + 2, 2), max(total + 1, 2), max(total, 2), total + 9})


def entries(env, kind, off, all_patterns):
    """(offsets, patterns, record index, index in the list) of the match-list entries of the valid records"""
    n = np.where(kind > 0, kind if all_patterns else 1, 0)
    rec = np.repeat(np.arange(kind.size), n)
    j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
    return off[rec], env.lists[kind[rec], j], rec, j


def out_planes(cap, count=2):
    bufs = [DeviceArray(cap * 4) for _ in range(count)]
    poison.fill(bufs, P)
    return bufs


def poisoned_ws(nbytes):
    ws = DeviceArray(max(nbytes, 16))
    ws.fill(0xA5)
    return ws


# ------------------------------------------------------------------ segment


def check_segment(env, m, starts, report, with_seg, with_counts, max_records=None, cap=None):
    kind, off, sp, d_sp, d_op, _ = env.planes(m)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    keep = kind[:mm] > 0
    S = len(starts)
    seg = np.searchsorted(np.asarray(starts, dtype=np.int64), off[:mm], side="right").astype(np.int32) - 1
    val = env.lists[kind[:mm], 0] if report == _lib.REPORT_HEAD else sp[1:1 + mm]
    exp = (off[:mm][keep], val[keep].astype(np.int32), int(sp[1 + mm]))
    total = int(keep.sum())
    cap = total + 9 if cap is None else cap
    pat, o, sg = out_planes(cap, 3)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int32), pad_to=0) if S else None
    cnt = DeviceArray(max(S, 1) * 4)
    cnt.fill(P)
    nb = env.m.lib.acm_segment_workspace_bytes(mr)
    ws = poisoned_ws(nb)
    env.m.segment_async(d_sp, d_op, mr, d_st, S, 4 * m + 4, pat, o, cap, seg_out=sg if with_seg else None,
                        seg_counts=cnt if with_counts and S else None, report=report, workspace=(ws.ptr, nb))
    what = "segment m=%d max_records=%d cap=%d S=%d" % (m, mr, cap, S)
    poison.check_planes(pat, o, cap, exp, what=what)
    got = sg.to_numpy(np.int32, cap)
    if with_seg:
        stored = min(total, cap - 2)
        assert got[0] == total and np.array_equal(got[1:1 + stored], seg[keep][:stored]), what
        assert got[stored + 1] == exp[2] and np.all(got[stored + 2:] == PV), what
    else:
        assert np.all(got == PV), what
    if with_counts and S:
        k = seg[keep]
        assert np.array_equal(cnt.to_numpy(np.int32, S), np.bincount(k[k >= 0], minlength=S)), what


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_segment(env, m):
    starts = np.arange(0, 4 * m + 4, 12 * 4, dtype=np.int64)
    for report in (_lib.REPORT_HEAD, _lib.REPORT_STATE):
        for with_seg in (True, False):
            for with_counts in (True, False):
                check_segment(env, m, starts, report, with_seg, with_counts)
    if m == BIG:
        return
    check_segment(env, m, [], _lib.REPORT_HEAD, True, False)
    total = int((env.planes(m)[0] > 0).sum())
    for mr in max_records_of(m):
        check_segment(env, m, starts, _lib.REPORT_HEAD, True, True, max_records=mr)
    for cap in caps_of(total):
        check_segment(env, m, starts, _lib.REPORT_STATE, True, True, cap=cap)


@pytest.mark.parametrize("slice_len", [0, 2048, 2049])
def test_segment_slice(env, slice_len):
    """the slice of starts that tile 0 spans: empty, exactly the LDS budget, one more (searched in global
    memory); tile 1 of the 1025 records follows with a slice of its own"""
    m = 1025
    starts = [4 * m + 100] if slice_len == 0 else [0] + [4] * (slice_len - 1) + [4096]
    check_segment(env, m, starts, _lib.REPORT_HEAD, True, True)


# ------------------------------------------------------------------ word


def word_expected(env, m, mr, all_patterns):
    kind, off, sp, _, _, text = env.planes(m)
    mm = min(m, mr)
    eo, ep, rec, j = entries(env, kind[:mm], off[:mm], True)
    is_w = text == WORD[0]
    ok = ~is_w[eo.astype(np.int64) + 1] & ~is_w[eo.astype(np.int64) - (ep + 1)]   # pattern p is p + 1 bytes long
    if not all_patterns:   # the first word-bounded entry of each record
        seen = np.zeros(kind.size, dtype=bool)
        pick = np.zeros(rec.size, dtype=bool)
        for step in range(3):
            sel = ok & (j == step) & ~seen[rec]
            pick |= sel
            seen[rec[sel]] = True
        ok = pick
    return eo[ok], ep[ok], int(sp[1 + mm])


def check_word(env, m, all_patterns, max_records=None, cap=None):
    _, _, _, d_sp, d_op, text = env.planes(m)
    mr = m if max_records is None else max_records
    exp = word_expected(env, m, mr, all_patterns)
    cap = len(exp[0]) + 9 if cap is None else cap
    pat, o = out_planes(cap)
    nb = env.m.lib.acm_word_workspace_bytes(mr)
    ws = poisoned_ws(nb)
    d_text = DeviceArray.from_numpy(text)
    env.m.word_async(d_sp, d_op, mr, d_text, 0, text.size, pat, o, cap, word_mask=Matcher.word_mask(WORD),
                     all_patterns=all_patterns, workspace=(ws.ptr, nb))
    poison.check_planes(pat, o, cap, exp, what="word m=%d max_records=%d cap=%d all=%d" % (m, mr, cap, all_patterns))
    return exp


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_word(env, m):
    for all_patterns in (False, True):
        exp = check_word(env, m, all_patterns)
        if m == BIG:
            continue
        for mr in max_records_of(m):
            check_word(env, m, all_patterns, max_records=mr)
        for cap in caps_of(len(exp[0])):
            check_word(env, m, all_patterns, cap=cap)


def test_word_list_across_the_cut(env):
    """a record whose list writes entries on both sides of the cap - 2 cut"""
    m = 257
    eo, _, _ = word_expected(env, m, m, True)
    i = int(np.flatnonzero((eo[1:] == eo[:-1]))[-1])   # entries i and i + 1 are one record's
    check_word(env, m, True, cap=i + 1 + 2)


# ------------------------------------------------------------------ word, case and position alike


@pytest.mark.parametrize("m", [0, 65, 1025, 2049])
def test_entry_passes_agree(env, m):
    """The word, case and position (STATE input) passes are one skeleton (csrc/entry_pass.h) around three
    predicates.  Where no predicate drops anything -- no byte of the text is a word byte, the automaton is
    neither mixed nor positioned, there are no segments -- the three write the same planes cell for cell: the
    match lists of the valid records (head: their first entries), on a plane that holds them all and on one
    that is a cell short."""
    kind, off, sp, d_sp, d_op, text = env.planes(m)
    assert ord("#") not in text
    d_text = DeviceArray.from_numpy(text)
    for all_patterns in (False, True):
        eo, ep, _, _ = entries(env, kind, off, all_patterns)
        exp = (eo, ep, int(sp[1 + m]))
        for cap in sorted({len(eo) + 2, max(len(eo) + 1, 2)}):
            got = {}
            for name in ("word", "case", "position"):
                pat, o = out_planes(cap)
                nb = getattr(env.m.lib, "acm_%s_workspace_bytes" % name)(m)
                ws = poisoned_ws(nb)
                what = "%s m=%d cap=%d all=%d" % (name, m, cap, all_patterns)
                if name == "word":
                    env.m.word_async(d_sp, d_op, m, d_text, 0, text.size, pat, o, cap, word_mask=Matcher.word_mask(b"#"),
                                     all_patterns=all_patterns, workspace=(ws.ptr, nb))
                elif name == "case":
                    env.m.case_async(d_sp, d_op, m, d_text, 0, text.size, pat, o, cap, all_patterns=all_patterns,
                                     workspace=(ws.ptr, nb))
                else:
                    info = DeviceArray(16)
                    info.fill(P)
                    env.m.position_async(d_sp, d_op, m, pat, o, cap, info, report=_lib.REPORT_STATE, text_end=text.size,
                                         open_end=text.size, all_patterns=all_patterns, workspace=(ws.ptr, nb))
                    assert info.to_numpy(np.int32, 4).tolist() == [0, 0, 0, 0], what
                    info.free()
                poison.check_planes(pat, o, cap, exp, what=what)
                got[name] = (pat.to_numpy(np.int32, cap), o.to_numpy(np.int32, cap))
                for x in (pat, o, ws):
                    x.free()
            for name in ("case", "position"):
                for a, b in zip(got["word"], got[name]):
                    assert np.array_equal(a, b), "word and %s differ, m=%d cap=%d all=%d" % (name, m, cap, all_patterns)
    d_text.free()


# ------------------------------------------------------------------ tally


def check_tally(env, m, all_patterns, starts, class_of=None, C=3, max_records=None):
    kind, off, _, d_sp, d_op, _ = env.planes(m)
    mr = m if max_records is None else max_records
    mm = min(m, mr)
    eo, ep, _, _ = entries(env, kind[:mm], off[:mm], all_patterns)
    S = len(starts)
    exp = tally_model.tally(eo, ep, class_of, C, np.asarray(starts, dtype=np.int64) if S else None)
    tot, rows, lead = DeviceArray(C * 8), DeviceArray(max(S * C, 1) * 4), DeviceArray(C * 4)
    poison.fill([tot, rows, lead], P)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int32), pad_to=0) if S else None
    d_map = DeviceArray.from_numpy(np.asarray(class_of, dtype=np.int32), pad_to=0) if class_of is not None else None
    nb = env.m.lib.acm_tally_workspace_bytes(mr, C)
    ws = poisoned_ws(nb)
    env.m.tally_async(d_sp, d_op, mr, tot, report=_lib.REPORT_STATE, all_patterns=all_patterns, class_of=d_map,
                      num_classes=C, seg_start=d_st, segments=S, seg_class=rows if S else None, lead=lead,
                      workspace=(ws.ptr, nb))
    what = "tally m=%d max_records=%d all=%d S=%d C=%d" % (m, mr, all_patterns, S, C)
    assert np.array_equal(tot.to_numpy(np.uint64, C), exp[0]), what
    assert np.array_equal(lead.to_numpy(np.int32, C), exp[2]), what
    if S:
        assert np.array_equal(rows.to_numpy(np.int32, S * C).reshape(S, C), exp[1]), what


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_tally(env, m):
    starts = np.arange(48, 4 * m + 4, 12 * 4, dtype=np.int64)   # the first records are the lead's
    for all_patterns in (False, True):
        check_tally(env, m, all_patterns, [])
        check_tally(env, m, all_patterns, starts)
    if m != BIG:
        for mr in max_records_of(m):
            check_tally(env, m, True, starts, max_records=mr)


@pytest.mark.parametrize("n_rows,C,class_of", [(1024, 2, [0, 1, 0]), (683, 3, None), (682, 3, None)])
def test_tally_rows_in_lds_and_not(env, n_rows, C, class_of):
    """the rows of tile 0 times the classes: 2048 cells (the LDS budget), 2049 (global atomics), 2046"""
    starts = [0] + list(range(4, 4 * n_rows, 4)) + [4096]
    assert len(starts) == n_rows + 1
    check_tally(env, 1025, True, starts, class_of=class_of, C=C)


# ------------------------------------------------------------------ line select


@pytest.mark.parametrize("lines", [1, 31, 32, 33, 256 * 32, 256 * 32 + 1])
@pytest.mark.parametrize("lead", [False, True])
def test_line_select(env, lines, lead):
    m = 1025
    _, off, _, _, d_op, _ = env.planes(m)
    L = lines - (1 if lead else 0)
    end = 4 * m + 4
    rng = np.random.default_rng(lines)
    # starts over the offsets' span and beyond it, so that some lines hold records and some none
    st = np.sort(rng.choice(np.arange(1 if lead else 0, 3 * end), L, replace=False)).astype(np.int64)
    if not lead and L:
        st[0] = 0
    end = int(max(end, st[-1] + 1 if L else end))
    capacity = L + 3
    ls = np.full(capacity, 0x7FFFFFFF, dtype=np.int32)
    ls[:L] = st
    info = np.array([L, L, 0 if lead else 1, 0, 0, 0, 0, 0], dtype=np.int32)
    d_ls, d_info = DeviceArray.from_numpy(ls, pad_to=0), DeviceArray.from_numpy(info, pad_to=0)
    nb = env.m.lib.acm_line_select_workspace_bytes(capacity)
    for invert in (False, True):
        ent = line_model.select(st, info, 0, end, off, invert=invert)
        for cap in caps_of(len(ent[0])):
            outs = out_planes(cap, 3)
            ws = poisoned_ws(nb)
            env.m.line_select_async(d_ls, capacity, d_info, 0, end, d_op, m, outs[0], outs[1], outs[2], cap,
                                    invert=invert, workspace=(ws.ptr, nb))
            for got, exp in zip(outs, line_model.planes(ent, cap, PV)):
                assert np.array_equal(got.to_numpy(np.int32, cap), exp), "lines=%d lead=%d invert=%d cap=%d" % (
                    lines, lead, invert, cap)


# ------------------------------------------------------------------ expand


@pytest.mark.parametrize("m", [1, 65, 257, 1025])
def test_expand_header_and_trailer(env, m):
    kind, off, sp, d_sp, d_op, _ = env.planes(m, valid_only=True)
    for mr in max_records_of(m):
        if mr == 0:
            continue
        mm = min(m, mr)
        eo, ep, _, _ = entries(env, kind[:mm], off[:mm], True)
        exp = (eo, ep, int(sp[1 + mm]))
        nb = env.m.lib.acm_expand_workspace_bytes(mr)
        for cap in caps_of(len(eo)):
            pat, o = out_planes(cap)
            ws = poisoned_ws(nb)
            _lib.check(env.m.lib.acm_expand_matches_async(env.m.dfa, d_sp.ptr, d_op.ptr, mr, pat.ptr, o.ptr, cap, ws.ptr,
                                                          nb, None), "acm_expand_matches_async")
            poison.check_planes(pat, o, cap, exp, what="expand m=%d max_records=%d cap=%d" % (m, mr, cap))


# ------------------------------------------------------------------ case

CASE_PATS = [(b"a", False), (b"bA", False), (b"cba", True), (b"Dcba", False)]
CASE_BYTES = np.frombuffer(b"Dcba", dtype=np.uint8)
CASE_ORIGIN = 2                              # the text starts here: bytes 0 and 1 of the stream are `before`
CUT_RECORDS = (1023, 1024)                   # the last record of tile 0, the first of tile 1: three kept entries each
SLACK = 16                                   # guard cells behind the case pass's output planes


class CaseEnv:
    def __init__(self):
        self.model = cm.CaseModel(CASE_PATS)
        a = cm.build(CASE_PATS)
        assert a.mixed_case
        self.m = Matcher(a, 0, max_text=4096)
        self.state = {k: int(self.model.walk(b"dcba"[4 - k:])[2]) for k in (1, 2, 3, 4)}   # kind -> state
        self.lists = np.full((5, 4), -1, dtype=np.int32)                                    # [kind, j] -> pattern
        for k in (1, 2, 3, 4):
            lst = self.model.list_of(self.state[k])
            assert sorted(lst) == list(range(k))
            self.lists[k, :k] = lst
        self.cache = {}

    def planes(self, m):
        """(kinds, offsets, host state plane, device state plane, device offset plane, stream bytes, device
        stream, holds[record, pattern]) of m records.  Record 0 and, beyond 1024 records, the records either
        side of the first tile cut are "Dcba" whole."""
        if m not in self.cache:
            rng = np.random.default_rng(3000 + m)
            kind = rng.integers(1, 5, m)
            kind[rng.random(m) < 0.25] = 0
            text = np.where(rng.random((m + 1, 4)) < 0.7, CASE_BYTES, CASE_BYTES ^ 0x20).astype(np.uint8)
            for i in ((0,) if m else ()) + (CUT_RECORDS if m > 1025 else ()):
                kind[i], text[i] = 4, CASE_BYTES
            off = (np.arange(m, dtype=np.int64) * 4 + 3).astype(np.int32)
            lut = np.array([NO_STATE] + [self.state[k] for k in (1, 2, 3, 4)], dtype=np.int32)
            sp = np.concatenate([[m], lut[kind], [self.state[1]]]).astype(np.int32)
            op = np.concatenate([[m], off, [self.state[1]]]).astype(np.int32)
            t = text[:m]
            holds = np.stack([t[:, 3] == ord("a"), (t[:, 2] == ord("b")) & (t[:, 3] == ord("A")),
                              np.ones(m, dtype=bool), (t == CASE_BYTES).all(axis=1)], axis=1)
            text = text.reshape(-1)
            self.cache[m] = (kind, off, sp, DeviceArray.from_numpy(sp), DeviceArray.from_numpy(op), text,
                             DeviceArray.from_numpy(text), holds)
        return self.cache[m]


@pytest.fixture(scope="module")
def cenv(gpu):
    e = CaseEnv()
    yield e
    for v in e.cache.values():
        for x in v:
            if isinstance(x, DeviceArray):
                x.free()
    e.m.close()


def case_expected(cenv, m, mr, all_patterns):
    """(offsets, patterns, trailer): every entry of the first min(m, mr) records that holds, or the first of
    each record, by numpy alone"""
    kind, off, sp, _, _, _, _, holds = cenv.planes(m)
    mm = min(m, mr)
    n = kind[:mm]
    rec = np.repeat(np.arange(mm), n)
    start = np.cumsum(n) - n
    j = np.arange(rec.size) - np.repeat(start, n)
    p = cenv.lists[kind[rec], j]
    keep = holds[rec, p]
    if not all_patterns and rec.size:
        ahead = np.cumsum(keep) - keep                       # kept entries in front, all records
        keep &= ahead == np.repeat(ahead[np.minimum(start, rec.size - 1)], n)
    return off[rec][keep], p[keep], int(sp[1 + mm])


def check_case(cenv, m, all_patterns, max_records=None, cap=None):
    _, _, _, d_sp, d_op, text, d_text, _ = cenv.planes(m)
    mr = m if max_records is None else max_records
    eo, ep, last = case_expected(cenv, m, mr, all_patterns)
    cap = len(eo) + 9 if cap is None else cap
    pat, o = out_planes(cap + SLACK)
    tail = DeviceArray(64)
    tail.fill(P)
    nb = cenv.m.lib.acm_case_workspace_bytes(mr)
    ws = poisoned_ws(nb)
    d_before = DeviceArray.from_numpy(text[:CASE_ORIGIN])
    cenv.m.case_async(d_sp, d_op, mr, d_text.ptr + CASE_ORIGIN, CASE_ORIGIN, text.size, pat, o, cap, before=d_before,
                      before_len=CASE_ORIGIN, all_patterns=all_patterns, tail_out=tail, workspace=(ws.ptr, nb))
    what = "case m=%d max_records=%d cap=%d all=%d" % (m, mr, cap, all_patterns)
    for got, exp in zip((pat, o), cm.planes(ep, eo, cap, PV, last)):
        got = got.to_numpy(np.int32, cap + SLACK)
        assert int(got[0]) == len(eo), "%s: count %d, expected %d" % (what, got[0], len(eo))
        assert np.array_equal(got[:cap], exp), "%s: plane differs at %s" % (what, np.flatnonzero(got[:cap] != exp)[:5])
        assert np.all(got[cap:] == PV), what + ": written behind the capacity"
    tb = tail.to_numpy(np.uint8, 64)
    assert np.array_equal(tb[:4], text[-4:]) and np.all(tb[4:] == P), what + ": tail"
    for x in (pat, o, tail, ws, d_before):
        x.free()
    return eo, ep, last


@pytest.mark.parametrize("m", COUNTS + [BIG])
def test_case(cenv, m):
    for all_patterns in (False, True):
        exp = check_case(cenv, m, all_patterns)
        if m == BIG:
            assert len(exp[0]) > m // 2
            continue
        # the numpy expectation is the model's
        _, off, sp, _, _, text, _, _ = cenv.planes(m)
        mp, mo = cenv.model.filter(sp[1:1 + m], off, text[CASE_ORIGIN:], all_patterns, CASE_ORIGIN,
                                   bytes(text[:CASE_ORIGIN]))
        assert np.array_equal(mp, exp[1]) and np.array_equal(mo, exp[0]), "m=%d all=%d" % (m, all_patterns)
        for mr in max_records_of(m):
            check_case(cenv, m, all_patterns, max_records=mr)
        for cap in caps_of(len(exp[0])):
            check_case(cenv, m, all_patterns, cap=cap)


@pytest.mark.parametrize("m", [2049, BIG])
def test_case_list_across_the_cut(cenv, m):
    """cap - 2 falls inside the list of the last record of tile 0, then of the first record of tile 1: two
    blocks' tiles at 2049 records, the two tiles of block 0 at the big count"""
    eo, ep, _ = case_expected(cenv, m, m, True)
    for i in CUT_RECORDS:
        at = int(np.searchsorted(eo, 4 * i + 3))
        assert eo[at:at + 3].tolist() == [4 * i + 3] * 3 and sorted(ep[at:at + 3].tolist()) == [0, 2, 3]
        for stored in (at + 1, at + 2):       # one entry of the record in front of the cut, then two
            check_case(cenv, m, True, cap=stored + 2)
