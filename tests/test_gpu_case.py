"""Case sensitivity per pattern on the device (acm_case_matches_async, Matcher.scan_case): the records of
a mixed automaton's scan, made exact, compared cell for cell with the model of tests/case_model.py; the
same set through every scan route; a cross-check against the case-sensitive automaton that does not use
the model; automata that are not mixed; streaming, the state carried out of an overflowed plane, segments,
overflow, bounds and argument errors."""
import functools

import numpy as np
import pytest

import case_model as cm
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib

pytestmark = pytest.mark.gpu

POISON_BYTE = 0xA5
POISON = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])

# exact and caseless patterns in one state's list (abc / ABC / aBc); lengths 1, 3, 7, 8, 9, 16, 17 and 33;
# bytes that differ only in bit 5 and are no letters (@ `, [ {); bytes >= 0x80
LONG = [
    (b"abc", False), (b"ABC", False), (b"aBc", True),
    (b"abcdefa", False), (b"AbCdEfA", False),
    (b"bcdefabc", False),
    (b"cdefabcde", False), (b"CDEFABCDE", True),
    (b"defabcdefabcdefa", False),
    (b"efabcdEfabcdefabc", False),
    (b"fAbcdeFabcdefabcDefabcdefaBcdefabc"[:33], False),
    (b"a@b[c", False), (b"a`b{c", False), (b"A@B[C", True),
    (b"\xe1bc\xc1de\x80f", False), (b"\xe1BC\xc1dE\x80F", False), (b"\xc1bc\xe1de\x80f", True),
]
FULL = LONG + [(b"d", False), (b"E", True), (b"", False)]
assert sorted({len(p) for p, _ in FULL}) == [0, 1, 3, 5, 7, 8, 9, 16, 17, 33]


@functools.lru_cache(maxsize=None)
def model_of(name):
    return cm.CaseModel({"full": FULL, "long": LONG}[name])


@functools.lru_cache(maxsize=None)
def text_of(name, tokens, seed, gap=5):
    t = cm.planted_text({"full": FULL, "long": LONG}[name], tokens, seed, filler=b" .,\n0123456789", gap=gap)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def expected(name, tokens, seed, all_patterns, gap=5):
    return model_of(name).records(text_of(name, tokens, seed, gap), all_patterns)


def poisoned(cells):
    d = DeviceArray(max(cells * 4, 16))
    d.fill(POISON_BYTE)
    return d


def same(got, exp, what):
    assert got[0].size == exp[0].size, "%s: %d records, expected %d" % (what, got[0].size, exp[0].size)
    assert np.array_equal(got[0], exp[0]), "%s: offsets differ" % what
    assert np.array_equal(got[1], exp[1]), "%s: patterns differ" % what
    assert got[2] == exp[2], "%s: final state %d != %d" % (what, got[2], exp[2])


def case_planes(m, sp, so, max_records, d_text, origin, end, ocap, all_patterns, slack=16, **kw):
    """the output planes of one call, whole (ocap cells and slack cells behind them), from poisoned buffers"""
    pat, off = poisoned(ocap + slack), poisoned(ocap + slack)
    m.case_async(sp, so, max_records, d_text, origin, end, pat, off, ocap, all_patterns=all_patterns, **kw)
    p, o = pat.to_numpy(np.int32, ocap + slack), off.to_numpy(np.int32, ocap + slack)
    pat.free()
    off.free()
    return p, o


def check_planes(got, pats, offs, cap, trailer, what):
    ep, eo = cm.planes(pats, offs, cap, POISON, trailer)
    p, o = got
    assert int(p[0]) == len(pats), "%s: count %d, model %d" % (what, int(p[0]), len(pats))
    assert np.array_equal(p[:cap], ep), "%s: pattern plane differs at %s" % (what, np.flatnonzero(p[:cap] != ep)[:5])
    assert np.array_equal(o[:cap], eo), "%s: offset plane differs at %s" % (what, np.flatnonzero(o[:cap] != eo)[:5])
    assert (p[cap:] == POISON).all() and (o[cap:] == POISON).all(), "%s: written behind the capacity" % what


@pytest.mark.parametrize("tokens,lo,hi", [(660, 2500, 3600), (15000, 65000, 78000)], ids=["3k", "70k"])
def test_against_model(gpu, tokens, lo, hi):
    a = cm.build(FULL)
    assert a.mixed_case and not a.nocase
    model = model_of("full")
    text = text_of("full", tokens, 5)
    states, offs, last = model.walk(text)
    assert lo < states.size < hi, states.size
    m = Matcher(a, 0, max_text=text.size)
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    # the candidates are the nocase automaton's records
    sp = m.pat_plane.to_numpy(np.int32, states.size + 2)
    so = m.off_plane.to_numpy(np.int32, states.size + 2)
    assert int(sp[0]) == states.size and int(sp[-1]) == last
    assert np.array_equal(sp[1:-1], states) and np.array_equal(so[1:-1], offs)
    every = 0
    for all_patterns in (False, True):
        eo, ep, _ = expected("full", tokens, 5, all_patterns)
        ocap = eo.size + 2 + 7
        got = case_planes(m, m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, ocap, all_patterns)
        check_planes(got, ep, eo, ocap, last, "all" if all_patterns else "head")
        every = eo.size
    # most candidates fail, some of every pattern hold
    entries = sum(len(model.list_of(int(s))) for s in states)
    assert every < entries * 0.7
    assert set(ep.tolist()) == {i for i, (p, _) in enumerate(FULL) if p}
    # the Python front end gives the same records
    same(m.scan_case(text, True), expected("full", tokens, 5, True), "scan_case all")
    same(m.scan_case(text, False), expected("full", tokens, 5, False), "scan_case head")
    d.free()
    m.close()


ROUTES = {
    "sparse": ("sparse", {"ACM_SCAN_NO_LDSWALK": "1"}, False),
    "chain": ("chain", {"ACM_SCAN_NO_LDSWALK": "1"}, False),
    "lds": ("chain", {}, True),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_routes(gpu, monkeypatch, route):
    mode, env, lds = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = cm.build(LONG)
    assert a.mixed_case
    text = text_of("long", 4000, 11, 48)
    m = Matcher(a, 0, max_text=text.size)
    assert m.set_mode(mode) == mode
    assert m.lds_resident() == lds
    if mode == "sparse":
        assert m.sparse_eligible()
    for all_patterns in (False, True):
        same(m.scan_case(text, all_patterns), expected("long", 4000, 11, all_patterns, 48),
             "%s %s" % (route, "all" if all_patterns else "head"))
    assert m.path_taken(text.size) == mode
    m.close()


def test_cross_check_without_model(gpu):
    """all patterns exact plus one caseless pattern that never occurs: the all form's pairs are those of
    the case-sensitive automaton of the exact patterns"""
    exact = [p for p, _ in LONG]
    mixed = cm.build([(p, False) for p in exact] + [(b"zzzzqqqq", True)])
    assert mixed.mixed_case
    plain = cm.build([(p, False) for p in exact])
    assert not plain.mixed_case and not plain.nocase
    text = text_of("long", 4000, 11, 48)
    m1, m2 = Matcher(mixed, 0, max_text=text.size), Matcher(plain, 0, max_text=text.size)
    go, gp, _ = m1.scan_case(text, True)
    eo, ep, _ = m2.scan_all(text)
    got, exp = list(zip(go.tolist(), gp.tolist())), list(zip(eo.tolist(), ep.tolist()))
    assert len(exp) > 1000 and len(got) == len(set(got))
    assert set(got) == set(exp)
    assert go.tolist() == sorted(go.tolist())
    # and the candidates were more than that
    assert m1.scan_all(text)[0].size > len(exp)
    m1.close()
    m2.close()


@pytest.mark.parametrize("nocase", [False, True], ids=["case", "nocase"])
def test_not_mixed(gpu, nocase):
    """legal, and every entry is kept: the HEAD scan's records and the expansion, bit for bit (a set without
    an empty pattern: the scan reports one, the pass never does)"""
    a = cm.build([(p, False) for p, _ in FULL if p], nocase=nocase)
    assert not a.mixed_case and a.nocase == nocase
    text = text_of("full", 560, 5)
    m = Matcher(a, 0, max_text=text.size)
    head, every = m.scan(text), m.scan_all(text)
    assert every[0].size > head[0].size > 500
    same(m.scan_case(text, False), head, "head form vs scan")
    same(m.scan_case(text, True), every, "all form vs scan_all")
    # bit for bit, planes and all
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    ocap = every[0].size + 2
    ws = m.lib.acm_expand_workspace_bytes(cap - 2)
    xw, xp, xo = DeviceArray(ws), poisoned(ocap + 16), poisoned(ocap + 16)
    _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, ocap,
                                              xw.ptr, ws, None), "acm_expand_matches_async")
    got = case_planes(m, m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, ocap, True)
    assert np.array_equal(got[0], xp.to_numpy(np.int32, ocap + 16))
    assert np.array_equal(got[1], xo.to_numpy(np.int32, ocap + 16))
    for x in (d, xw, xp, xo):
        x.free()
    if nocase:   # a mixed automaton is the nocase automaton plus its case tables; this one carries none
        mm = Matcher(cm.build(FULL), 0, max_text=text.size)
        assert mm.device_bytes > m.device_bytes
        mm.close()
    m.close()


def chained(m, pieces, all_patterns, drop_before_at=None):
    """pieces scanned one after the other: each scan starts from the previous case output's trailer
    (d_init_plane), each case pass gets the previous pass's tail as d_before.  Returns the records in the
    coordinates of the concatenation and the final state.  drop_before_at: a piece given no before."""
    cap = m.plane_capacity
    ocap = 8 * cap
    L = 33
    wsb = m.lib.acm_case_workspace_bytes(cap - 2)
    ws = DeviceArray(max(wsb, 16))
    tails = [poisoned(16), poisoned(16)]
    outs = [(DeviceArray(ocap * 4), DeviceArray(ocap * 4)), (DeviceArray(ocap * 4), DeviceArray(ocap * 4))]
    offs, pats, keep = [], [], []
    before, before_len, prev, lo, last, whole = None, 0, None, 0, 0, b""
    for i, piece in enumerate(pieces):
        piece = np.frombuffer(bytes(piece), dtype=np.uint8)
        d = DeviceArray.from_numpy(piece)
        keep.append(d)
        b = m.make_batch(d, piece.size, m.stream, m.pat_plane, m.off_plane, cap, (m.ws.ptr, m.ws_bytes),
                         report=_lib.REPORT_STATE, init_plane=prev, init_plane_capacity=ocap if prev is not None else 0)
        m.enqueue(b)
        if drop_before_at == i:
            before, before_len = None, 0
        pat, off = outs[i % 2]
        tail = tails[i % 2]
        m.case_async(m.pat_plane, m.off_plane, cap - 2, d, 0, piece.size, pat, off, ocap, before=before,
                     before_len=before_len, all_patterns=all_patterns, tail_out=tail, workspace=(ws.ptr, wsb))
        n = int(pat.to_numpy(np.int32, 1)[0])
        assert n <= ocap - 2
        p, o = pat.to_numpy(np.int32, n + 2), off.to_numpy(np.int32, n + 2)
        offs.append(o[1:1 + n].astype(np.int64) + lo)
        pats.append(p[1:1 + n].copy())
        last = int(p[n + 1])
        assert int(o[n + 1]) == last
        whole = (whole if drop_before_at != i else b"") + bytes(piece)
        tl = min(L, before_len + piece.size)
        assert bytes(tail.to_numpy(np.uint8, tl)) == whole[len(whole) - tl:], "tail of piece %d" % i
        before, before_len, prev = tail, tl, pat
        lo += piece.size
    for x in keep + tails + [ws] + [y for pair in outs for y in pair]:
        x.free()
    return np.concatenate(offs).astype(np.uint32), np.concatenate(pats).astype(np.int32), last


def test_streaming(gpu):
    a = cm.build(FULL)
    m = Matcher(a, 0, max_text=4096)
    model = model_of("full")
    long33, len17 = FULL[10][0], FULL[9][0]
    text = b"..abc" + long33 + b"ABC aBc" + len17 + cm.fold(len17) + b"\xe1bc\xc1de\x80f."
    k = text.index(long33)
    for all_patterns in (False, True):
        exp = model.records(text, all_patterns)
        same(m.scan_case(text, all_patterns), exp, "one call")
        assert (k + 32) in exp[0].tolist()
        for c in range(k - 2, k + 36):      # every cut across the 33-byte match, with pieces of 1 and 0 bytes
            pieces = [text[:c], text[c:c + 1], b"", text[c + 1:]]
            same(chained(m, pieces, all_patterns), exp, "cut at %d" % c)
        same(chained(m, [b""] + [text[i:i + 1] for i in range(len(text))], all_patterns), exp, "byte by byte")
    # a piece with no before in mid-stream: exact patterns that reach back are dropped, caseless ones stay
    text = b"..cdefabc" + b"de" + b"fabc"
    cut = 9
    s = model.walk(text[:cut])[2]
    for all_patterns in (False, True):
        first = model.records(text[:cut], all_patterns)
        second = model.records(text[cut:], all_patterns, init_state=s, before=b"")
        exp = (np.concatenate([first[0], second[0] + cut]).astype(np.uint32), np.concatenate([first[1], second[1]]),
               second[2])
        got = chained(m, [text[:cut], text[cut:]], all_patterns, drop_before_at=1)
        same(got, exp, "no before")
        whole = model.records(text, all_patterns)
        assert got[0].size < whole[0].size
    pairs = set(zip(got[0].tolist(), got[1].tolist()))
    assert (cut + 1, 7) in pairs and (cut + 1, 6) not in pairs     # CDEFABCDE caseless, cdefabcde exact
    assert (cut + 1, 6) in set(zip(whole[0].tolist(), whole[1].tolist()))
    m.close()


def test_scan_case_in_mid_stream(gpu):
    """scan_case on a piece in mid-stream, init_state and before given: an exact pattern that reaches back is kept
    as far as before lets the pass compare"""
    m = Matcher(cm.build(FULL), 0, max_text=4096)
    model = model_of("full")
    text = b"..cdefabc" + b"de" + b"fabc"
    cut = 9
    s = model.walk(text[:cut])[2]
    for all_patterns in (False, True):
        sizes = []
        for before in (text[:cut], text[cut - 3:cut], b""):
            exp = model.records(text[cut:], all_patterns, init_state=s, before=before)
            same(m.scan_case(text[cut:], all_patterns, init_state=s, before=before), exp, "before %r" % before)
            sizes.append(exp[0].size)
        assert sizes[0] > sizes[2]
        whole = model.records(text, all_patterns)
        first = m.scan_case(text[:cut], all_patterns)
        second = m.scan_case(text[cut:], all_patterns, init_state=first[2], before=text[:cut])
        same((np.concatenate([first[0], second[0] + cut]), np.concatenate([first[1], second[1]]), second[2]), whole,
             "two calls")
    m.close()


def test_carry_from_an_overflowed_plane(gpu):
    """a stream in four pieces as chained() runs them, the second piece's case output in fewer cells than its
    records need: its planes are the model's for that capacity, the trailer in the last cell, and the third
    piece's scan, given those planes and that capacity as d_init_plane, goes on from it"""
    a = cm.build(FULL)
    m = Matcher(a, 0, max_text=4096)
    model = model_of("full")
    text = bytes(text_of("full", 120, 5))
    cut = [0, len(text) // 4, len(text) // 2, 3 * len(text) // 4 + 1, len(text)]
    pieces = [text[cut[i]:cut[i + 1]] for i in range(4)]
    cap = m.plane_capacity
    wsb = m.lib.acm_case_workspace_bytes(cap - 2)
    ws = DeviceArray(max(wsb, 16))
    for all_patterns in (False, True):
        exps, state = [], 0
        for i, piece in enumerate(pieces):
            exps.append(model.records(piece, all_patterns, init_state=state, before=text[max(0, cut[i] - 33):cut[i]]))
            state = exps[-1][2]
        whole = model.records(text, all_patterns)
        assert state == whole[2] and sum(e[0].size for e in exps) == whole[0].size
        count = exps[1][0].size
        assert count > 20
        for small in (2, 3, count, count + 1, count + 2):     # (the last: the last cell, and no overflow)
            caps = [8 * cap, small, 8 * cap, 8 * cap]
            outs = [(poisoned(c + 16), poisoned(c + 16)) for c in caps]
            tails = [poisoned(16) for _ in pieces]
            keep = []
            for i, piece in enumerate(pieces):
                d = DeviceArray.from_numpy(np.frombuffer(piece, dtype=np.uint8))
                keep.append(d)
                m.enqueue(m.make_batch(d, len(piece), m.stream, m.pat_plane, m.off_plane, cap, (m.ws.ptr, m.ws_bytes),
                                       report=_lib.REPORT_STATE, init_plane=outs[i - 1][0] if i else None,
                                       init_plane_capacity=caps[i - 1] if i else 0))
                m.case_async(m.pat_plane, m.off_plane, cap - 2, d, 0, len(piece), outs[i][0], outs[i][1], caps[i],
                             before=tails[i - 1] if i else None, before_len=min(33, cut[i]), all_patterns=all_patterns,
                             tail_out=tails[i], workspace=(ws.ptr, wsb))
            for i in range(4):
                eo, ep, last = exps[i]
                got = tuple(x.to_numpy(np.int32, caps[i] + 16) for x in outs[i])
                check_planes(got, ep, eo, caps[i], last, "piece %d in %d cells, all %d" % (i, caps[i], all_patterns))
            for x in keep + tails + [y for pair in outs for y in pair]:
                x.free()
    ws.free()
    m.close()


def test_segments(gpu):
    """packed texts with a cased pattern at every text's first and last bytes, each matched alone"""
    rng = np.random.default_rng(21)
    src = [p for p, _ in LONG]
    texts = []
    for i in range(300):
        head, tail = src[int(rng.integers(len(src)))], src[int(rng.integers(len(src)))]
        if i % 3 == 1:
            head, tail = cm.random_case(head, rng), cm.one_flip(tail, rng)
        mid = bytes(cm.planted_text(LONG, int(rng.integers(0, 4)), 1000 + i, filler=b" .", gap=3))
        texts.append(head + mid + tail)
    texts[7] = b""                           # an empty text
    texts[20], texts[21] = b"..ab", b"cdefa"  # a pattern that would straddle two texts
    texts[40], texts[41] = src[10][:20], src[10][20:]
    a = cm.build(LONG)
    model = model_of("long")
    m = Matcher(a, 0, max_text=sum(len(t) for t in texts))
    for all_patterns in (False, True):
        exp = model.per_text(texts, all_patterns)
        got = m.scan_case(None, all_patterns, texts=texts)
        same(got, exp, "segments %s" % all_patterns)
        joined = model.records(b"".join(texts), all_patterns)
        assert joined[0].size > exp[0].size > 600
    m.close()


def test_overflow(gpu):
    a = cm.build(FULL)
    text = text_of("full", 560, 5)
    m = Matcher(a, 0, max_text=text.size)
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    for all_patterns in (False, True):
        eo, ep, last = expected("full", 560, 5, all_patterns)
        for ocap in (2, 3, eo.size + 1, eo.size + 2):
            got = case_planes(m, m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, ocap, all_patterns)
            check_planes(got, ep, eo, ocap, last, "capacity %d" % ocap)
    # max_records below the count: only the first records are looked at, the trailer is the cell behind them
    states, offs, _ = model_of("full").walk(text)
    k = 1500
    ep, eo = model_of("full").filter(states[:k], offs[:k], text, True)
    got = case_planes(m, m.pat_plane, m.off_plane, k, d, 0, text.size, ep.size + 9, True)
    check_planes(got, ep, eo, ep.size + 9, int(states[k]), "max_records")
    d.free()
    m.close()


def test_bounds(gpu):
    """text and before allocated exactly inside guard regions, and planes with hostile cells: states out of
    range, negative offsets, offsets at and beyond text_end.  The guards hold the bytes that would complete
    a pattern begun or ended in the bytes given: a read outside them keeps an entry the rule drops."""
    a = cm.build(FULL)
    model = model_of("full")
    m = Matcher(a, 0, max_text=4096)
    exact33, exact9 = FULL[10][0], FULL[6][0]
    G = 259                                   # (odd: the text starts at an odd address)
    text = exact33[31:] + b"d." + exact33 + b"xx" + exact9 + b"d" + exact9[:5]
    before = exact33[25:] + b".." + exact33[:31]
    n, nb = len(text), len(before)
    pad = b"\x00" * G
    dt = DeviceArray.from_numpy(np.frombuffer((pad + exact33[:31])[-G:] + text + (exact9[5:] + pad)[:G], dtype=np.uint8))
    db = DeviceArray.from_numpy(np.frombuffer((pad + exact33[:25])[-G:] + before + (exact33[31:] + pad)[:G],
                                              dtype=np.uint8))
    s33, s9, sd = model.walk(exact33)[2], model.walk(exact9)[2], model.walk(b"d")[2]
    assert 10 in model.list_of(s33) and 6 in model.list_of(s9) and 7 in model.list_of(s9) and 17 in model.list_of(sd)
    origin = 1000
    cells = []
    for s in (s33, s9, sd, -1, model.num_states, 0x7FFFFFFF, -(2 ** 31), 0):
        for o in (-(2 ** 31), -5, 0, 1, origin - nb - 1, origin - nb, origin - nb + 7, origin - 1, origin, origin + 1,
                  origin + 8, origin + 36, origin + 48, origin + n - 1, origin + n, origin + n + 1, origin + n + 3,
                  origin + n + 32, origin + n + G, 2 ** 31 - 1):
            cells.append((s, o))
    states = np.array([c[0] for c in cells], dtype=np.int64)
    offs = np.array([c[1] for c in cells], dtype=np.int64)
    trailer = 77
    for count in (len(cells), 2 ** 31 - 1, -1):      # ([0] beyond max_records: max_records cells are looked at)
        sp = np.concatenate([[count], states, [trailer]]).astype(np.int64).astype(np.int32)
        so = np.concatenate([[count], offs, [trailer]]).astype(np.int64).astype(np.int32)
        dsp, dso = DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(so, pad_to=0)
        for all_patterns in (False, True):
            for bl in (nb, 0):
                ep, eo = model.filter(states, offs, text, all_patterns, origin, before if bl else b"")
                ocap = ep.size + 5
                tail = poisoned(64)
                got = case_planes(m, dsp, dso, len(cells), dt.ptr + G, origin, origin + n, ocap, all_patterns,
                                  before=db.ptr + G if bl else None, before_len=bl, tail_out=tail)
                what = "count %d all %d before %d" % (count, all_patterns, bl)
                check_planes(got, ep, eo, ocap, trailer, what)
                kept = set(zip(eo.tolist(), ep.tolist()))
                assert (origin + 36, 10) in kept and (origin + 48, 17) in kept, what
                assert ((origin + 1, 10) in kept) == (bl > 0), what            # across the seam
                assert (origin - nb + 7, 10) not in kept and (origin + n + 3, 6) not in kept, what
                if all_patterns:
                    assert (origin + n + 3, 7) in kept, what                   # caseless: nothing is read
                assert not any(o >= origin + n and not FULL[p][1] for o, p in kept), what
                tl = min(33, bl + n)
                tb = tail.to_numpy(np.uint8, 64 * 4)
                assert bytes(tb[:tl]) == ((before if bl else b"") + text)[-tl:], what
                assert (tb[tl:] == POISON_BYTE).all(), what
                tail.free()
        dsp.free()
        dso.free()
    # text_end == text_origin with no text at all: everything lies in before
    sp = np.array([1, s9, 5], dtype=np.int32)
    so = np.array([1, origin - 1, 5], dtype=np.int32)
    dsp, dso = DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(so, pad_to=0)
    bf = b"." + exact9
    dbf = DeviceArray.from_numpy(np.frombuffer(bf, dtype=np.uint8))
    got = case_planes(m, dsp, dso, 1, None, origin, origin, 8, True, before=dbf, before_len=len(bf))
    ep, eo = model.filter([s9], [origin - 1], b"", True, origin, bf)
    assert {6, 7} <= set(ep.tolist()) and len(set(eo.tolist())) == 1   # (and E, caseless, which ends there too)
    check_planes(got, ep, eo, 8, 5, "all in before")
    for x in (dt, db, dsp, dso, dbf):
        x.free()
    m.close()


def test_argument_errors(gpu):
    a = cm.build(FULL)
    m = Matcher(a, 0, max_text=4096)
    buf, out = DeviceArray(4096), poisoned(1024)
    buf.fill(0)
    ws = m.lib.acm_case_workspace_bytes(100)
    assert ws % 256 == 0 and ws > 0
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20, 1 << 22, 0x7FFFFFFE):
        b = m.lib.acm_case_workspace_bytes(r)
        assert b % 256 == 0 and b >= prev
        prev = b
    base = dict(dfa=m.dfa, sp=buf.ptr, so=buf.ptr, max_records=100, text=buf.ptr, origin=0, end=100, before=None,
                before_len=0, po=out.ptr, oo=out.ptr + 2048, cap=100, ws=buf.ptr, ws_bytes=ws)
    bad = [dict(dfa=None), dict(sp=None), dict(so=None), dict(po=None), dict(oo=None), dict(cap=1), dict(cap=0),
           dict(ws_bytes=ws - 1), dict(ws=None), dict(end=-1), dict(text=None), dict(before_len=4),
           dict(before_len=0x80000000, before=buf.ptr), dict(max_records=0x7FFFFFFF)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_case_matches_async(x["dfa"], x["sp"], x["so"], x["max_records"], x["text"], x["origin"], x["end"],
                                          x["before"], x["before_len"], 0, x["po"], x["oo"], x["cap"], None, x["ws"],
                                          x["ws_bytes"], None)
        assert rc == -1, args
    _lib.check(m.lib.acm_rt_device_sync(), "sync")
    assert (out.to_numpy(np.int32, 1024) == POISON).all()       # nothing was enqueued
    with pytest.raises(AcmError):
        m.case_async(buf, buf, 100, buf, 0, 100, out, out, 1)
    # the same call with good arguments is accepted (an empty state plane: no records)
    m.case_async(buf, buf, 100, buf, 0, 100, out.ptr, out.ptr + 2048, 100)
    assert out.to_numpy(np.int32, 2).tolist() == [0, 0]
    buf.free()
    out.free()
    m.close()
