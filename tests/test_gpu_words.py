"""Whole-word matching on the device (acm_word_matches_async, Matcher.scan_words): bit for bit the model
of tests/word_model.py (the oracle's all-patterns scan, each entry tested for word bytes around it),
one row per pipeline: sparse, chain with halo, speculative chain and the LDS walk, each also nocase."""
import numpy as np
import pytest

import word_model as wm
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib
import fixtures

pytestmark = pytest.mark.gpu

KiB = 1 << 10

# (set, scan mode, environment at upload, LDS walk expected)
ROWS = {
    "sparse": ("clamav2000", "sparse", {}, False),
    "chain-halo": ("clamav2000", "chain", {}, False),
    "chain-speculative": ("clamav2000", "chain", {"ACM_SCAN_HALO": "0"}, False),
    "lds-walk": ("sentiment", "chain", {}, True),
}
WORD_SETS = {"default": wm.DEFAULT, "empty": wm.EMPTY, "full": wm.FULL, "custom": wm.CUSTOM}


def matcher(name, max_text, nocase=False):
    a = Automaton(nocase=nocase)
    path, hx, max_len = fixtures.set_source(name)
    a.load_file(path, hx, max_len)
    a.compile()
    return Matcher(a, 0, max_text=max_text), a


def scramble(t, seed):
    t = np.array(t, dtype=np.uint8, copy=True)
    letter = ((t | 0x20) >= ord("a")) & ((t | 0x20) <= ord("z"))
    t[letter & (np.random.default_rng(seed).random(t.size) < 0.5)] ^= 0x20
    return t


def same(got, exp, what):
    assert got[0].size == exp[0].size, "%s: %d records, model %d" % (what, got[0].size, exp[0].size)
    assert np.array_equal(got[0], exp[0]), "%s: offsets differ" % what
    assert np.array_equal(got[1], exp[1]), "%s: patterns differ" % what
    assert got[2] == exp[2], "%s: final state %d != %d" % (what, got[2], exp[2])


def read_planes(pat, off, cap):
    full = int(pat.to_numpy(np.int32, 1)[0])
    cells = min(full + 2, cap)
    return full, pat.to_numpy(np.int32, cells), off.to_numpy(np.int32, cells)


def chained(m, text, L, sizes, all_patterns, mask):
    """the text scanned piece by piece: every scan starts from the previous word output's trailer
    (d_init_plane), every word pass gets the previous pass's tail as d_before and the next piece's
    first byte as next_byte.  Returns (offsets, patterns, final state)."""
    cap = m.plane_capacity
    ocap = 8 * cap if all_patterns else cap
    ws = DeviceArray(m.lib.acm_word_workspace_bytes(cap - 2))
    wsb = m.lib.acm_word_workspace_bytes(cap - 2)
    tails = [DeviceArray(4096), DeviceArray(4096)]
    outs = [(DeviceArray(ocap * 4), DeviceArray(ocap * 4)), (DeviceArray(ocap * 4), DeviceArray(ocap * 4))]
    offs, pats, before, before_len, prev, lo, last, i = [], [], None, 0, None, 0, None, 0
    keep = []
    while lo < text.size:
        hi = min(text.size, lo + sizes[i % len(sizes)])
        d = DeviceArray.from_numpy(text[lo:hi])
        keep.append(d)
        b = m.make_batch(d, hi - lo, m.stream, m.pat_plane, m.off_plane, cap, (m.ws.ptr, m.ws_bytes),
                         report=_lib.REPORT_STATE, init_plane=prev, init_plane_capacity=ocap if prev is not None else 0)
        m.enqueue(b)
        pat, off = outs[i % 2]
        tail = tails[i % 2]
        m.word_async(m.pat_plane, m.off_plane, cap - 2, d, 0, hi - lo, pat, off, ocap, before=before,
                     before_len=before_len, next_byte=int(text[hi]) if hi < text.size else -1, word_mask=mask,
                     all_patterns=all_patterns, tail_out=tail, workspace=(ws.ptr, wsb))
        n, p, o = read_planes(pat, off, ocap)
        assert n <= ocap - 2
        offs.append(o[1:1 + n].astype(np.int64) + lo)
        pats.append(p[1:1 + n].copy())
        last = int(p[n + 1])
        tl = min(L, before_len + hi - lo)
        assert bytes(tail.to_numpy(np.uint8, tl)) == bytes(text[max(0, hi - tl):hi]), "tail of the piece at %d" % lo
        before, before_len, prev = tail, tl, pat
        lo, i = hi, i + 1
    for x in keep + tails + [ws] + [a for pair in outs for a in pair]:
        x.free()
    return np.concatenate(offs).astype(np.uint32), np.concatenate(pats).astype(np.int32), last


@pytest.mark.parametrize("nocase", [False, True], ids=["case", "nocase"])
@pytest.mark.parametrize("row", list(ROWS))
def test_row(gpu, monkeypatch, row, nocase):
    name, mode, env, lds = ROWS[row]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, a = matcher(name, 512 * KiB, nocase)
    assert m.set_mode(mode) == mode
    assert m.lds_resident() == lds
    model = wm.WordModel(name, nocase)
    text = wm.planted_text(model.pats, 160 * KiB, 7, max_len=24)
    if nocase:
        text = scramble(text, 3)
    if mode == "sparse":
        m.scan(text)
        assert m.path_taken(text.size) == "sparse"

    for wname, ws in WORD_SETS.items():
        for all_patterns in (False, True):
            exp = model.words(text, ws, all_patterns)
            got = m.scan_words(text, all_patterns, word_set=ws)
            same(got, exp, "%s %s" % (wname, "all" if all_patterns else "head"))
            if wname == "default":
                assert exp[0].size > 50
                assert exp[0].size < model.words(text, wm.EMPTY, all_patterns)[0].size
    # an empty W is the plain scan and the expansion, bit for bit
    same(m.scan_words(text, False, word_set=b""), m.scan(text), "empty head vs scan")
    same(m.scan_words(text, True, word_set=b""), m.scan_all(text), "empty all vs scan_all")

    # a text chained in pieces, some shorter than the longest pattern
    L = a.max_pattern_len
    for all_patterns in (False, True):
        one = m.scan_words(text, all_patterns)
        sizes = [1, 3, max(1, L - 1), 20000, 7, L, L + 1, 50021]
        same(chained(m, text, L, sizes, all_patterns, None), one, "chained %s" % all_patterns)
        same(one, model.words(text, all_patterns=all_patterns), "one-shot")

    # a segmented batch: scan -> segment pass -> word pass
    rng = np.random.default_rng(13)
    starts = np.sort(rng.choice(text.size, 600, replace=False)).astype(np.int32)
    starts[0] = 0
    starts = np.concatenate([starts[:300], starts[300:301], starts[300:]])   # one empty segment
    for all_patterns in (False, True):
        same(m.scan_words(text, all_patterns, segments=starts),
             model.words(text, all_patterns=all_patterns, starts=starts), "segments %s" % all_patterns)

    # a shard: its halo is part of d_text (text_origin = offset_shift), one byte in front as d_before
    halo = L - 1
    load_begin = 64 * KiB + 5
    begin, end = load_begin + halo, 130001
    d = DeviceArray.from_numpy(text)
    dt = DeviceArray.from_numpy(text[load_begin:end])
    db = DeviceArray.from_numpy(text[load_begin - 1:load_begin])
    cap = m.plane_capacity
    m.scan_async(dt, end - load_begin, halo=halo, offset_shift=load_begin, report=_lib.REPORT_STATE)
    pat, off = DeviceArray(cap * 4), DeviceArray(cap * 4)
    m.word_async(m.pat_plane, m.off_plane, cap - 2, dt, load_begin, end, pat, off, cap, before=db, before_len=1,
                 next_byte=int(text[end]))
    n, p, o = read_planes(pat, off, cap)
    exp = model.words(text)
    sel = (exp[0] >= begin) & (exp[0] < end)
    assert n == int(sel.sum()) > 0
    assert np.array_equal(o[1:1 + n].astype(np.uint32), exp[0][sel])
    assert np.array_equal(p[1:1 + n], exp[1][sel])

    # an output too small for the records: the full count in [0], the trailer in the last cell
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    small = 10
    ps, os_ = DeviceArray(small * 4), DeviceArray(small * 4)
    m.word_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, ps, os_, small)
    n, p, o = read_planes(ps, os_, small)
    assert n == exp[0].size > small
    assert np.array_equal(o[1:small - 1].astype(np.uint32), exp[0][:small - 2])
    assert np.array_equal(p[1:small - 1], exp[1][:small - 2])
    assert int(p[small - 1]) == exp[2] and int(o[small - 1]) == exp[2]
    for x in (d, dt, db, pat, off, ps, os_):
        x.free()
    m.close()


def test_planted_boundaries(gpu):
    """a pattern next to every kind of byte, at the text start and at the text end"""
    a = Automaton()
    for p in (b"cat", b"at", b"-x", b"\xe9t\xe9"):
        a.add(p)
    a.compile()
    m = Matcher(a, 0, max_text=4096)
    text = b"cat cats bobcat cat_ cat1 (cat) at,at.\xe9cat\xe9 a-x -x x-x \xe9t\xe9 a\xe9t\xe9 cat"
    got = m.scan_words(text, True)
    exp = wm.brute_force([b"cat", b"at", b"-x", b"\xe9t\xe9"], np.frombuffer(text, np.uint8))
    assert list(zip(got[0].tolist(), got[1].tolist())) == sorted(exp)
    pairs = set(zip(got[0].tolist(), got[1].tolist()))
    assert (2, 0) in pairs and (len(text) - 1, 0) in pairs       # at the start and at the end
    for word in (b"bobcat", b"cats", b"cat_", b"cat1", b"a-x", b"x-x"):
        end = text.index(word) + len(word) - (2 if word in (b"cats", b"cat_", b"cat1") else 1)
        assert not any(o == end for o, _ in pairs), word            # inside a word, or '-' after a letter
    for word in (b"(cat)", b".\xe9cat\xe9", b" -x ", b"at,", b" \xe9t\xe9 "):
        k = text.index(word)
        assert any(k < o < k + len(word) for o, _ in pairs), word   # next to punctuation or bytes >= 0x80
    m.close()


def test_bytes_around_the_text(gpu):
    """scan_words with before and next_byte: the text is a piece of a longer one, found whole by brute force"""
    pats = [b"cat", b"at", b"-x", b"\xe9t\xe9"]
    a = Automaton()
    for p in pats:
        a.add(p)
    a.compile()
    m = Matcher(a, 0, max_text=4096)
    text = b"cat bobcat at -x (cat) cat"
    seen = set()
    for before in (b"", b"bob", b"a ", b"x-", b"_"):
        for nxt in (-1, ord("s"), ord("."), 0xe9):
            whole = before + text + (bytes([nxt]) if nxt >= 0 else b"")
            k = len(before)
            exp = sorted((o - k, p) for o, p in wm.brute_force(pats, np.frombuffer(whole, np.uint8))
                         if o - len(pats[p]) + 1 >= k and o < k + len(text))      # the piece's own entries
            for all_patterns in (True, False):
                got = m.scan_words(text, all_patterns, before=before, next_byte=nxt)
                if not all_patterns:                   # the first in list order of every offset
                    exp = [e for i, e in enumerate(exp) if i == 0 or exp[i - 1][0] != e[0]]
                assert list(zip(got[0].tolist(), got[1].tolist())) == exp, (before, nxt, all_patterns)
            seen.add(((2, 0) in exp, (len(text) - 1, 0) in exp))
    assert len(seen) == 4                              # the first and the last "cat" come and go on their own
    m.close()


def test_argument_errors(gpu):
    a = Automaton()
    a.add(b"abc")
    a.compile()
    m = Matcher(a, 0, max_text=4096)
    buf = DeviceArray(4096)
    ws = m.lib.acm_word_workspace_bytes(100)
    base = dict(max_records=100, text=buf.ptr, origin=0, end=100, before=None, before_len=0, next_byte=-1,
                seg=None, segments=0, cap=100, ws=buf.ptr, ws_bytes=ws)
    bad = [dict(cap=1), dict(segments=3), dict(ws_bytes=ws - 1), dict(ws=None), dict(end=-1),
           dict(text=None), dict(before_len=4), dict(next_byte=256), dict(next_byte=-2),
           dict(max_records=0x7FFFFFFF)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = m.lib.acm_word_matches_async(m.dfa, buf.ptr, buf.ptr, x["max_records"], x["text"], x["origin"],
                                          x["end"], x["before"], x["before_len"], x["next_byte"], x["seg"],
                                          x["segments"], None, 0, buf.ptr, buf.ptr, x["cap"], None, x["ws"],
                                          x["ws_bytes"], None)
        assert rc == -1, args
    with pytest.raises(AcmError):
        m.word_async(buf, buf, 100, buf, 0, 100, buf, buf, 100, segments=2)
    with pytest.raises(ValueError):
        m.word_async(buf, buf, 100, buf, 0, 100, buf, buf, 100, word_mask=b"x")
    buf.free()
    m.close()
