"""Match rewriting on the device (acm_rewrite_async, Matcher.scan_rewrite), byte for byte against the model of
tests/rewrite_model.py: text lengths around every power-of-two tile, every source shift and replacement length
against the tile cuts, spans at the ends of the text, chains of adjacent spans, total deletion, dense growth, fills,
contexts, text_origin, capacities, planes that did not come from select, argument errors, and Matcher.scan_rewrite
against re.sub.  The output, d_at_out, d_seg_out and d_info lie between guard bands and are poisoned before every
call, the text is followed by poison, and the workspace is exactly of the queried size and poisoned."""
import ctypes as C

import numpy as np
import pytest

import ops_guard as og
import rewrite_model as rw
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib
from gpu_pattern_matching_amd._lib import check

pytestmark = pytest.mark.gpu

NO_CELL = 0x7FFFFF00
INT32_MAX = 0x7FFFFFFF
PAST = 4096                                  # poisoned bytes behind round16(n) of every text


def random_text(n, seed=0, alphabet=None):
    rng = np.random.default_rng(seed)
    if alphabet is None:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)]


class Set:
    """a pattern set with replacements, uploaded: pats are bytes; repl per pattern None, bytes or ("fill", byte)"""

    def __init__(self, pats, repl, nocase=False, automaton=None):
        a = automaton
        if a is None:
            a = Automaton(nocase=nocase)
            for i, p in enumerate(pats):
                a.add(p, i)
        self.repl = []
        for i, r in enumerate(repl):
            if r is None:
                self.repl.append(None)
            elif isinstance(r, tuple):
                a.set_replacement(i, fill=r[1])
                self.repl.append((bytes([r[1]]), True))
            else:
                a.set_replacement(i, r)
                self.repl.append((bytes(r), False))
        a.compile()
        self.a = a
        self.lens = [len(a.pattern(i)[0]) for i in range(a.num_patterns)]
        ctx = [a.wildcard_lengths(i) for i in range(a.num_patterns)]
        self.model = rw.RewriteModel(self.lens, self.repl, [c[0] for c in ctx], [c[1] for c in ctx])
        self.m = Matcher(a, 0, max_text=4096)

    def close(self):
        self.m.close()


def upload_planes(cells, offs, count=None, tail=()):
    m = len(cells) if count is None else count
    sp = np.concatenate([[m], cells, tail]).astype(np.int64).astype(np.int32)
    so = np.concatenate([[m], offs, tail]).astype(np.int64).astype(np.int32)
    return DeviceArray.from_numpy(sp, pad_to=0), DeviceArray.from_numpy(so, pad_to=0)


def upload_text(text):
    t = np.asarray(text, dtype=np.uint8)
    h = np.full(((t.size + 15) & ~15) + PAST, 0xC3, dtype=np.uint8)
    h[:t.size] = t
    return DeviceArray.from_numpy(h)


class Call:
    """one call from poisoned outputs; the downloads check the guard bands"""

    def __init__(self, matcher, d_text, n, planes, max_records, cap, origin=0, at_cap=None, seg_start=None, with_out=True,
                 ws_fill=0xFF, stream=None):
        self.cap = cap
        self.out = og.Guarded(cap if with_out else 16, dtype=np.uint8)
        self.at = og.Guarded(at_cap) if at_cap is not None else None
        nseg = 0 if seg_start is None else len(seg_start)
        self.seg_in = og.Guarded(max(nseg, 1), host=np.asarray(seg_start, dtype=np.int32)) if nseg else None
        self.seg = og.Guarded(nseg) if nseg else None
        self.info = og.Guarded(8)
        nb = matcher.lib.acm_rewrite_workspace_bytes(max_records, nseg)
        self.ws = og.Workspace(nb, ws_fill)
        matcher.rewrite_async(d_text, n, planes[0], planes[1], max_records, self.out.ptr if with_out else None,
                              cap if with_out else 0, self.info.ptr, text_origin=origin,
                              at_out=self.at.ptr if self.at else None, at_capacity=at_cap or 0,
                              seg_start=self.seg_in.ptr if nseg else None, segments=nseg,
                              seg_out=self.seg.ptr if nseg else None, workspace=(self.ws.ptr, nb), stream=stream)
        self.stream = stream
        self.with_out = with_out

    def read(self, what=""):
        st = self.stream
        self.ws.check(st, what)
        res = dict(out=self.out.read(st, what), info=self.info.read(st, what),
                   at=self.at.read(st, what) if self.at else None, seg=self.seg.read(st, what) if self.seg else None)
        for x in (self.out, self.at, self.seg_in, self.seg, self.info, self.ws):
            if x is not None:
                x.free()
        return res


def run(s, text, cells, offs, origin=0, cap=None, seg_start=None, max_records=None, at_cap=None, with_out=True,
        count=None, tail=(), what="", d_text=None, planes=None):
    """one call compared whole with the model; returns (model output, info)"""
    text = np.asarray(text, dtype=np.uint8)
    cells, offs = np.asarray(cells, dtype=np.int64), np.asarray(offs, dtype=np.int64)
    mr = len(cells) if max_records is None else max_records
    behind = np.asarray(tail, dtype=np.int64)                 # (the cells behind the records stand in both planes)
    seen = min((len(cells) if count is None else count) & 0xFFFFFFFF, mr)   # the count cell is read as unsigned
    assert seen <= len(cells) + behind.size
    seg = None if seg_start is None else list(seg_start)
    xo, xinfo, xat, xseg = s.model.run(text.tobytes(), np.r_[cells, behind][:seen], np.r_[offs, behind][:seen], origin, seg,
                                       None, with_out)
    m = len(xo)
    cap = m + 37 if cap is None else cap
    xinfo[6] = int(with_out and m > cap)
    at_cap = len(xat) + 5 if at_cap is None else at_cap
    dt = d_text if d_text is not None else upload_text(text)
    pl = planes if planes is not None else upload_planes(cells, offs, count, tail)
    got = Call(s.m, dt, text.size, pl, mr, cap, origin, at_cap, seg, with_out).read(what)
    what = "%s n=%d records=%d max_records=%d cap=%d origin=%d" % (what, text.size, len(cells), mr, cap, origin)
    assert got["info"].tolist() == xinfo, "%s: info %s, model %s" % (what, got["info"].tolist(), xinfo)
    if with_out:
        k = min(m, cap)
        exp = np.frombuffer(xo[:k], dtype=np.uint8)
        bad = np.flatnonzero(got["out"][:k] != exp)
        assert bad.size == 0, "%s: output byte %d = %d, model %d (%d differ)" % (
            what, bad[0], got["out"][bad[0]], exp[bad[0]], bad.size)
        assert (got["out"][k:] == og.FILL).all(), "%s: a byte at or behind min(m, capacity) = %d was written" % (what, k)
    else:
        assert (got["out"] == og.FILL).all()
    u = len(xat)
    stored = min(u, at_cap - 2)
    xa = np.full(at_cap, og.FILL32, dtype=np.int64)
    xa[0] = u
    xa[1:1 + stored] = xat[:stored]
    xa[min(u + 1, at_cap - 1)] = 0
    og.same(got["at"], xa, what + ": at plane")
    if seg is not None:
        og.same(got["seg"], xseg, what + ": seg_out")
    if d_text is None:
        dt.free()
    if planes is None:
        for x in pl:
            x.free()
    return xo, xinfo


# ------------------------------------------------------------------ the sets

LENS18 = [bytes([0x61 + i % 26]) * (i + 1) for i in range(35)]       # patterns of 1 .. 35 bytes
REPL_LENGTHS = [0, 1, 15, 16, 17, 4096, 65535]


def blob(n, seed):
    return bytes(random_text(n, 1000 + seed, b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"))


@pytest.fixture(scope="module")
def shift_set(gpu):
    """pattern i has i + 1 bytes and becomes 18 bytes: a delta of 17 - i, that is +17 .. -17"""
    s = Set(LENS18, [blob(18, i) for i in range(35)])
    yield s
    s.close()


@pytest.fixture(scope="module")
def length_set(gpu):
    """seven one-byte patterns, pattern i becomes REPL_LENGTHS[i] bytes; then a 64-byte pattern without replacement,
    a one-byte pattern that is deleted, a one-byte pattern filled, an empty pattern, a 64-byte pattern deleted and a
    one-byte pattern that becomes 255 bytes"""
    pats = [bytes([0x61 + i]) for i in range(7)] + [b"h" * 64, b"i", b"j", b"", b"k" * 64, b"l"]
    s = Set(pats, [blob(k, k) for k in REPL_LENGTHS] + [None, b"", ("fill", 0x2A), b"never", b"", blob(255, 7)])
    yield s
    s.close()


KEEP64, DEL1, FILL1, EMPTY, DEL64, GROW255 = 7, 8, 9, 10, 11, 12


# ------------------------------------------------------------------ 1. text lengths, no records


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, 65535, 65536, 65537, 2 ** 20 + 1025])
def test_text_lengths_without_records(length_set, n):
    text = random_text(n, n)
    for cap in sorted({n, n + 100, max(n - 1, 0)}):
        xo, info = run(length_set, text, [], [], cap=cap, seg_start=[0, n // 2, n], what="lengths")
        assert xo == text.tobytes() and info[:4] == [0, 0, n, 0]


def test_unchanged_set_without_replacements(gpu):
    """a set without replacements: the output is the text whatever is selected, and the upload is what it was"""
    pats = [b"ab", b"abc", b"q"]
    plain = Set(pats, [None, None, None])
    cleared = Set(pats, [b"x", None, ("fill", 1)])
    assert cleared.m.device_bytes > plain.m.device_bytes
    a = Automaton()
    for i, p in enumerate(pats):
        a.add(p, i)
    a.set_replacement(0, b"x")
    a.clear_replacement(0)
    again = Set(pats, [None] * 3, automaton=a)
    assert again.m.device_bytes == plain.m.device_bytes and not a.has_replacements
    text = random_text(70000, 5, b"abcq")
    cells, offs = rw.selected(pats, [text.tobytes()])
    assert cells.size > 10000
    xo, info = run(plain, text, cells, offs, seg_start=[0, 35000])
    assert xo == text.tobytes() and info[0] == cells.size
    for s in (plain, cleared, again):
        s.close()
    # a fixture set: replacements set and cleared again leave the upload what it is without them
    import fixtures
    path, hx, max_len = fixtures.set_source("tests")
    sizes = []
    for touch in (False, True):
        a = Automaton()
        n = a.load_file(path, hx, max_len)
        if touch:
            for i in range(n):
                a.set_replacement(i, b"x" * (i % 7))
            for i in range(n):
                a.clear_replacement(i)
        a.compile()
        m = Matcher(a, 0, max_text=4096)
        sizes.append(m.device_bytes)
        m.close()
    assert sizes[0] == sizes[1] > 0


# ------------------------------------------------------------------ 2. source shift


@pytest.mark.parametrize("delta", range(-17, 18))
def test_source_shift(shift_set, delta):
    """one record early in the text, then 128 KiB and more of gap read at the shift the delta gives"""
    p = 17 - delta                                           # the pattern of p + 1 bytes
    n = 128 * 1024 + 3000 + delta
    text = random_text(n, 77 + delta)
    xo, info = run(shift_set, text, [p], [40 + p], seg_start=[0, 41, 50000], what="shift")
    assert info[0] == 1 and len(xo) == n + delta


# ------------------------------------------------------------------ 3. replacement lengths against tile cuts


@pytest.mark.parametrize("k", range(len(REPL_LENGTHS)), ids=[str(x) for x in REPL_LENGTHS])
def test_replacement_lengths_across_cuts(length_set, k):
    """the one record of the call begins at output offsets j * 4096 - 18 .. j * 4096 + 1 for j = 1 .. 16, whole tiles of
    gap on both sides: every multiple of a power-of-two tile up to 64 KiB is a cut that the replacement crosses, ends
    on or begins on at every alignment, whatever the tile size is.  Among them: the deletion that sits exactly on a
    cut (length 0, offset j * 4096), and replacements of 1 and 17 bytes that begin on a cut's last byte in front and
    on its first byte behind."""
    n = 17 * 4096 + 11
    text = random_text(n, 300 + k)
    dt = upload_text(text)
    for j in range(1, 17):
        for at in range(j * 4096 - 18, j * 4096 + 2):
            xo, info = run(length_set, text, [k], [at], d_text=dt, what="cuts")
            assert len(xo) == n - 1 + REPL_LENGTHS[k] and info[0] == 1
    # two of them around a cut: the second one begins where the first one's growth has pushed it
    for cut in (8192, 16384, 32768, 65536):
        run(length_set, text, [k, k], [cut - 2, cut + 8], d_text=dt, seg_start=[cut - 1, cut + 8, cut + 9], what="cuts")
    dt.free()


@pytest.mark.parametrize("cut", [4096, 8192, 16384, 32768, 65536])
def test_records_on_a_cut(length_set, cut):
    """records whose place in the OUTPUT is a cut, behind a record that has moved everything: a deletion whose empty
    replacement lies exactly on the cut, alone and in a run of 300, with a tile of gap behind it; replacements of 1 and
    17 bytes and a fill that begin on the byte in front of the cut and on the cut; a kept span that straddles it"""
    n = cut + 70000
    text = random_text(n, cut)
    dt = upload_text(text)
    grow = 255 - 1                                                  # GROW255 at offset 100 moves what follows by 254
    for kind, length in ((DEL1, 1), (1, 1), (4, 1), (FILL1, 1), (KEEP64, 64), (DEL64, 64)):
        for out_at in (cut - 1, cut, cut - 16, cut + 15):
            s = out_at - grow                                       # the span begins here in the text
            xo, info = run(length_set, text, [GROW255, kind], [100, s + length - 1], d_text=dt,
                           seg_start=[s, s + length, cut], what="on a cut")
            assert info[0] == 2
    s = cut - grow
    run(length_set, text, [GROW255] + [DEL1] * 300, [100] + list(range(s, s + 300)), d_text=dt, seg_start=[s, s + 300],
        what="deletions on a cut")
    dt.free()


# ------------------------------------------------------------------ 4. span positions


def test_spans_at_the_ends(length_set):
    text = random_text(5000, 9)
    for k in (0, 1, 3, 5, KEEP64, DEL1, FILL1, GROW255):
        L = length_set.lens[k]
        run(length_set, text, [k], [L - 1], what="first byte")
        run(length_set, text, [k], [4999], what="last byte")
        run(length_set, text, [k, k], [L - 1, 4999], what="both")
    for k in (KEEP64, DEL64):                                # the whole text is one span
        xo, info = run(length_set, text[:64], [k], [63], seg_start=[0, 1, 64], what="whole")
        assert len(xo) == (64 if k == KEEP64 else 0)
    for k in (0, 5, DEL1, FILL1):
        run(length_set, text[:1], [k], [0], seg_start=[0, 1], what="one byte")


@pytest.mark.parametrize("chain", [1, 2, 1025, 70000])
def test_adjacent_spans(length_set, chain):
    """e + 1 == s' all along: one-byte spans that grow, shrink, fill and vanish, no gap between them"""
    kinds = np.array([2, DEL1, 1, FILL1, 4, DEL1, DEL1, 0], dtype=np.int64)
    n = chain + 5000
    text = random_text(n, chain)
    cells = kinds[np.arange(chain) % kinds.size]
    offs = 1000 + np.arange(chain, dtype=np.int64)
    xo, info = run(length_set, text, cells, offs, seg_start=[999, 1000, 1001, 1000 + chain // 2, 1000 + chain], what="chain")
    assert info[0] == chain and info[4] == chain


# ------------------------------------------------------------------ 5. total deletion


def test_total_deletion(gpu):
    n = 2 ** 20
    s = Set([b"a", b"b"], [b"", None])
    text = np.full(n, 0x61, dtype=np.uint8)
    cells, offs = np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    xo, info = run(s, text, cells, offs, cap=4096, seg_start=[0, 5, n], what="deleted")
    assert xo == b"" and info == [n, 0, 0, 0, n, 0, 0, 0]
    # every 4097th byte stays: 4096 records of no bytes between two output bytes
    keep = np.arange(4096, n, 4097)
    text[keep] = 0x62
    sel = np.ones(n, dtype=bool)
    sel[keep] = False
    xo, info = run(s, text, cells[sel], offs[sel], seg_start=[0, 4096, 4097, 4098, n], what="sparse survivors")
    assert xo == b"b" * keep.size and keep.size == 255
    s.close()


# ------------------------------------------------------------------ 6. dense, alternating growth


@pytest.mark.parametrize("deletions", [1, 70])
def test_dense_alternating_growth(length_set, deletions):
    """a one-byte span that becomes 255 bytes, then `deletions` adjacent 64-byte spans that vanish, over and over: with
    70 of them 16 * 71 = 1136 records feed every 4 KiB of output"""
    groups = 300 if deletions == 1 else 40
    unit = 1 + 64 * deletions + (3 if deletions == 1 else 0)       # (a gap of three bytes in the 1:1 form)
    n = 100 + groups * unit + 50
    text = random_text(n, 600 + deletions)
    cells, offs = [], []
    for g in range(groups):
        base = 100 + g * unit
        cells.append(GROW255)
        offs.append(base)
        for d in range(deletions):
            cells.append(DEL64)
            offs.append(base + 64 * (d + 1))
    xo, info = run(length_set, text, cells, offs, seg_start=[0, 100, 100 + 7 * unit, n], what="dense")
    assert info[0] == groups * (1 + deletions) and len(xo) == n + groups * (254 - 64 * deletions)
    if deletions == 70:
        assert 16 * (1 + deletions) > 1000


# ------------------------------------------------------------------ 7. fill, mixed kinds, contexts


def test_fill_keeps_the_length(gpu):
    pats = [b"secret", b"key", b"x"]
    s = Set(pats, [("fill", 0x2A), ("fill", 0x00), ("fill", 0xFF)])
    rng = np.random.default_rng(12)
    tokens = [b"secret", b"key", b"x", b" ", b"se", b"ke", b"t", b"cr"]
    text = np.frombuffer(b"".join(tokens[i] for i in rng.integers(0, len(tokens), 16000)), dtype=np.uint8)
    cells, offs = rw.selected(pats, [text.tobytes()])
    xo, info = run(s, text, cells, offs, what="fill")
    out = np.frombuffer(xo, dtype=np.uint8)
    assert out.size == text.size and cells.size > 3000 and set(cells.tolist()) == {0, 1, 2}
    inside = np.zeros(text.size, dtype=bool)
    for c, o in zip(cells.tolist(), offs.tolist()):
        inside[o - len(pats[c]) + 1:o + 1] = True
    assert np.array_equal(out[~inside], text[~inside]) and not np.isin(out[inside], text[~inside]).any()
    assert xo == rw.re_sub(pats, s.repl, text.tobytes())
    s.close()


def test_mixed_kinds(gpu):
    pats = [b"cat", b"dog", b"bird", b"o"]
    s = Set(pats, [b"feline", None, b"", ("fill", 0x5F)])
    text = b"a cat, a dog and a bird; dogcatbirddog o catdog"
    cells, offs = rw.selected(pats, [text])
    xo, info = run(s, np.frombuffer(text, dtype=np.uint8), cells, offs, seg_start=[0, 9, 10, 24])
    assert xo == b"a feline, a dog and a ; dogfelinedog _ felinedog" and info[0] == 10
    s.close()


def test_contexts_belong_to_the_span(gpu):
    ANY = range(256)
    a = Automaton()
    a.add_wildcard([ANY, b"k", b"e", b"y", ANY, ANY], 0)         # 0: pre 1, anchor 3, post 2
    a.add(b"zz", 1)
    a.add_wildcard([b"i", b"d", b"=", ANY, ANY, ANY, ANY], 2)    # 2: anchor 3, post 4
    a.add_wildcard([ANY, ANY, b"q"], 3)                          # 3: pre 2
    s = Set(None, [b"<K>", b"Z", ("fill", 0x23), b""], automaton=a)
    assert s.lens == [3, 2, 3, 1]
    #       0123456789012345678901234567890123
    text = b"..-key12..zz..id=abcd..xyq..id=12"
    #   0 @5: [2, 7]; 1 @11: [10, 11]; 2 @16: [14, 20]; 3 @25: [23, 25]; 2 @30: the post context leaves the text
    xo, info = run(s, np.frombuffer(text, dtype=np.uint8), [0, 1, 2, 3, 2], [5, 11, 16, 25, 30], seg_start=[3, 8, 21])
    assert xo == b"..<K>..Z..#######....id=12" and info[:2] == [4, 1]
    s.close()


# ------------------------------------------------------------------ 8. text_origin and records that are skipped


@pytest.mark.parametrize("origin", [-1000, 0, 12345, -(2 ** 31) + 100, 2 ** 31 - 70000])
def test_text_origin_and_skipped_records(length_set, origin):
    n = 20000
    text = random_text(n, 3)
    good_c = [0, 5, DEL1, KEEP64, FILL1, 3, 1]
    good_o = [10, 500, 501, 700, 9000, 16384, n - 1]
    # records in front of the text, behind it, across its ends, no pattern, a pattern of no bytes: all in their place
    cells = [KEEP64, 0, NO_CELL] + good_c[:3] + [-1, EMPTY, 99] + good_c[3:] + [DEL64, 0, 1, KEEP64]
    offs = [20, -1, 5] + good_o[:3] + [600, 600, 601] + good_o[3:] + [n + 10, n, n + 5, n]
    offs = [o + origin for o in offs]
    xo, info = run(length_set, text, cells, offs, origin=origin, seg_start=[origin - 5, origin, origin + 501, origin + n],
                   what="origin")
    assert info[0] == len(good_c) and info[1] == len(cells) - len(good_c)
    only, _ = run(length_set, text, good_c, [o + origin for o in good_o], origin=origin, what="origin")
    assert xo == only


# ------------------------------------------------------------------ 9. capacities


def test_capacities(length_set):
    n = 30000
    text = random_text(n, 8)
    cells, offs = [3, 5, DEL1, 1], [100, 9000, 20000, 29000]        # 16 bytes; 4096 bytes; deleted; 1 byte
    m = n + 15 + 4095 - 1                                           # the second replacement begins at 9015
    dt = upload_text(text)
    pl = upload_planes(cells, offs)
    for cap in (m, m - 1, m + 1, 5000, 9015 + 100, 9015 + 4096, 16, 15, 1, 100 + 5):
        xo, info = run(length_set, text, cells, offs, cap=cap, d_text=dt, planes=pl, what="capacity")
        assert len(xo) == m and info[6] == int(cap < m)
    xo, info = run(length_set, text, cells, offs, cap=0, with_out=False, d_text=dt, planes=pl, seg_start=[0, 101, n])
    assert info[2] == m and info[6] == 0
    for at_cap in (2, 3, 4, 5, 6):                                  # the at plane: the scan's overflow contract
        run(length_set, text, cells, offs, at_cap=at_cap, d_text=dt, planes=pl, what="at capacity")
    # no at plane: nothing else changes
    got = Call(length_set.m, dt, n, pl, 4, m, at_cap=None).read()
    assert bytes(got["out"]) == xo and got["info"].tolist()[:4] == [4, 0, m, 0]
    dt.free()
    for x in pl:
        x.free()


# ------------------------------------------------------------------ 10. planes that did not come from select


def test_hostile_planes(length_set):
    """overlapping and descending spans, random cells, offsets at the ends of int32: guard bands intact (Call.read),
    every record looked at is counted once, and two runs give the same bytes"""
    rng = np.random.default_rng(17)
    n = 50000
    text = random_text(n, 4)
    dt = upload_text(text)
    m = 3000
    pool = np.array(list(range(13)) + [-1, NO_CELL, 13, INT32_MAX, -(2 ** 31)], dtype=np.int64)
    edge = np.array([-(2 ** 31), -1, 0, 1, n - 1, n, n + 63, INT32_MAX], dtype=np.int64)
    for kind in ("overlap", "descend", "random", "same"):
        cells = pool[rng.integers(0, pool.size, m)]
        offs = np.sort(rng.integers(0, n, m))
        if kind == "descend":
            offs = offs[::-1].copy()
        elif kind == "random":
            offs = np.where(rng.random(m) < 0.2, edge[rng.integers(0, edge.size, m)], rng.permutation(offs))
        elif kind == "same":
            offs[:] = 25000
        pl = upload_planes(cells, offs)
        for cap in (n, 200000, 1000):
            runs = [Call(length_set.m, dt, n, pl, m, cap, 0, 100, [0, 100, n], ws_fill=f).read(kind) for f in (0xFF, 0x00)]
            for key in ("out", "info", "at", "seg"):
                assert np.array_equal(runs[0][key], runs[1][key]), (kind, key)
            info = runs[0]["info"]
            assert int(info[0]) + int(info[1]) == m and info[7] == 0 and info[6] in (0, 1)
            _, _, used = length_set.model.used(cells, offs, n)
            assert int(info[0]) == int(used.sum())
        for x in pl:
            x.free()
    dt.free()


# ------------------------------------------------------------------ 11. records beyond the count


def test_records_beyond_the_count(length_set):
    n = 9000
    text = random_text(n, 6)
    cells = [0, 1, 2, 3, 4, DEL1, FILL1, 5]
    offs = [10, 20, 30, 40, 50, 60, 70, 80]
    for mr in (0, 1, 4, 7, 8, 9, 5000):
        run(length_set, text, cells, offs, max_records=mr, what="max_records")
    # a count cell below the records in the planes, and a poisoned tail: nothing behind [0] is a record
    tail = [GROW255] * 40
    for count in (0, 3, 8):
        run(length_set, text, cells, offs, max_records=48, count=count, tail=tail, what="count")
    # a count cell that is no count
    for count in (-1, INT32_MAX):
        xo, info = run(length_set, text, cells, offs, max_records=8, count=count, tail=tail, what="count")
        assert info[0] == 8


# ------------------------------------------------------------------ 12. stability, streams


def test_stability_and_streams(length_set):
    n = 300000
    text = random_text(n, 2, b"abcdefg ")
    pats = [bytes([0x61 + i]) for i in range(7)]
    cells, offs = rw.selected(pats, [text.tobytes()])
    keep = (np.arange(cells.size) % 29 == 0) & (cells != 6)         # (7 in 8 bytes match: keep one in 29 of them)
    cells, offs = cells[keep], offs[keep]
    xo, info = run(length_set, text, cells, offs, what="stable")
    dt = upload_text(text)
    pl = upload_planes(cells, offs)
    s = C.c_void_p()
    check(length_set.m.lib.acm_rt_stream_create(C.byref(s)), "acm_rt_stream_create")
    runs = [Call(length_set.m, dt, n, pl, cells.size, len(xo), at_cap=cells.size + 2, seg_start=[0, 1000, n], ws_fill=f,
                 stream=st).read("streams") for f, st in ((0xFF, None), (0xA5, None), (0x00, s.value), (0xFF, s.value))]
    for r in runs:
        assert bytes(r["out"]) == xo and r["info"].tolist() == info
        assert np.array_equal(r["at"], runs[0]["at"]) and np.array_equal(r["seg"], runs[0]["seg"])
    length_set.m.lib.acm_rt_stream_destroy(s.value)
    dt.free()
    for x in pl:
        x.free()


# ------------------------------------------------------------------ 13. argument errors


def test_argument_errors(length_set):
    m = length_set.m
    lib = m.lib
    prev = 0
    for r in (0, 1, 1023, 1024, 1025, 100000, 1 << 20, 1 << 22, 0x7FFFFFFE):
        for segs in (0, 1, 1 << 20):
            b = lib.acm_rewrite_workspace_bytes(r, segs)
            assert b % 256 == 0 and b > 0 and b >= prev and b >= lib.acm_rewrite_workspace_bytes(r, 0)
        prev = lib.acm_rewrite_workspace_bytes(r, 0)
    buf = og.Guarded(1 << 14)                                      # text, planes, starts: zeros
    check(lib.acm_rt_memset(buf.ptr, 0, 1 << 16, None), "acm_rt_memset")
    out = og.Guarded(4096)
    ws = lib.acm_rewrite_workspace_bytes(100, 4)
    w = DeviceArray(ws)
    big = 2 ** 31 - 16
    base = dict(dfa=m.dfa, text=buf.ptr, n=1000, origin=0, sp=buf.ptr + 4096, so=buf.ptr + 4096, mr=100, out=out.ptr, cap=1000,
                at=out.ptr + 4096, at_cap=100, st=buf.ptr + 8192, segs=4, sg=out.ptr + 8192, info=out.ptr + 12288, ws=w.ptr,
                ws_bytes=ws)
    bad = [dict(dfa=None), dict(text=None), dict(sp=None), dict(so=None), dict(info=None), dict(text=buf.ptr + 8),
           dict(out=out.ptr + 4), dict(n=big), dict(cap=big), dict(out=None), dict(at_cap=1), dict(at_cap=0), dict(st=None),
           dict(sg=None), dict(segs=0), dict(ws_bytes=ws - 1), dict(ws=None), dict(mr=0x7FFFFFFF), dict(origin=2 ** 31),
           dict(origin=-(2 ** 31) - 1)]
    for args in bad:
        x = dict(base)
        x.update(args)
        rc = lib.acm_rewrite_async(x["dfa"], x["text"], x["n"], x["origin"], x["sp"], x["so"], x["mr"], x["out"], x["cap"],
                                   x["at"], x["at_cap"], x["st"], x["segs"], x["sg"], x["info"], x["ws"], x["ws_bytes"], None)
        assert rc == -1, args
        assert lib.acm_last_error()
    check(lib.acm_rt_device_sync(), "sync")
    out.untouched(what="argument errors")                           # nothing was enqueued
    with pytest.raises(AcmError):
        m.rewrite_async(buf.ptr, 1000, buf.ptr, buf.ptr, 100, None, 16, out.ptr)
    # the same call with good arguments is accepted; so are a NULL text of no bytes and a NULL output of no room
    x = base
    for text, n, o, cap in ((x["text"], 1000, x["out"], 1000), (None, 0, x["out"], 1000), (x["text"], 1000, None, 0)):
        assert lib.acm_rewrite_async(x["dfa"], text, n, 0, x["sp"], x["so"], 100, o, cap, x["at"], 100, x["st"], 4, x["sg"],
                                     x["info"], x["ws"], ws, None) == 0
        got = out.read()
        assert got[12288 // 4:12288 // 4 + 8].tolist() == [0, 0, n, 0, 0, 0, 0, 0]
        assert got[4096 // 4:4096 // 4 + 2].tolist() == [0, 0] and got[8192 // 4:8192 // 4 + 4].tolist() == [0, 0, 0, 0]
    for b in (buf, out, w):
        b.free()


# ------------------------------------------------------------------ 14. end to end

E2E = [b"a", b"ab", b"abc", b"bc", b"bcd", b"cd", b"dddd"]
E2E_REPL = [b"", b"<AB>", None, ("fill", 0x2D), b"0123456789", b"C", b"#"]


def test_scan_rewrite(gpu):
    rng = np.random.default_rng(31)
    s = Set(E2E, E2E_REPL)
    text = bytes(random_text(64 * 1024, 21, b"abcd"))
    out, info, at, seg = s.m.scan_rewrite(text)
    exp = rw.re_sub(E2E, s.repl, text)
    assert out == exp and seg is None and info[0] == at.size > 20000 and info[1] == 0 and info[6] == 0
    assert ((int(info[3]) << 32) | (int(info[2]) & 0xFFFFFFFF)) == len(exp)
    cells, offs = rw.selected(E2E, [text])
    xo, xinfo, xat, _ = s.model.run(text, cells, offs)
    assert xo == exp and info.tolist() == xinfo and at.tolist() == xat
    # as texts: every text rewritten alone, found in the output by seg_out
    cuts = np.sort(rng.integers(0, 20000, 30))
    texts = [text[a:b] for a, b in zip(np.r_[0, cuts], np.r_[cuts, 20000])]
    texts = texts[:12] + [b""] + texts[12:]
    out, info, at, seg = s.m.scan_rewrite(texts=texts)
    assert seg.size == len(texts) and seg[0] == 0
    ends = np.r_[seg[1:], len(out)]
    for k, t in enumerate(texts):
        assert out[seg[k]:ends[k]] == rw.re_sub(E2E, s.repl, t), k
    assert out != rw.re_sub(E2E, s.repl, text[:20000])             # a cut inside a match changes the result
    # an output that does not fit is an error
    with pytest.raises(AcmError) as e:
        s.m.scan_rewrite(text, out_capacity=len(exp) - 1)
    assert e.value.code == _lib.ACM_ERR_CAPACITY
    assert s.m.scan_rewrite(text, out_capacity=len(exp))[0] == exp
    # before: a match may begin in the bytes in front; the output is before + text, rewritten
    assert text[:5] == b"bdbcb"
    out, info, at, seg = s.m.scan_rewrite(text[3:3000], before=text[:3], init_state=s.m.scan_all(text[:3])[2])
    assert out == rw.re_sub(E2E, s.repl, text[:3000]) and out.startswith(b"bd--")
    s.close()


def test_scan_rewrite_identity_nocase_mixed_positioned(gpu):
    text = bytes(random_text(16 * 1024, 22, b"abcdABCD"))
    # every pattern replaced by itself
    s = Set(E2E, list(E2E))
    out, info, at, _ = s.m.scan_rewrite(text)
    assert out == text and info[0] > 1500                       # (one byte in eight is an a, and every a begins a match)
    s.close()
    # a nocase set
    s = Set(E2E, E2E_REPL, nocase=True)
    out, info, at, _ = s.m.scan_rewrite(text)
    assert out == rw.re_sub(E2E, s.repl, text, nocase=True) and out != rw.re_sub(E2E, s.repl, text)
    s.close()
    # a mixed set: the case pass makes the candidates exact before they are selected
    pats = [(b"Ab", True), (b"abc", False), (b"BC", False), (b"cD", True), (b"d", False)]
    a = Automaton()
    for i, (p, nc) in enumerate(pats):
        a.add(p, i, nocase=nc)
    s = Set(None, [b"[ab]", b"", ("fill", 0x2E), None, b"DD"], automaton=a)
    assert a.mixed_case
    cells, offs = rw.occurrences(pats, [text])
    ep, eo, _, _ = s.model.sel.run(cells, offs)
    xo, xinfo, xat, _ = s.model.run(text, ep, eo)
    out, info, at, _ = s.m.scan_rewrite(text)
    assert out == xo and info.tolist() == xinfo and at.tolist() == xat and set(ep.tolist()) == set(range(5))
    s.close()
    # a positioned set, as texts
    plain = [b"ab", b"abc", b"bc", b"c", b"dd"]
    windows = {0: (0, 0, False), 1: (2, None, False), 3: (1, 4, True)}
    a = Automaton()
    for i, p in enumerate(plain):
        a.add(p, i)
    for i, (lo, hi, fe) in windows.items():
        a.set_position(i, lo, hi, fe)
    s = Set(None, [b"AB", b"", b"<bc>", ("fill", 0x5F), None], automaton=a)
    texts = [b"abcabc", b"ab", b"", b"cabcddabc", b"ddd", b"abcc", b"xxabcxx", b"abab"]
    cells, offs = rw.occurrences(plain, texts, windows=windows)
    ep, eo, _, _ = s.model.sel.run(cells, offs)
    starts = np.r_[0, np.cumsum([len(t) for t in texts])[:-1]]
    xo, xinfo, xat, xseg = s.model.run(b"".join(texts), ep, eo, seg_start=starts)
    out, info, at, seg = s.m.scan_rewrite(texts=texts)
    assert out == xo and info.tolist() == xinfo and at.tolist() == xat and seg.tolist() == xseg
    s.close()
