"""The normalise and remap kernels (csrc/normalize.hip) where test_gpu_normalize.py stops: more text starts and more
records than the grid has threads, a map of tens of thousands of cells searched by the remap, runs of cells that emit
nothing (equal d_block cells: the search must take the last of them), and starts taken through the wildcard table.
Expected values are the serial model's (tests/normalize_model.py); buffers, poison and guards as in
test_gpu_normalize.py, whose Call, Mapped, run and upload_text do the work here too.

The builders and the conditions that keep a case from being vacuous (m over the grid, equal consecutive cells, which
records' starts land where) need no device: tests/test_host_normalize.py checks them on the host."""
import functools

import numpy as np
import pytest

import normalize_model as nm
import ops_guard as og
import wildcard_model as wm
from gpu_pattern_matching_amd import Automaton, Matcher
from gpu_pattern_matching_amd._lib import check
from normalize_model import PERCENT, SQUEEZE, STRIP
from test_gpu_normalize import PATS, TILE, Call, Mapped, mode_id, random_text, run, upload_text

pytestmark = pytest.mark.gpu

GRID_THREADS = 1024 * 256          # the most threads any of the kernels' grids has
ORIGIN = -12345


@pytest.fixture(scope="module", autouse=True)
def needs_gpu(gpu):
    return gpu


@pytest.fixture(scope="module")
def matcher(gpu):
    a = Automaton()
    for i, p in enumerate(PATS):
        a.add(p, i)
    a.compile()
    m = Matcher(a, 0, max_text=1 << 16)
    yield m
    m.close()


def mapped(lib, text, flags, x, origin=0, seg_start=None):
    """a Mapped around a model result that exists already (Mapped itself would walk the text again)"""
    mp = Mapped.__new__(Mapped)
    mp.text, mp.flags, mp.origin, mp.x = np.asarray(text, dtype=np.uint8), flags, origin, x
    mp.dt = upload_text(mp.text)
    mp.call = Call(lib, mp.dt, mp.text.size, flags, x.m + 16, origin, seg_start=seg_start)
    return mp


def close_whole(mp, seg, what):
    """what the normalise call of a Mapped left, compared whole with the model (guards checked), and its buffers freed"""
    got, x = mp.call.read(what), mp.x
    mp.dt.free()
    assert got["info"].tolist() == x.info, "%s: info %s, model %s" % (what, got["info"].tolist(), x.info)
    og.same(got["keep"], x.keep_words, what + ": keep words")
    og.same(got["block"], x.block, what + ": block cells")
    og.same(got["out"][:x.m], np.frombuffer(x.out, dtype=np.uint8), what + ": output")
    assert (got["out"][x.m:] == og.FILL).all(), "%s: a byte behind m was written" % what
    if seg:
        og.same(got["seg"], x.seg_out, what + ": seg_out")


def remap_all(lib, matcher, mp, seed, what):
    """every output offset (and m, m + 1, -1): plain, with starts through PATS, in place"""
    m = mp.x.m
    offs = np.r_[np.arange(m), m, m + 1, -1]
    mp.remap(lib, matcher, offs, what=what + ", every offset")
    mp.remap(lib, matcher, offs, pats=np.random.default_rng(seed).integers(0, len(PATS), offs.size), what=what + ", starts")
    mp.remap(lib, matcher, offs[::-1].copy(), in_place=True, what=what + ", in place")


# ------------------------------------------------------------------ 1. more items than the grid has threads


@functools.lru_cache(maxsize=None)
def grid_case(flags):
    """(text, starts, the model's result): 600 001 bytes and 300 000 starts, one every 2 bytes; 40 in front of the origin
    and 40 at and behind the text's end (clamped); 50 000 equal ones, which leave 100 000 bytes without a start, where
    triples and runs live"""
    n = 600001
    text = random_text(n, 900 + flags)
    k = np.arange(300000, dtype=np.int64)
    starts = ORIGIN + 2 * k
    starts[:40] = ORIGIN - 40 + k[:40]
    starts[-40:] = ORIGIN + n + k[:40]
    starts[50000:100000] = starts[50000]
    starts[200000:200010] = starts[200000]
    starts.sort()
    x = nm.normalize(text.tobytes(), flags, origin=ORIGIN, seg_start=starts.tolist())
    return text, starts.astype(np.int32), x


def check_grid_case(flags):
    """the conditions of the case, from the model alone"""
    text, starts, x = grid_case(flags)
    assert starts.size > GRID_THREADS and x.m > GRID_THREADS              # the second trip of k_norm_starts and of k_norm_remap
    assert (starts < ORIGIN).sum() == 40 and (starts >= ORIGIN + text.size).sum() == 40 and np.unique(starts).size < starts.size - 50000
    assert x.info[2] > 1000 and x.info[1] > 5000                           # triples and dropped units where no start cuts them
    return text, starts, x


@pytest.mark.parametrize("flags", [PERCENT | SQUEEZE, PERCENT | STRIP], ids=mode_id)
def test_more_items_than_threads(lib, matcher, flags):
    text, starts, x = check_grid_case(flags)
    mp = mapped(lib, text, flags, x, ORIGIN, starts)
    remap_all(lib, matcher, mp, flags, "more records than threads")
    close_whole(mp, True, "more starts than threads")


# ------------------------------------------------------------------ 2. a map of many cells

REPS = 520


@functools.lru_cache(maxsize=None)
def tiled_period():
    """the period of test_gpu_normalize.test_a_block_of_several_tiles and the model's walk over it: the period begins and
    ends with a letter, so the whole text's result is the period's, repeated"""
    period = random_text(4 * TILE + 1024, 9)
    period[0] = period[-1] = 0x78
    return period, nm.normalize(period.tobytes(), PERCENT | SQUEEZE)


class Shifted:
    """first[] or last[] of the repeated text, by index, from the period's"""

    def __init__(self, a, m, size):
        self.a, self.m, self.size = a, m, size

    def __getitem__(self, o):
        return (o // self.m) * self.size + int(self.a[o % self.m])


class Tiled:
    """what nm.remap reads of a Norm, for the period repeated"""

    def __init__(self, p, size, reps):
        self.m = reps * p.m
        self.first, self.last = Shifted(p.first, p.m, size), Shifted(p.last, p.m, size)


def tiled_offsets(p, size, reps):
    """the first and last output byte of every 97th period; every offset within 2 of the first byte a cell emits, for 512
    cells spread over the text; m - 1, m, m + 1"""
    M, cells = reps * p.m, size // nm.BLOCK
    offs = [r * p.m + d for r in range(0, reps, 97) for d in (0, p.m - 1)]
    for j in np.linspace(1, reps * cells - 1, 512).astype(np.int64).tolist():
        at = (j // cells) * p.m + int(p.block[j % cells])
        offs += [o for o in range(at - 2, at + 3) if 0 <= o < M]
    return np.array(offs + [M - 1, M, M + 1], dtype=np.int64)


@pytest.fixture(scope="module")
def tiled(lib):
    """the 34 MiB text of test_a_block_of_several_tiles normalised once, its map left on the device (no output: that
    test compares it)"""
    period, p = tiled_period()
    text = np.tile(period, REPS)
    mp = Mapped.__new__(Mapped)
    mp.text, mp.flags, mp.origin, mp.x = text, PERCENT | SQUEEZE, 0, Tiled(p, period.size, REPS)
    mp.dt = upload_text(text)
    mp.call = Call(lib, mp.dt, text.size, mp.flags, 0, with_out=False)
    yield mp
    for b in (mp.call.out, mp.call.keep, mp.call.block, mp.call.info, mp.call.ws, mp.dt):
        b.free()


def test_a_map_of_many_cells(lib, matcher, tiled):
    period, p = tiled_period()
    cells = period.size // nm.BLOCK
    assert tiled.text.size // nm.BLOCK > 32768 and REPS * p.m < 2 ** 31
    offs = tiled_offsets(p, period.size, REPS)
    assert 2000 < offs.size < 5000 and np.unique(offs // p.m).size > 300
    rng = np.random.default_rng(2)
    tiled.remap(lib, matcher, offs, what="many cells")
    tiled.remap(lib, matcher, offs, pats=rng.integers(0, len(PATS), offs.size), what="many cells, starts")
    tiled.remap(lib, matcher, offs[::-1].copy(), in_place=True, what="many cells, in place")
    # the map that was searched is the model's, and the calls above left it alone
    c = tiled.call
    c.ws.check(None, "many cells")
    assert c.info.read(what="many cells").tolist() == [REPS * p.m, REPS * p.info[1], REPS * p.info[2], REPS * p.info[3], 0, 0, 0, 0]
    og.same(c.keep.read(what="many cells"), np.tile(p.keep_words, REPS), "keep words")
    block = (np.arange(REPS, dtype=np.int64)[:, None] * p.m + p.block[None, :cells]).reshape(-1)
    og.same(c.block.read(what="many cells"), np.r_[block, REPS * p.m], "block cells")
    c.out.untouched(what="many cells: no output was asked for")


# ------------------------------------------------------------------ 3. cells that emit nothing


def blanks(k):
    return np.frombuffer(b" \t\n\r", dtype=np.uint8)[np.arange(k) % 4]


def dropped_cell_texts():
    """(name, text, modes, starts, equal): texts in which whole 1024-byte cells emit nothing under `modes`, text starts
    some of which lie in those cells, and how many pairs of equal consecutive d_block cells there are at the least"""
    n, X = 3 * TILE + 100, 0x78
    both = (STRIP, SQUEEZE, PERCENT | STRIP, PERCENT | SQUEEZE)
    out = []
    j = 9                                                              # a run that covers cells j .. j + 4; under squeeze
    t = random_text(n, 301)                                            # its one blank lies in cell j - 1
    lo, hi = j * 1024 - 5, (j + 5) * 1024 + 7
    t[lo:hi] = blanks(hi - lo)
    t[lo - 1] = t[hi] = X
    out.append(("a run over five cells", t, both, [0, j * 1024 + 1, (j + 2) * 1024 + 500, (j + 4) * 1024 + 1023, hi], 4))
    t = random_text(n, 302)                                            # the last 5 KiB: several cells equal m
    t[n - 5120:] = blanks(5120)
    t[n - 5121] = X
    out.append(("a blank tail", t, both, [0, n - 5000, n - 1024, n - 1, n], 4))
    t = random_text(n, 303)                                            # the first 3 KiB: the leading cells are 0
    t[:3072] = blanks(3072)
    t[3072] = X
    out.append(("a blank head", t, both, [0, 1, 1024, 2047, 3072], 2))
    for k, (triple, modes) in enumerate(((b"%20", (PERCENT | STRIP, PERCENT | SQUEEZE)), (b"%41", (PERCENT | STRIP,)))):
        c = 20 + k                                                     # cell c: the two digits of a triple headed in
        t = random_text(n, 304 + k)                                    # cell c - 1, and blanks
        t[c * 1024 - 1:c * 1024 + 2] = np.frombuffer(triple, dtype=np.uint8)
        t[c * 1024 + 2:(c + 1) * 1024] = blanks(1022)
        t[c * 1024 - 2] = t[(c + 1) * 1024] = X
        out.append(("the digits of %s" % triple.decode(), t, modes, [0, c * 1024, c * 1024 + 1, c * 1024 + 2, (c + 1) * 1024], 1))
    t = random_text(3 * TILE, 306)                                     # n a multiple of 1024
    t[-2100:] = blanks(2100)
    t[-2101] = X
    out.append(("n = 48 cells", t, both, [0, 3 * TILE - 1500, 3 * TILE], 2))
    for k, last in enumerate((X, 0x20)):                               # and one byte more: a letter, a blank
        t = random_text(3 * TILE + 1, 307 + k)
        t[-2101:] = blanks(2101)
        t[-2102] = X
        t[-1] = last
        out.append(("n = 48 cells and a %s" % ("letter", "blank")[k], t, both, [0, 3 * TILE - 1500, 3 * TILE, 3 * TILE + 1], 2))
    return out


def equal_cells(x):
    """pairs of consecutive d_block cells that are equal: a cell that emits nothing"""
    return int((np.diff(x.block) == 0).sum())


DROPPED = [(name, f) for name, _, modes, _, _ in dropped_cell_texts() for f in modes]


@pytest.mark.parametrize("name,flags", DROPPED, ids=["%s-%s" % (n.replace(" ", "_"), mode_id(f)) for n, f in DROPPED])
def test_cells_that_emit_nothing(lib, matcher, name, flags):
    t, starts, least = next((t, s, e) for nme, t, _, s, e in dropped_cell_texts() if nme == name)
    run(lib, t, flags, seg_start=starts, what=name)                  # whole, d_seg_out of the starts in the dropped cells too
    mp = Mapped(lib, t, flags)
    assert equal_cells(mp.x) >= least, (name, mode_id(flags), equal_cells(mp.x))
    remap_all(lib, matcher, mp, 5, name)
    mp.close()
    mp = Mapped(lib, t, flags, origin=ORIGIN, seg_start=[ORIGIN + s for s in starts])
    remap_all(lib, matcher, mp, 6, name + ", texts")
    close_whole(mp, True, name + ", texts")


# ------------------------------------------------------------------ 4. starts through the wildcard table

ANY = bytes(range(256))
WILD = [[b"ab", 0x68, 0x72, 0x65, 0x66, b"xy ", ANY],                  # [ab] href [xy ] ?     pre 1, post 2
        [ANY, b"%a", 0x30, 0x41, b" b"],                               # ? [%a] 0A [ b]        pre 2, post 1
        [b" \t", ANY, ANY, 0x61, 0x20, 0x62, ANY]]                     # [ \t] ? ? 'a b' ?     pre 3, post 1
PLAIN = [b"href", b"a", b"0A"]


def wild_set():
    """(patterns of the model, start distance per pattern): a record (p, o) starts at o - L + 1 - pre"""
    pats = wm.as_patterns(WILD + [list(p) for p in PLAIN])
    assert [(p.pre, p.L, p.post) for p in pats] == [(1, 4, 2), (2, 2, 1), (3, 3, 1), (0, 4, 0), (0, 1, 0), (0, 2, 0)]
    return pats, [p.L + p.pre for p in pats]


@functools.lru_cache(maxsize=None)
def wild_case(flags):
    """(text, model result, offsets, patterns): every output offset under every pattern"""
    text = np.concatenate([np.frombuffer(b"%41b  \t href%20%09x", dtype=np.uint8), random_text(2 * nm.BLOCK + 77, 400 + flags,
                                                                                                b"a b%4%200Ahref \t")])
    x = nm.normalize(text.tobytes(), flags)
    offs = np.repeat(np.arange(x.m), len(WILD) + len(PLAIN))
    pats = np.tile(np.arange(len(WILD) + len(PLAIN)), x.m)
    return text, x, offs, pats


def wild_starts(flags):
    """per record of wild_case its start in the normalised text, and the counts the test wants to be positive: records of
    the wildcard patterns whose start is offset 0, is -1, is emitted by a triple, is the one blank of a squeezed run"""
    text, x, offs, pats = wild_case(flags)
    model, dist = wild_set()
    s = offs - np.array(dist)[pats] + 1
    wild = pats < len(WILD)
    inside = wild & (s >= 0)
    triple = np.zeros(s.size, dtype=bool)
    triple[inside] = x.last[s[inside]] - x.first[s[inside]] == 2
    t = text.tobytes()
    run_blank = np.zeros(s.size, dtype=bool)
    if flags & SQUEEZE:
        for k in np.flatnonzero(inside).tolist():
            f = int(x.first[s[k]])
            run_blank[k] = x.out[s[k]] == 0x20 and x.last[s[k]] == f and t[f] in nm.DEFAULT_BLANKS and t[f + 1:f + 2] != b"" and \
                t[f + 1] in nm.DEFAULT_BLANKS
    return s, dict(zero=int((wild & (s == 0)).sum()), minus_one=int((wild & (s == -1)).sum()), triple=int(triple.sum()),
                   run=int(run_blank.sum()))


def check_wild_case(flags):
    s, seen = wild_starts(flags)
    assert seen["zero"] == len(WILD) and seen["minus_one"] == len(WILD) and seen["triple"] > 20, seen
    assert seen["run"] > 20 or not flags & SQUEEZE, seen
    return s


@pytest.mark.parametrize("flags", [PERCENT | SQUEEZE, PERCENT | STRIP], ids=mode_id)
def test_wildcard_spans(lib, flags):
    model, dist = wild_set()
    a = Automaton()
    for i, p in enumerate(WILD):
        assert a.add_wildcard(p, i) == i
    for i, p in enumerate(PLAIN):
        a.add(p, len(WILD) + i)
    for i, w in enumerate(model):                                    # pre, post and L as the automaton itself has them
        assert a.pattern(i)[0] == w.anchor and len(w.anchor) == w.L and a.wildcard_lengths(i) == (w.pre, w.post)
    a.compile()
    assert a.has_wildcards
    m = Matcher(a, 0, max_text=4096)
    text, x, offs, pats = wild_case(flags)
    s = check_wild_case(flags)
    mp = mapped(lib, text, flags, x)
    for in_place in (False, True):
        what = "wildcard spans" + (", in place" if in_place else "")
        plane = np.r_[offs.size, offs].astype(np.int32)
        off_in = og.Guarded(offs.size + 1, host=plane)
        off_out = off_in if in_place else og.Guarded(offs.size + 1)
        pat_in = og.Guarded(offs.size + 1, host=np.r_[offs.size, pats].astype(np.int32))
        start, info = og.Guarded(offs.size + 1), og.Guarded(8)
        check(lib.acm_normalize_remap_async(m.dfa, mp.dt.ptr, text.size, 0, flags, mp.call.keep.ptr, mp.call.block.ptr, pat_in.ptr,
                                            off_in.ptr, offs.size, off_out.ptr, start.ptr, info.ptr, None), "acm_normalize_remap_async")
        ok = s >= 0                                                 # (every offset lies in the text; s < m as well)
        exp_start = np.where(ok, x.first[np.maximum(s, 0)], -1)
        assert info.read(what=what).tolist() == [offs.size, int((~ok).sum()), 0, 0, 0, 0, 0, 0]
        og.same(start.read(what=what), np.r_[offs.size, exp_start], what + ": starts")
        og.same(off_out.read(what=what), np.r_[offs.size, x.last[offs]], what + ": ends")
        og.same(pat_in.read(what=what), np.r_[offs.size, pats], what + ": the pattern plane")
        for b in {off_in, off_out, pat_in, start, info}:
            b.free()
    close_whole(mp, False, "wildcard spans")
    m.close()
    a.close()
