"""The emit kernel's rounds of 256 rows and the walker's short load chain, bit for bit against the oracle.

k_sieve_emit runs in 256-thread workgroups: the walker's row on its own, then the rows behind it 256 a round
(sparse.hip).  A round hands the next one the largest extent so far (which shadows the heads of the next
round's rows) and the number of cells written so far.  Here:

A. row counts either side of a round: single batches of 256, 257, 257, 513 (the most) and 258 rows, launch
   groups of four with 257 and 256 rows of 16 tiles;
B. records on both sides of the borders between rows 255 | 256 | 257 and 511 | 512: signatures that end in the
   last tile of a row and start in the first of the next, and a nested pair whose outer follower starts in
   the earlier row and shadows the head of the next row's list (tests/sieve_model.py's followers / surviving
   say on the CPU that the placement does that);
C. rounds without records: records in the last row only, none at all, and only in the walker's row (a state
   carried in from the batch in front through d_init_plane);
D. more cells than threads: over 100 k records in 4 MiB, and the same text into planes smaller than that;
E. the helped variant (ACM_SIEVE_HELPERS=1, read once per process: a fresh child) on a sample-heavy 4 MiB text
   whose blocks have sub-rows in every round, and on the texts of B;
F. the walk at the end of the text: texts of 1, 2, tail_walk - 1, tail_walk, tail_walk + 1 bytes (texts under
   64 bytes are the chain pipeline's whatever the mode: the smallest sparse ones, 64 and 65 bytes, are here
   too), and a text that ends inside a pattern at every depth 1..D, for a set with 3-byte filter keys, one with
   6-byte keys (tail_walk = W + 4) and a nocase set, each alone and as the last batch of a group of four.

Planes and workspaces are filled with a poison byte before every launch (tests/poison.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import poison
import sieve_model as sm
import variants
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
MAX_TILES = 4096
INNER = b"inner=nested"                       # a pattern, and a part of OUTER: the pair of B
OUTER = b"OUTER-lead:" + INNER + b"-tail"
LONG = b"carried/over/the/batch/border!"      # C: cut between two batches
BEHIND = b"right-behind"


def rows_of(n, tpc):
    """static rows of a text of n bytes with blocks of tpc tiles (sparse.hip: geometry_for)"""
    tile = KiB
    while -(-n // tile) > MAX_TILES:
        tile *= 2
    return -(-(-(-n // tile)) // tpc) + 1


def patterns():
    return sm.seam_patterns() + [INNER, OUTER, LONG, BEHIND]


_built = {}


def the_set():
    """(patterns, model): shortest 10, so W = 8, D = 10, 3-byte filter keys; built once"""
    if not _built:
        pats = patterns()
        m = sm.Model(pats)
        assert (m.W, m.D, m.LG) == (8, 10, 3)
        _built["set"] = (pats, m)
    return _built["set"]


def compiled(pats):
    a, o = Automaton(), orc.Oracle()
    for i, p in enumerate(pats):
        a.add(p, i + 1)
        o.add(p, i + 1)
    a.compile()
    o.compile()
    return a, o


@pytest.fixture(scope="module")
def kit(gpu):
    pats, model = the_set()
    a, o = compiled(pats)
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    assert m.set_mode("sparse") == "sparse"
    yield m, o, model
    m.close()
    a.close()
    o.close()


class Bufs:
    """device buffers of a test, freed together"""

    def __init__(self):
        self.all = []

    def new(self, nbytes, byte):
        b = DeviceArray(nbytes)
        b.fill(byte)
        self.all.append(b)
        return b

    def text(self, t):
        b = DeviceArray.from_numpy(np.ascontiguousarray(t))
        self.all.append(b)
        return b

    def free(self):
        for b in self.all:
            b.free()
        self.all = []


def scan_checked(m, o, texts, inits=None, cap=None, init_planes=None, what="", text_of=None, expect_path="sparse"):
    """One launch: a batch alone (one text) or a launch group (several of one size), poisoned workspaces and
    planes, every batch's planes against the oracle.  init_planes: per batch None or (pat plane, capacity, state)
    of the scan whose final state it starts in.  Returns the oracle's results."""
    n = texts[0].size
    assert all(t.size == n for t in texts)
    inits = inits or [0] * len(texts)
    init_planes = init_planes or [None] * len(texts)
    text_of = text_of or (lambda t: t)
    exps = [o.scan(text_of(t), ip[2] if ip else s) for t, s, ip in zip(texts, inits, init_planes)]
    c = cap or max(e[0].size for e in exps) + 2 + 64
    wsb = m.lib.acm_scan_workspace_bytes(m.dfa, n)
    bufs = Bufs()
    try:
        d = [bufs.text(t) for t in texts]
        ws = [bufs.new(wsb, 0xA5) for _ in texts]
        pl = [(bufs.new(c * 4, poison.PLANE_POISON), bufs.new(c * 4, poison.PLANE_POISON)) for _ in texts]
        batches = [m.make_batch(d[k], n, m.stream, pl[k][0], pl[k][1], c, (ws[k].ptr, wsb), init_state=inits[k],
                                init_plane=init_planes[k][0] if init_planes[k] else None,
                                init_plane_capacity=init_planes[k][1] if init_planes[k] else 0)
                   for k in range(len(texts))]
        if len(batches) == 1:
            m.enqueue(batches[0])
        else:
            m.enqueue_many(batches)
        for k in range(len(texts)):
            poison.check_planes(pl[k][0], pl[k][1], c, exps[k], what="%s batch %d of %d, n=%d" % (what, k, len(texts), n),
                                stream=m.stream)
            if expect_path and n >= 64:
                assert m.path_taken(n, workspace=(ws[k].ptr, wsb)) == expect_path
    finally:
        bufs.free()
    return exps


# ------------------------------------------------------------------------------------------------- texts
def border_bytes():
    """the borders between rows r and r + 1 that lie at a round's edge: rows of 8 tiles (a batch alone, up to 4 MiB)
    and of 16 tiles (a launch group)"""
    return sorted({8 * KiB * r for r in (255, 256, 511)} | {16 * KiB * 255})


def ends_text(model, n):
    """quiet filler with, at every round border, a signature that ends with the last tile of the row in front and
    one that starts with the first tile of the row behind, and a signature at the very end"""
    t = model.filler_text(n, 1)
    pats = model.patterns
    for i, b in enumerate(border_bytes()):
        if b + 64 <= n:
            p, q = pats[i % 24], pats[24 + i % 24]
            sm.plant(t, b - len(p), p)
            sm.plant(t, b, q)
            sm.plant(t, b - 3 * KiB, pats[(i + 5) % 24])       # and one in the middle of the row in front
    sm.plant(t, n - len(pats[7]), pats[7])
    return t


def nested_text(model, n, check=True):
    """quiet filler with, at every round border b, OUTER planted so that its own sample lies in the last tile of the
    row in front (start b - 11, sample b - 8) and INNER, a part of it, starts at b: INNER's follower is the head of
    the next row's list and OUTER's extent shadows its hit.  At every other border a pattern follows right behind
    OUTER, so that one row loses its whole list and the other only its head."""
    t = model.filler_text(n, 1)
    at = []
    for i, b in enumerate(border_bytes()):
        if b + 64 <= n:
            s = b - len(b"OUTER-lead:")
            sm.plant(t, s, OUTER)
            if i % 2 == 0:
                sm.plant(t, s + len(OUTER), BEHIND)
            at.append((b, s, i % 2 == 0))
    sm.plant(t, n - len(model.patterns[9]), model.patterns[9])
    if check:
        for b, s, behind in at:
            lo = b - 4 * KiB                                    # a slice on the sample and tile grid around the border
            fols = sm.followers(model, t[lo:b + 4 * KiB])
            kept = sm.surviving(fols)
            outer = [k for k, f in enumerate(fols) if f[0] + lo == s]
            inner = [k for k, f in enumerate(fols) if f[0] + lo == b]
            assert len(outer) == 1 and len(inner) == 1, "the nested pair's followers at border %d" % b
            fo, fi = fols[outer[0]], fols[inner[0]]
            assert fo[1] + lo < b <= fi[1] + lo, "OUTER's sample in front of border %d, INNER's behind it" % b
            assert fi[3] and not kept[inner[0]], "INNER's hit is shadowed by OUTER's extent"
            assert fo[2] + lo == s + len(OUTER) and len(kept[outer[0]]) == 2
            later = [k for k, f in enumerate(fols) if f[0] + lo > b and kept[k]]
            assert bool(later) == behind, "a surviving hit behind the dropped head in the same row"
    return t


def dense_text(model, n, stretch, every, start=20 * KiB):
    """quiet filler with stretches of "abab..." (a record at every position of a stretch from its tenth byte on)"""
    t = model.filler_text(n, 1)
    for at in range(start, n - stretch - 64, every):
        sm.plant(t, at, (b"ab" * (stretch // 2 + 1))[:stretch])
    return t


# ----------------------------------------------------------------------------------------------------- A, B
SINGLE = [(2040 * KiB, 256), (2040 * KiB + 1, 257), (2048 * KiB, 257), (4 * MiB, 513), (4 * MiB + 1, 258)]
GROUPS = [(4 * MiB, 257), (4080 * KiB, 256)]


@pytest.mark.parametrize("n,rows", SINGLE, ids=["n=%d rows=%d" % c for c in SINGLE])
def test_row_count_seams_single(kit, n, rows):
    m, o, model = kit
    assert rows_of(n, 8) == rows
    for name, t in (("ends", ends_text(model, n)), ("nested", nested_text(model, n))):
        exp = scan_checked(m, o, [t], inits=[3], what=name)[0]
        assert exp[0].size >= (3 if n > 2040 * KiB + 64 else 1)     # (the smallest text ends at the first border)


@pytest.mark.parametrize("n,rows", GROUPS, ids=["n=%d rows=%d" % c for c in GROUPS])
def test_row_count_seams_group(kit, n, rows):
    m, o, model = kit
    assert rows_of(n, 16) == rows
    e, s = ends_text(model, n), nested_text(model, n)
    texts = [e, s, np.roll(e, 8 * KiB), model.filler_text(n, 1)]
    exps = scan_checked(m, o, texts, inits=[0, 5, 0, 9], what="group")
    assert exps[0][0].size >= 3 and exps[1][0].size >= 3 and exps[3][0].size == 0


# -------------------------------------------------------------------------------------------------------- C
def test_empty_rounds(kit):
    m, o, model = kit
    n = 4 * MiB
    last = model.filler_text(n, 1)
    sm.plant(last, n - len(model.patterns[3]), model.patterns[3])
    exp = scan_checked(m, o, [last], what="records in the last row only")[0]
    assert exp[0].size == 1 and exp[0][0] == n - 1
    quiet = model.filler_text(n, 1)
    exp = scan_checked(m, o, [quiet], what="no records")[0]
    assert exp[0].size == 0
    # the walker's row only: the batch in front ends inside LONG, its planes hand the state over
    cut = 17
    front = model.filler_text(64 * KiB, 1)
    sm.plant(front, front.size - cut, LONG[:cut])
    behind = model.filler_text(n, 1)
    sm.plant(behind, 0, LONG[cut:])
    wsb = m.lib.acm_scan_workspace_bytes(m.dfa, front.size)
    bufs = Bufs()
    try:
        d, ws = bufs.text(front), bufs.new(wsb, 0xA5)
        cap = 16
        p, q = bufs.new(cap * 4, poison.PLANE_POISON), bufs.new(cap * 4, poison.PLANE_POISON)
        m.scan_async(d, front.size, 0, pat_plane=p, off_plane=q, plane_capacity=cap, workspace=(ws.ptr, wsb))
        e0 = o.scan(front)
        poison.check_planes(p, q, cap, e0, what="the batch in front", stream=m.stream)
        assert e0[2] != 0 and e0[0].size == 0
        for group in (1, 4):
            texts = [behind] + [quiet] * (group - 1)
            exps = scan_checked(m, o, texts, init_planes=[(p, cap, e0[2])] + [None] * (group - 1),
                                what="records in the walker's row only")
            assert exps[0][0].tolist() == [len(LONG) - cut - 1]
    finally:
        bufs.free()


# -------------------------------------------------------------------------------------------------------- D
def test_more_cells_than_threads(kit):
    m, o, model = kit
    n = 4 * MiB
    t = dense_text(model, n, 2 * KiB, 64 * KiB)
    sm.plant(t, n - len(model.patterns[3]), model.patterns[3])
    quiet = model.filler_text(n, 1)
    exp = scan_checked(m, o, [t], what="dense")[0]
    assert exp[0].size >= 100000
    # the same into planes that are too small: the header counts every record, the trailer sits in the last cell;
    # behind the dense batch the launch has helper waves, behind a quiet one it has none
    scan_checked(m, o, [t], cap=50000, what="dense, small planes, helped")
    scan_checked(m, o, [quiet], what="quiet")
    scan_checked(m, o, [t], cap=50000, what="dense, small planes")
    scan_checked(m, o, [quiet], what="quiet")
    scan_checked(m, o, [t, quiet, t, quiet], cap=3000, what="dense group, small planes")
    scan_checked(m, o, [quiet], what="quiet")      # (the module's next launch without helper waves)


# -------------------------------------------------------------------------------------------------------- E
def helped_texts(model):
    n = 4 * MiB
    heavy = dense_text(model, n, 4 * KiB, 64 * KiB, start=20 * KiB + 8)
    for i, b in enumerate(border_bytes()):      # records at the round borders too
        sm.plant(heavy, b - 10, model.patterns[i % 24])
        sm.plant(heavy, b, model.patterns[24 + i % 24])
    return [heavy, ends_text(model, n), nested_text(model, n, check=False), ends_text(model, 2040 * KiB + 1)]


def test_helped_variant_in_a_child(kit):
    """ACM_SIEVE_HELPERS is read once per process: the scans run in a child started with it"""
    m, o, model = kit
    heavy = helped_texts(model)[0]
    # a stretch of 4 KiB flags more than 256 samples of its block: the block has a sub-row, there are 63 such blocks
    # from the first round to the last, and 513 static rows: more than 512 rows in all
    stretches = list(range(20 * KiB + 8, heavy.size - 4 * KiB - 64, 64 * KiB))
    lo = stretches[0] // (8 * KiB) * (8 * KiB)
    assert model.flagged_positions(heavy[lo:lo + 8 * KiB]).size > 256 and rows_of(heavy.size, 8) == 513
    assert stretches[0] < 2 * MiB - 64 * KiB and stretches[-1] > 4 * MiB - 128 * KiB and len(stretches) > 60
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ACM_SIEVE_HELPERS="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "helped"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "helped ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def helped_child():
    pats, model = the_set()
    a, o = compiled(pats)
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    assert m.set_mode("sparse") == "sparse"
    texts = helped_texts(model)
    for i, t in enumerate(texts):
        exp = scan_checked(m, o, [t], inits=[i], what="helped text %d" % i)[0]
        assert exp[0].size >= (3 if t.size == 4 * MiB else 1)
    assert scan_checked(m, o, [texts[0]], cap=70000, what="helped, small planes")[0][0].size > 200000
    scan_checked(m, o, texts[:3] + [texts[1]], what="helped group")
    m.close()
    print("helped ok")


# -------------------------------------------------------------------------------------------------------- F
TAIL_REGIMES = ("s10_letters", "s16_letters", "s8_mixed")


@pytest.mark.parametrize("regime", TAIL_REGIMES)
def test_tail_walk(gpu, regime):
    vs = variants.regime(regime)
    W, D = vs.stride, min(vs.shortest, 10)
    tail_walk = max(D - 1, W + 4) if vs.key_len == 6 else D - 1
    assert vs.key_len == {"s10_letters": 3, "s16_letters": 6, "s8_mixed": 3}[regime]
    assert vs.nocase == (regime == "s8_mixed") and tail_walk <= 12
    a, o = vs.compiled()
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    rng = np.random.default_rng(len(regime))
    try:
        assert m.set_mode("sparse") == "sparse"
        base = variants.text(vs, 3000, 21, "random")
        others = [variants.text(vs, 3000, 22 + k, "planted") for k in range(3)]
        longest = max(vs.patterns, key=len)
        pieces = []
        for n in (1, 2, tail_walk - 1, tail_walk, tail_walk + 1, 64, 65):
            pieces.append(("n=%d" % n, np.ascontiguousarray(np.frombuffer(longest, dtype=np.uint8)[:n]) if n <= len(longest)
                           else np.ascontiguousarray(base[:n])))
            pieces.append(("n=%d random" % n, np.ascontiguousarray(base[100:100 + n])))
        for p in (longest, min(vs.patterns, key=len), vs.patterns[int(rng.integers(len(vs.patterns)))]):
            for depth in range(1, D + 1):
                t = base[:2000 + depth].copy()
                t[2000:] = np.frombuffer(p[:depth], dtype=np.uint8)
                if vs.nocase:
                    t = variants.scramble(t, depth)
                pieces.append(("depth %d of %r" % (depth, p), t))
        for what, t in pieces:
            path = "sparse" if t.size >= 64 else None
            scan_checked(m, o, [t], inits=[0], what=regime + " " + what, text_of=vs.text_of, expect_path=path)
            group = [np.ascontiguousarray(x[:t.size]) for x in others] + [t]
            scan_checked(m, o, group, inits=[2, 0, 1, 0], what=regime + " group " + what, text_of=vs.text_of,
                         expect_path=path)
    finally:
        m.close()
        a.close()
        o.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["helped"]:
        helped_child()
