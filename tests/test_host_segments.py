"""Segmented scans on the host, no GPU needed: the fail/depth accessors and the clamp rule.

The rule (acm_segment_matches_async): the state a walk restarted at a segment's start would be in after
byte p is the first state on the fail chain of the serial walk's state whose depth is <= the bytes of
the segment up to p.  Here the serial walk runs in Python over Automaton.reference_table(), its
records are clamped with acm_automaton_state_fail / _depth, and the result must equal the oracle
scanning every segment on its own from state 0.
"""
import os

import numpy as np
import pytest

import fixtures
import orc
from gpu_pattern_matching_amd import AcmError, Automaton

SETS = ["tests", "clamav2000_m12", "sentiment"]


def product(name, nocase=False):
    path, hx, max_len = fixtures.set_source(name)
    a = Automaton(nocase=nocase)
    a.load_file(path, hx, max_len)
    return a.compile()


def text_of(name, n, seed):
    pats = fixtures.patterns_of(name)
    if name.startswith("clamav"):
        return fixtures.text_for({"kind": "clamav", "n": n, "seed": seed, "n_plant": max(4, n // 256)}, pats)
    if name == "sentiment":
        return fixtures.text_for({"kind": "words", "n": n, "seed": seed}, pats)
    t = np.fromfile(os.path.join(orc.DATA, "ref_tests", "input.txt"), dtype=np.uint8)
    return np.tile(t, n // max(t.size, 1) + 1)[:n]


def oracle_segments(o, text, starts, init_state=0, all_patterns=False):
    """Ground truth: every segment scanned alone from state 0 (the bytes in front of the first start
    continue from init_state, segment -1).  Returns (offsets, patterns, segment ids, per-segment counts,
    final state)."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    starts = np.asarray(starts, dtype=np.int64)
    scan = o.scan_all if all_patterns else o.scan
    bounds = [0] + [int(min(max(s, 0), text.size)) for s in starts] + [text.size]
    offs, pats, segs = [], [], []
    counts = np.zeros(starts.size, dtype=np.int32)
    state = init_state
    for k in range(-1, starts.size):
        lo, hi = bounds[k + 1], bounds[k + 2]
        if k >= 0:
            state = 0
        if hi < lo:
            hi = lo
        p, q, state = scan(text[lo:hi], state)
        offs.append(p.astype(np.int64) + lo)
        pats.append(q)
        segs.append(np.full(p.size, k, dtype=np.int32))
        if k >= 0:
            counts[k] = p.size
    return (np.concatenate(offs).astype(np.uint32), np.concatenate(pats).astype(np.int32),
            np.concatenate(segs), counts, state)


class Tables:
    """per-state fail, depth, head and finality of a product automaton, read through the accessors"""

    def __init__(self, a):
        n = a.num_states
        self.table = a.reference_table()
        self.fail = np.array([a.state_fail(s) for s in range(n)], dtype=np.int64)
        self.depth = np.array([a.state_depth(s) for s in range(n)], dtype=np.int64)
        self.head = np.array([a.state_output(s) for s in range(n)], dtype=np.int64)
        self.final = np.array([s != 0 and len(a.state_matches(s)) > 0 for s in range(n)])

    def walk_states(self, text, s=0):
        """STATE records of the serial walk: (positions, states), final state"""
        pos, st = [], []
        t = self.table
        for x, c in enumerate(np.asarray(text, dtype=np.uint8).tolist()):
            v = int(t[s, 0, c])
            if v < 0:
                v = -v
                pos.append(x)
                st.append(v)
            s = v
        return np.array(pos, dtype=np.int64), np.array(st, dtype=np.int64), s

    def clamp(self, s, b):
        while self.depth[s] > b:
            s = int(self.fail[s])
        return s

    def segmented(self, text, starts, init_state=0):
        """the segment pass in Python: (offsets, heads, segment ids, final state)"""
        starts = np.asarray(starts, dtype=np.int64)
        pos, st, last = self.walk_states(text, init_state)
        offs, heads, segs = [], [], []
        for p, s in zip(pos.tolist(), st.tolist()):
            k = int(np.searchsorted(starts, p, side="right")) - 1
            if k >= 0:
                s = self.clamp(s, p - int(starts[k]) + 1)
            if not self.final[s]:
                continue
            offs.append(p)
            heads.append(int(self.head[s]))
            segs.append(k)
        k = int(np.searchsorted(starts, len(text), side="right")) - 1
        if k >= 0:
            last = self.clamp(last, len(text) - int(starts[k]))
        return (np.array(offs, dtype=np.uint32), np.array(heads, dtype=np.int32), np.array(segs, dtype=np.int32),
                last)


def random_starts(n, rng, max_len):
    """segment starts over n bytes: sizes 0, 1, shorter than the longest pattern and longer, a start at 0"""
    starts, x = [0], 0
    while x < n:
        r = rng.random()
        if r < 0.1:
            size = 0
        elif r < 0.2:
            size = 1
        elif r < 0.6:
            size = int(rng.integers(1, max(2, max_len)))
        else:
            size = int(rng.integers(max_len, 4 * max_len + 2))
        x += size
        if x < n:
            starts.append(x)
    return np.array(starts, dtype=np.int32)


def assert_same(got, exp):
    assert got[0].size == exp[0].size, "record count %d != %d" % (got[0].size, exp[0].size)
    assert np.array_equal(got[0], exp[0]), "offsets differ"
    assert np.array_equal(got[1], exp[1]), "pattern indices differ"
    assert np.array_equal(got[2], exp[2]), "segment ids differ"
    assert got[3] == exp[3], "final state %d != %d" % (got[3], exp[3])


@pytest.mark.parametrize("name", SETS + ["nocase:sentiment"])
def test_accessors(lib, name):
    nocase = name.startswith("nocase:")
    a = product(name.split(":")[-1], nocase=nocase)
    assert a.state_depth(0) == 0
    assert a.state_fail(0) == 0
    n = a.num_states
    for s in range(1, n, max(1, n // 3000)):
        f = a.state_fail(s)
        assert 0 <= f < n
        assert a.state_depth(f) < a.state_depth(s)
        assert a.state_depth(s) <= a.max_pattern_len
    for bad in (-1, n):
        with pytest.raises(AcmError):
            a.state_fail(bad)
        with pytest.raises(AcmError):
            a.state_depth(bad)


def test_accessors_need_a_compiled_automaton(lib):
    a = Automaton()
    a.add(b"abc")
    with pytest.raises(AcmError):
        a.state_fail(0)
    with pytest.raises(AcmError):
        a.state_depth(0)


@pytest.mark.parametrize("name", SETS + ["nocase:sentiment"])
def test_clamp_rule_matches_per_segment_scans(lib, name):
    nocase = name.startswith("nocase:")
    base = name.split(":")[-1]
    a = product(base, nocase=nocase)
    tb = Tables(a)
    o = fixtures.oracle_for(base)
    if nocase:
        from test_host_nocase import fold, folded_oracle
        o = folded_oracle(base)
    rng = np.random.default_rng(7)
    for seed in range(3):
        text = text_of(base, 3000, 40 + seed)
        if nocase:
            from test_host_nocase import scramble
            text = scramble(text, seed)
        starts = random_starts(text.size, rng, a.max_pattern_len)
        got = tb.segmented(text, starts)
        exp = oracle_segments(o, fold(text) if nocase else text, starts)
        assert_same(got, (exp[0], exp[1], exp[2], exp[4]))


@pytest.mark.parametrize("name", ["tests", "clamav2000_m12"])
def test_segment_shapes(lib, name):
    a = product(name)
    tb = Tables(a)
    o = fixtures.oracle_for(name)
    text = text_of(name, 700, 3)
    shapes = {
        "one per byte": np.arange(text.size, dtype=np.int32),
        "one segment": np.array([0], dtype=np.int32),
        "late first start": np.array([100, 100, 101, 350], dtype=np.int32),
        "starts at and past the end": np.array([0, 600, text.size, text.size, text.size + 5], dtype=np.int32),
        "empty runs": np.repeat(np.arange(0, text.size, 37, dtype=np.int32), 3),
    }
    for what, starts in shapes.items():
        got = tb.segmented(text, starts)
        exp = oracle_segments(o, text, starts)
        assert_same(got, (exp[0], exp[1], exp[2], exp[4]))
    # carried state: a text that began in a previous scan continues up to the first start
    _, _, mid = o.scan(text[:300])
    starts = np.array([50, 400], dtype=np.int32)
    got = tb.segmented(text[300:], starts, init_state=mid)
    exp = oracle_segments(o, text[300:], starts, init_state=mid)
    assert_same(got, (exp[0], exp[1], exp[2], exp[4]))


def test_clamping_changes_the_head(lib):
    # list(abcd) = [bcd, cd, abcd]: the serial scan reports bcd at the d; with a text starting at the c
    # only cd lies inside it
    a = Automaton()
    for p in (b"abcd", b"bcd", b"cd"):
        a.add(p)
    a.compile()
    tb = Tables(a)
    text = np.frombuffer(b"xxabcdxx", dtype=np.uint8)
    plain = tb.segmented(text, [])
    assert plain[0].tolist() == [5] and plain[1].tolist() == [1]
    got = tb.segmented(text, [0, 4])   # boundary between b and c
    assert got[0].tolist() == [5] and got[1].tolist() == [2] and got[2].tolist() == [1]
    got = tb.segmented(text, [0, 5])   # boundary between c and d: nothing left
    assert got[0].size == 0
