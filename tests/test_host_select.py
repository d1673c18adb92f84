"""The select pass without a device: the model of tests/select_model.py against a brute force that looks at every
entry again at every step, hand cases, and what acm_grep says about -o before it touches a device."""
import os
import subprocess

import numpy as np

import select_model as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpu_pattern_matching_amd", "acm_grep")

LENS = [1, 2, 3, 4, 2, 2, 4, 0, 2, 9]
PRE = [0, 0, 1, 0, 2, 0, 0, 0, 0, 3]
POST = [0, 0, 2, 0, 0, 5, 0, 0, 1, 0]


def test_model_against_brute_force():
    rng = np.random.default_rng(1)
    for case in range(400):
        ctx = case % 2 == 1
        pre, post = (PRE, POST) if ctx else ([0] * 10, [0] * 10)
        model = sel.SelectModel(LENS, pre, post)
        n = int(rng.integers(0, 40))
        cells = np.array([-1, 99, 0x7FFFFF00] + list(range(10)), dtype=np.int64)[rng.integers(0, 13, n)]
        offs = np.cumsum(rng.integers(0, 3, n)).astype(np.int64) + int(rng.integers(-4, 6))
        ms = int(rng.integers(-6, 12))
        ep, eo, es, info = model.run(cells, offs, ms)
        pick = sel.brute_force(cells, offs, LENS, pre, post, ms)
        assert ep.tolist() == [int(cells[i]) for i in pick], case
        assert eo.tolist() == [int(offs[i]) for i in pick], case
        s, e, elig, dropped = model.spans(cells, offs, ms)
        assert es.tolist() == [int(s[i]) for i in pick], case
        cursor = int(e[pick[-1]]) + 1 if pick else ms
        assert info == [int(elig.sum()), int(dropped.sum()), cursor, 0 if cursor >= 0 else -1], case
        # what a selection is: in start order, disjoint, and no eligible entry fits in a hole in front of its successor
        assert all(int(s[b]) > int(e[a]) for a, b in zip(pick, pick[1:])), case
        for i in np.flatnonzero(elig):
            if i not in pick:
                assert any(int(s[j]) <= int(e[i]) and int(s[i]) <= int(e[j]) for j in pick), case


def test_hand_cases():
    model = sel.SelectModel(LENS)
    AB, ABC, BC, CD, A, ABCD, AB2 = 1, 2, 4, 5, 0, 3, 8
    # "abcd" with {ab, abc, bc, cd}: four records, one match
    ep, eo, es, info = model.run([AB, ABC, BC, CD], [1, 2, 2, 3])
    assert (ep.tolist(), eo.tolist(), es.tolist(), info) == ([ABC], [2], [0], [4, 0, 3, 0])
    # nested prefixes: the longest at the leftmost start, then the next start behind it
    ep, eo, es, info = model.run([A, AB, ABC, BC, ABCD, CD, A], [10, 11, 12, 12, 13, 13, 14])
    assert (ep.tolist(), eo.tolist(), es.tolist(), info) == ([ABCD, A], [13, 14], [10, 14], [7, 0, 15, 0])
    # duplicates: the first in the input
    for pair in ([AB, AB2], [AB2, AB]):
        ep, eo, es, info = model.run([A] + pair, [10, 11, 11])
        assert (ep.tolist(), eo.tolist(), es.tolist()) == ([pair[0]], [11], [10])
    # min_start: an entry in front of it is no candidate even where it would have won; a negative one
    ep, eo, es, info = model.run([A, AB, ABC, BC, ABCD, CD, A], [10, 11, 12, 12, 13, 13, 14], 11)
    assert (ep.tolist(), eo.tolist(), es.tolist(), info) == ([BC, A], [12, 14], [11, 14], [3, 4, 15, 0])
    ep, eo, es, info = model.run([AB], [-3], -100)
    assert (ep.tolist(), eo.tolist(), es.tolist(), info) == ([AB], [-3], [-4], [1, 0, -2, -1])
    # nothing that takes part
    ep, eo, es, info = model.run([-1, 7, 0x7FFFFF00], [1, 2, 3], -9)
    assert ep.size == 0 and info == [0, 0, -9, -1]
    # contexts: the span reaches pre in front of the pattern and post behind the offset
    model = sel.SelectModel(LENS, PRE, POST)
    ep, eo, es, info = model.run([2, 0, 0, 0], [10, 11, 12, 13])      # abc: [10 - 3 + 1 - 1, 12]
    assert (ep.tolist(), eo.tolist(), es.tolist(), info) == ([2, 0], [10, 13], [7, 13], [4, 0, 14, 0])


def test_planes_helper():
    p, o, s = sel.planes([5, 6, 7], [10, 11, 12], [9, 9, 9], 4, -1, 77)
    assert p.tolist() == [3, 5, 6, 77] and o.tolist() == [3, 10, 11, 77] and s.tolist() == [3, 9, 9, 0]
    p, o, s = sel.planes([], [], [], 3, -1, 77)
    assert p.tolist() == [0, 77, -1] and s.tolist() == [0, 0, -1]


def test_usage_names_select():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "  -o   " in r.stdout and "leftmost-longest" in r.stdout and "tvxFMAiSWcno" in r.stdout


def test_refused_combinations(tmp_path):
    """every refused combination is a usage error: its ERROR: line, the usage text and a failure, no device needed"""
    pats = tmp_path / "p.txt"
    pats.write_text("ab\nabc\n")
    sigs = tmp_path / "s.txt"
    sigs.write_text("6162*6364\n")
    rules = tmp_path / "r.ldb"
    rules.write_text("0;6162\n")
    data = tmp_path / "d.txt"
    data.write_text("abcd\n")
    base = [CLI, "-f", str(data), "-p", str(pats), "-B", "64", "-D", "0", "-G", "16", "-L", "64", "-o"]
    for extra in (["-A"], ["-c"], ["-n"], ["-Q", str(sigs)], ["-K", str(rules), "-S"], ["-Q", str(sigs), "-E"], ["-F"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, extra
        assert "ERROR: -o cannot be combined with -A, -c, -n, -Q, -K, -E or -F" in r.stdout, extra
        assert "Usage:" in r.stdout, extra
