"""Whole-word matching on the host, no GPU needed: the word-boundary model the GPU tests compare with,
checked against brute force, its streaming contract, and the native workspace query.

The model (tests/word_model.py) keeps the entries of the oracle's all-patterns scan whose bytes
outside the match are not word bytes; brute force finds every occurrence of every pattern with
bytes.find and applies the same rule.  The two must agree on every set, nocase included, for the
default, empty, full and a custom word set.
"""
import numpy as np
import pytest

import word_model as wm

SETS = ["tests", "clamav2000_m12", "sentiment"]
WORD_SETS = {"default": wm.DEFAULT, "empty": wm.EMPTY, "full": wm.FULL, "custom": wm.CUSTOM}


def text_for(name, model, n, seed):
    if name.startswith("clamav"):
        return wm.planted_text(model.pats, n, seed, max_len=12)
    return wm.planted_text(model.pats, n, seed)


@pytest.mark.parametrize("nocase", [False, True], ids=["case", "nocase"])
@pytest.mark.parametrize("name", SETS)
def test_model_matches_brute_force(name, nocase):
    m = wm.WordModel(name, nocase)
    n = 1500 if name == "tests" else 2500
    for seed in range(2):
        t = text_for(name, m, n, seed)
        if nocase:
            t = t.copy()
            t[::3] = np.where((t[::3] >= ord("a")) & (t[::3] <= ord("z")), t[::3] - 32, t[::3])
        for wname, ws in WORD_SETS.items():
            offs, pats, _ = m.words(t, ws, all_patterns=True)
            got = set(zip(offs.tolist(), pats.tolist()))
            exp = wm.brute_force(m.pats, t, ws, nocase)
            assert got == exp, "%s %s: model %d entries, brute force %d" % (name, wname, len(got), len(exp))
            assert len(got) == offs.size, "an entry reported twice"
            assert np.all(np.diff(offs.astype(np.int64)) >= 0), "offsets not ascending"
            h_off, h_pat, _ = m.words(t, ws, all_patterns=False)
            # head: one record per offset that has a bounded entry, the first of them in list order
            assert np.array_equal(h_off, np.unique(offs)), wname
            for o, p in zip(h_off.tolist(), h_pat.tolist()):
                assert p == int(pats[np.nonzero(offs == o)[0][0]])


@pytest.mark.parametrize("name", SETS)
def test_empty_set_is_the_plain_scan(name):
    """with an empty W every pattern (length >= 1) passes: head = the scan's head records, all = scan_all"""
    m = wm.WordModel(name)
    t = text_for(name, m, 2000, 5)
    offs, pats, last = m.scan_all(t)
    a = m.words(t, wm.EMPTY, all_patterns=True)
    assert np.array_equal(a[0], offs) and np.array_equal(a[1], pats) and a[2] == last
    h = m.words(t, wm.EMPTY)
    ho, hp, hl = m.o.scan(t)
    assert np.array_equal(h[0], ho) and np.array_equal(h[1], hp) and h[2] == hl


@pytest.mark.parametrize("all_patterns", [False, True], ids=["head", "all"])
@pytest.mark.parametrize("name", ["tests", "sentiment"])
def test_streaming_splits(name, all_patterns):
    """a text cut in two, the second piece given max_pattern_len bytes in front of it and the first
    piece the byte after it, gives the one-shot records at every cut near planted words"""
    m = wm.WordModel(name)
    t = text_for(name, m, 400, 11)
    one = m.words(t, all_patterns=all_patterns)
    for c in list(range(0, 40)) + list(range(len(t) // 2 - 20, len(t) // 2 + 20)) + [len(t) - 1, len(t)]:
        a = m.words(t[:c], all_patterns=all_patterns, next_byte=int(t[c]) if c < len(t) else -1)
        before = bytes(t[max(0, c - m.max_len):c])
        b = m.words(t[c:], all_patterns=all_patterns, init_state=a[2], before=before)
        offs = np.concatenate([a[0].astype(np.int64), b[0].astype(np.int64) + c]).astype(np.uint32)
        pats = np.concatenate([a[1], b[1]]).astype(np.int32)
        assert np.array_equal(offs, one[0]) and np.array_equal(pats, one[1]), "cut at %d" % c
        assert b[2] == one[2]


def test_segments_are_text_boundaries():
    """a segment start is a text start and the end of the text in front of it"""
    m = wm.WordModel("tests")
    p = m.pats[0]
    t = np.frombuffer(b"x" + p + p + b"y", dtype=np.uint8)
    L = len(p)
    starts = [0, 1, 1 + L, 1 + 2 * L]
    offs, pats, _ = m.words(t, all_patterns=True, starts=starts)
    assert {(L, 0), (2 * L, 0)} <= set(zip(offs.tolist(), pats.tolist()))
    offs, pats, _ = m.words(t, all_patterns=True)
    assert (L, 0) not in set(zip(offs.tolist(), pats.tolist()))


def test_word_workspace_bytes_exported_and_monotone(lib):
    assert hasattr(lib, "acm_word_workspace_bytes") and hasattr(lib, "acm_word_matches_async")
    prev = 0
    for n in [0, 1, 1023, 1024, 1025, 1 << 16, 1 << 20, 1 << 24, 1 << 28]:
        b = lib.acm_word_workspace_bytes(n)
        assert b >= prev and b >= 4 and b % 256 == 0, (n, b)
        prev = b
