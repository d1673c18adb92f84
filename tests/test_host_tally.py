"""Match tallies on the host, no GPU needed: the numpy model the GPU tests compare with, checked against
a brute-force count; api.class_map and Automaton.iids; the exported symbols and the workspace query; the
CLI's usage text."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import word_model as wm
from gpu_pattern_matching_amd import Automaton, _lib, api
from tally_model import tally

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpu_pattern_matching_amd", "acm_grep")


def brute_entries(pats, text, starts=None):
    """every (end offset, pattern) pair found with bytes.find; with starts only occurrences that lie
    inside one segment (or wholly in front of the first start)"""
    t = bytes(np.ascontiguousarray(text, dtype=np.uint8))
    st = np.asarray(starts if starts is not None else [], dtype=np.int64)
    out = []
    for i, p in enumerate(pats):
        if not p:
            continue
        k = t.find(p)
        while k >= 0:
            o = k + len(p) - 1
            if st.size == 0 or np.searchsorted(st, k, side="right") == np.searchsorted(st, o, side="right"):
                out.append((o, i))
            k = t.find(p, k + 1)
    return out


@pytest.mark.parametrize("name", ["tests", "sentiment"])
@pytest.mark.parametrize("segmented", [False, True], ids=["whole", "segments"])
def test_model_matches_brute_force(name, segmented):
    m = wm.WordModel(name)
    t = wm.planted_text(m.pats, 3000, 4)
    starts = np.array([0, 0, 17, 140, 141, 900, 2999, 5000], dtype=np.int64) if segmented else None
    offs, pats, _ = m.scan_all(t, starts=starts)
    brute = brute_entries(m.pats, t, starts)
    assert len(brute) == offs.size > 100
    iids = np.array([iid for _, iid in m.o.patterns()], dtype=np.int64)
    for class_of, C in ((None, len(m.pats)), (api.class_map(np.sign(iids))[1], 2), (np.zeros(len(m.pats), np.int32), 1)):
        total, rows, lead = tally(offs, pats, class_of, C, starts)
        exp_total = np.zeros(C, dtype=np.uint64)
        exp_rows = np.zeros((len(starts) if segmented else 0, C), dtype=np.int32)
        for o, p in brute:
            c = p if class_of is None else int(class_of[p])
            if not 0 <= c < C:
                continue
            exp_total[c] += 1
            if segmented:
                exp_rows[np.searchsorted(starts, o, side="right") - 1, c] += 1
        assert np.array_equal(total, exp_total)
        assert not lead.any()   # start[0] == 0: nothing lies in front of it
        if segmented:
            assert np.array_equal(rows, exp_rows) and rows.dtype == np.int32
            assert int(rows.sum()) == int(total.sum())
        else:
            assert rows is None


def test_model_lead_and_dropped_classes():
    offs = np.array([1, 5, 5, 9, 30])
    pats = np.array([0, 1, 2, 0, 3])
    class_of = np.array([1, -1, 0, 7])
    total, rows, lead = tally(offs, pats, class_of, 2, [5, 5, 10])
    assert total.tolist() == [1, 2] and total.dtype == np.uint64
    assert lead.tolist() == [0, 1]
    assert rows.tolist() == [[0, 0], [1, 1], [0, 0]]


def test_class_map():
    vals = np.array([5, -3, 5, 0, -3, 9])
    labels, class_of = api.class_map(vals)
    assert labels.tolist() == [-3, 0, 5, 9]
    assert class_of.dtype == np.int32 and class_of.tolist() == [2, 0, 2, 1, 0, 3]
    assert np.array_equal(labels[class_of], vals)


def test_iids(lib):
    path, hx, max_len = fixtures.set_source("sentiment")
    a = Automaton()
    a.load_file(path, hx, max_len)
    a.compile()
    ids = a.iids()
    assert ids.dtype == np.int32 and ids.size == a.num_patterns
    assert ids.tolist() == [a.pattern(i)[1] for i in range(a.num_patterns)]
    labels, class_of = api.class_map(np.sign(ids))
    assert labels.tolist() == [-1, 1]
    assert np.bincount(class_of).tolist() == [2955, 1421]
    a.close()


def test_symbols_and_workspace_query(lib):
    assert hasattr(lib, "acm_tally_matches_async") and hasattr(lib, "acm_tally_workspace_bytes")
    assert "acm_tally_matches_async" in _lib.NATIVE_API
    prev = 0
    for n in (0, 1, 1024, 1 << 20, 1 << 25, (1 << 31) - 2):
        row = 0
        for c in (1, 2, 4376, 5632, 5633, 1 << 20, (1 << 31) - 1):
            b = lib.acm_tally_workspace_bytes(n, c)
            assert b > 0 and b % 256 == 0 and b >= row and b >= prev
            row = b
        prev = lib.acm_tally_workspace_bytes(n, 1)


def test_usage_names_count(lib):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-c " in r.stdout and "Count file" in r.stdout
