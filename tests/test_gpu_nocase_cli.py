"""acm_grep -i: over a directory of mixed-case files it prints what acm_grep without -i prints over
folded copies of the files with folded patterns -- except that each -v line quotes the pattern as
written in the pattern file."""
import os

import numpy as np
import pytest

import fixtures
from test_gpu_acm_grep import CLI, run
from test_host_nocase import fold, scramble

pytestmark = pytest.mark.gpu


def inputs(tmp_path, name, sizes):
    pats = fixtures.patterns_of(name)
    mixed, folded = tmp_path / "mixed", tmp_path / "folded"
    mixed.mkdir()
    folded.mkdir()
    for i, n in enumerate(sizes):
        if name.startswith("clamav"):
            t = fixtures.text_for({"kind": "clamav", "n": n, "seed": 70 + i, "n_plant": 80}, pats)
        else:
            rng = np.random.default_rng(i)
            t = np.concatenate([np.frombuffer(pats[k] + b" ", dtype=np.uint8) for k in rng.integers(0, len(pats), n // 8)])
        t = scramble(t, 90 + i)
        (mixed / ("f%d.bin" % i)).write_bytes(t.tobytes())
        (folded / ("f%d.bin" % i)).write_bytes(fold(t).tobytes())
    return str(mixed), str(folded)


def compare(tmp_path, name, hexpat, extra):
    path, hx, max_len = fixtures.set_source(name)
    o = fixtures.oracle_for(name)
    fpath = str(tmp_path / "folded_patterns.txt")
    categorical = any(o.pattern(i)[1] != i for i in range(o.num_patterns))
    with open(fpath, "wb") as f:
        for i in range(o.num_patterns):
            b, iid = o.pattern(i)
            b = fold(b).hex().encode() if hexpat else fold(b)
            f.write((b"%d " % iid if categorical else b"") + b + b"\n")
    mixed, folded = inputs(tmp_path, name, [200000, 70001, 333])
    common = ["-B", "4096", "-D", "0", "-G", "16", "-L", "256", "-w", "2", "-v"] + (["-x"] if hexpat else []) + extra
    if max_len != -1:
        common += ["-m", str(max_len)]
    got, gstats, _ = run(CLI, ["-i", "-f", mixed, "-p", path] + common)
    exp, estats, _ = run(CLI, ["-f", folded, "-p", fpath] + common)
    assert int(gstats["Matches"]) == int(estats["Matches"]) > 0
    assert int(gstats["Automaton states"]) == int(estats["Automaton states"])
    key = lambda h: (os.path.basename(h[2]), int(h[3]), int(h[0]))
    got_k = sorted(got, key=key)
    exp_k = sorted(exp, key=key)
    assert [(os.path.basename(g[2]), g[0], g[3], g[4]) for g in got_k] == \
        [(os.path.basename(e[2]), e[0], e[3], e[4]) for e in exp_k]
    if not hexpat:
        # the quoted pattern is the one written in the pattern file, not its folded form
        written = {}
        for i in range(o.num_patterns):
            b, iid = o.pattern(i)
            written.setdefault(str(iid), set()).add(b.decode("utf-8", errors="replace"))
        assert any(g[1] != g[1].upper() for g in got_k)
        for g in got_k:
            assert g[1] in written[g[0]]
    return got_k


def test_plain_patterns(gpu, tmp_path):
    compare(tmp_path, "tests", False, [])


def test_categorical_patterns_every_pattern(gpu, tmp_path):
    compare(tmp_path, "sentiment", False, ["-A"])


def test_hex_patterns(gpu, tmp_path):
    compare(tmp_path, "clamav2000_m12", True, [])
