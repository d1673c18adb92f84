"""acm_grep -W: whole words only.  A worker's files are one stream (with -S every file, with -t -S every
line, is its own text); the matches are those of the word model (tests/word_model.py) over that stream,
with buffers and chunks small enough that words straddle buffers and files."""
import collections
import os
import subprocess

import numpy as np
import pytest

import fixtures
import word_model as wm
from test_gpu_acm_grep import CLI, run

pytestmark = pytest.mark.gpu


def write_files(tmp_path, model, nocase, seed, sizes=(9000, 7001, 12345)):
    files = []
    for i, n in enumerate(sizes):
        t = wm.planted_text(model.pats, n, seed + i)
        if nocase:
            t = t.copy()
            up = (t >= ord("a")) & (t <= ord("z")) & (np.arange(t.size) % 3 == 0)
            t[up] -= 32
        p = str(tmp_path / ("w%d.txt" % i))
        open(p, "wb").write(t.tobytes())
        files.append((p, t))
    return files


def expected(model, files, all_patterns, segmented, text_mode):
    """(file, pattern, position in the file) of every record the model reports over the worker's stream"""
    stream = np.concatenate([t for _, t in files])
    bounds = np.cumsum([0] + [t.size for _, t in files])
    starts = None
    if segmented:
        s = set(bounds[:-1].tolist())
        if text_mode:
            s |= set((np.flatnonzero(stream == ord("\n")) + 1).tolist())
        starts = np.array(sorted(x for x in s if x < stream.size), dtype=np.int64)
    offs, pats, _ = model.words(stream, wm.DEFAULT, all_patterns, starts=starts)
    f = np.searchsorted(bounds, offs.astype(np.int64), side="right") - 1
    return [(os.path.basename(files[k][0]), model.pats[p].decode(), int(o) - int(bounds[k]))
            for o, p, k in zip(offs.tolist(), pats.tolist(), f.tolist())]


CASES = [  # (text mode, -A, -S, nocase)
    (False, False, False, False),
    (False, True, False, False),
    (False, False, True, False),
    (False, True, True, False),
    (False, False, False, True),
    (True, False, False, False),
    (True, True, False, False),
    (True, False, True, False),
    (True, False, False, True),
]


@pytest.mark.parametrize("text_mode,all_patterns,segmented,nocase", CASES,
                         ids=["-".join(n for n, v in zip(("t", "A", "S", "i"), c) if v) or "binary" for c in CASES])
def test_words(gpu, tmp_path, text_mode, all_patterns, segmented, nocase):
    name = "sentiment"
    model = wm.WordModel(name, nocase)
    path, _, _ = fixtures.set_source(name)
    files = write_files(tmp_path, model, nocase, 3)
    B = 256 if text_mode else 64
    args = ["-f", ",".join(p for p, _ in files), "-p", path, "-B", str(B), "-D", "0", "-G", "16", "-L", "64",
            "-w", "1", "-R", "64", "-v", "-W"]
    args += (["-t"] if text_mode else []) + (["-A"] if all_patterns else []) + (["-S"] if segmented else []) + \
        (["-i"] if nocase else [])
    exp = expected(model, files, all_patterns, segmented, text_mode)
    hits, stats, _ = run(CLI, args)
    assert int(stats["Kernel launches"]) > 20   # many buffers: words straddle them, and the files
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    plain, pstats, _ = run(CLI, [a for a in args if a != "-W"])
    assert int(pstats["Matches"]) > len(exp)     # the plain scan reports sub-word hits as well
    if text_mode:
        # chunks are lines, or pieces of a line at a buffer's end; a -v line after such a piece is printed
        # behind it and does not parse, so the parsed hits are a part of the expected ones
        got = collections.Counter((os.path.basename(h[2]), h[1]) for h in hits)
        want = collections.Counter((e[0], e[1]) for e in exp)
        assert sum(got.values()) > len(exp) // 2 and not got - want
    else:
        # relative offset - 1 = the match's last byte in its chunk, the B bytes of its file at a multiple of B
        got = sorted((os.path.basename(h[2]), h[1], int(h[4]) - 1) for h in hits)
        assert got == sorted((f, p, pos % B) for f, p, pos in exp)


def test_words_rejected_with_follow(gpu, tmp_path):
    path, _, _ = fixtures.set_source("sentiment")
    p = str(tmp_path / "x.txt")
    open(p, "wb").write(b"died\n")
    r = subprocess.run([CLI, "-f", p, "-p", path, "-B", "64", "-D", "0", "-G", "16", "-L", "64", "-W", "-F"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "-W cannot be combined with -F" in r.stdout + r.stderr
