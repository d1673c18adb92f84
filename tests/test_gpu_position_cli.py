"""acm_grep -P: a position file for the patterns of -p (then those of -I), with -S every file its own text.
The printed matches and the -c counts are those of the position model (tests/position_model.py) over the
worker's files; a file that spans two buffers is exact for windows counted from its start and an error,
never a silent loss, for candidates counted from its end."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import position_model as pm
from test_gpu_acm_grep import CLI

pytestmark = pytest.mark.gpu

EXACT = [b"Needle", b"abc", b"HEAD", b"tail", b"abcd", b"abc"]
LOOSE = [b"NeedLe", b"Tail"]
WINDOWS = {1: (2, 40, False), 2: (0, 0, False), 3: (4, 4, True), 4: (5, 60, True), 5: (100, None, False), 7: (4, 9, True)}
START_ONLY = {i: w for i, w in WINDOWS.items() if not w[2]}
B, G = 64, 16                 # buffers of 1024 bytes

LINE = re.compile(r"^Pattern (-?\d+) \('(.*)'\) found in file '(.*)' at (?:line (\d+) )?offset (\d+) \[relative: (-?\d+)\]$")
FILE_LINE = re.compile(r"^Count file '(.*)': (\d+)$", re.M)
PAT_LINE = re.compile(r"^Count pattern (-?\d+) \('(.*)'\): (\d+)$", re.M)


def run(args, ok=True):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120, errors="replace")
    if ok:
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = [m.groups() for m in (LINE.match(l) for l in p.stdout.splitlines()) if m]
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p


def write_files(tmp_path, windows):
    e, l, w = tmp_path / "exact.txt", tmp_path / "loose.txt", tmp_path / "windows.pos"
    e.write_bytes(b"".join(p + b"\n" for p in EXACT))
    l.write_bytes(b"".join(p + b"\n" for p in LOOSE))
    lines = ["# index lo hi [end]"]
    for i, (lo, hi, fe) in sorted(windows.items()):
        lines.append("%d %d %s%s" % (i, lo, "*" if hi is None else hi, " end" if fe else ""))
    w.write_text("\n".join(lines) + "\n\n")
    return str(e), str(l), str(w)


def make_text(seed, size):
    """about size bytes: the patterns in either case between word bytes and others, one at each end"""
    rng = np.random.default_rng(seed)
    glue = [b"", b" ", b". ", b"_", b"x", b"\n", b"  "]
    src = EXACT + LOOSE + [b"NEEDLE", b"TAIL", b"Abc"]
    t = bytearray(b"HEAD" if seed % 2 else b"abcd")
    while len(t) < size:
        t += glue[int(rng.integers(len(glue)))] + src[int(rng.integers(len(src)))]
    t += b" tail" if seed % 3 else b"_Tail"
    return bytes(t)


def inputs(tmp_path, sizes):
    d = tmp_path / "in"
    d.mkdir()
    for i, (seed, size) in enumerate(sizes):
        (d / ("p%d.txt" % i)).write_bytes(make_text(seed, size))
    order = [os.path.join(str(d), e) for e in os.listdir(str(d))]    # readdir order, as acm_grep walks it
    return str(d), [(f, open(f, "rb").read()) for f in order]


def expected(pats, windows, files, all_patterns, then=None):
    """(file, pattern bytes, position in the file) of every record: each file its own text"""
    model = pm.PositionModel(pats, windows)
    texts = [t for _, t in files]
    bounds = np.cumsum([0] + [len(t) for t in texts])
    offs, idx, _, und = model.records(texts, all_patterns, then=then)
    assert und == 0
    k = np.searchsorted(bounds, offs.astype(np.int64), side="right") - 1
    names = [p[0] if isinstance(p, tuple) else p for p in pats]
    return [(os.path.basename(files[f][0]), names[p].decode(), o - int(bounds[f])) for o, p, f in
            zip(offs.tolist(), idx.tolist(), k.tolist())]


def base_args(path, exact, pos):
    return ["-f", path, "-p", exact, "-P", pos, "-S", "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", "1", "-R", "128",
            "-v"]


def same_hits(hits, exp):
    got = sorted((os.path.basename(h[2]), h[1], int(h[5]) - 1) for h in hits)
    assert got == sorted((f, p, pos % B) for f, p, pos in exp)


@pytest.mark.parametrize("all_patterns", [False, True], ids=["first", "-A"])
def test_small_files(gpu, tmp_path, all_patterns):
    exact, _, pos = write_files(tmp_path, {i: w for i, w in WINDOWS.items() if i < len(EXACT)})
    path, files = inputs(tmp_path, [(1, 150), (2, 260), (3, 0), (4, 330)])
    windows = {i: w for i, w in WINDOWS.items() if i < len(EXACT)}
    exp = expected(EXACT, windows, files, all_patterns)
    free = expected(EXACT, {}, files, all_patterns)
    assert 10 < len(exp) < len(free)
    kept = {e[1] for e in exp}
    assert {"HEAD", "tail", "abcd", "Needle"} <= kept
    args = base_args(path, exact, pos) + (["-A"] if all_patterns else [])
    hits, stats, _ = run(args)
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    same_hits(hits, exp)
    # without the windows there are more
    _, s2, _ = run([a for a in args if a not in ("-P", pos)])
    assert int(s2["Matches"]) == len(free)
    # -c: counts tallied on the device from the pass's output
    hits, stats, p = run(args + ["-c"])
    same_hits(hits, exp)
    per_file = collections.Counter(e[0] for e in exp)
    assert {os.path.basename(f): int(n) for f, n in FILE_LINE.findall(p.stdout)} == \
        {os.path.basename(f): per_file[os.path.basename(f)] for f, _ in files}
    per_pat = collections.Counter()
    for _, name, _ in exp:
        per_pat[name] += 1
    assert {name: sum(int(n) for _, q, n in PAT_LINE.findall(p.stdout) if q == name) for name in per_pat} == dict(per_pat)


def test_file_across_buffers(gpu, tmp_path):
    d = tmp_path / "one"
    d.mkdir()
    text = make_text(5, 1500)
    assert 1024 < len(text) < 2048 and b"tail" in text[:1000]
    f = d / "long.txt"
    f.write_bytes(text)
    files = [(str(f), text)]
    # windows counted from the start: exact, whichever buffer the match lies in
    exact, _, pos = write_files(tmp_path, START_ONLY)
    exp = expected(EXACT, {i: w for i, w in START_ONLY.items() if i < len(EXACT)}, files, True)
    assert any(name == "abc" and at > 1024 for _, name, at in exp)         # pattern 5: 100 bytes or more into the file
    hits, stats, p = run(base_args(str(f), exact, pos) + ["-A"])
    assert int(stats["Kernel launches"]) == 2 and "ERROR" not in p.stdout
    assert int(stats["Matches"]) == len(exp)
    same_hits(hits, exp)
    # a window counted from the end: the candidates in the first buffer cannot be decided
    exact, _, pos = write_files(tmp_path, {i: w for i, w in WINDOWS.items() if i < len(EXACT)})
    hits, stats, p = run(base_args(str(f), exact, pos) + ["-A"], ok=False)
    assert p.returncode != 0
    m = re.search(r"^ERROR: (\d+) end-anchored candidates lie in files that span buffers \(raise -B/-G\)$", p.stdout, re.M)
    model = pm.PositionModel(EXACT, {})
    o, q, _, _ = model.records([text], True)
    lost = sum(1 for x, y in zip(o.tolist(), q.tolist()) if x < 1024 and WINDOWS.get(y, (0, 0, False))[2])
    assert m and int(m.group(1)) == lost > 0
    # with buffers that hold the file it is exact again
    exp = expected(EXACT, {i: w for i, w in WINDOWS.items() if i < len(EXACT)}, files, True)
    args = [a for a in base_args(str(f), exact, pos)]
    args[args.index("-G") + 1] = "32"
    hits, stats, p = run(args + ["-A"])
    assert int(stats["Matches"]) == len(exp)
    same_hits(hits, exp)


def test_refused_without_segments_or_with_follow(gpu, tmp_path):
    exact, loose, pos = write_files(tmp_path, WINDOWS)
    f = str(tmp_path / "x.txt")
    open(f, "wb").write(b"abc\n")
    common = ["-f", f, "-p", exact, "-P", pos, "-B", "64", "-D", "0", "-G", "16", "-L", "64"]
    r = subprocess.run([CLI] + common, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "ERROR: -P needs -S" in r.stdout
    r = subprocess.run([CLI] + common + ["-S", "-F"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "ERROR: -P cannot be combined with -F" in r.stdout
    r = subprocess.run([CLI] + common + ["-S", "-W", "-I", loose], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-I cannot be combined with -W or -F: the case pass and those are not composed" in r.stdout
    bad = tmp_path / "bad.pos"
    bad.write_text("0 0 0\n9 0 0\n")
    r = subprocess.run([CLI] + [str(bad) if a == pos else a for a in common] + ["-S"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "bad.pos:2:" in r.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-P file" in r.stdout


@pytest.mark.parametrize("all_patterns", [False, True], ids=["first", "-A"])
@pytest.mark.parametrize("then", ["words", "case"])
def test_composed_with_words_and_case(gpu, tmp_path, then, all_patterns):
    path, files = inputs(tmp_path, [(7, 200), (8, 300), (9, 280)])
    if then == "words":
        pats = EXACT
        windows = {i: w for i, w in WINDOWS.items() if i < len(EXACT)}
        exact, _, pos = write_files(tmp_path, windows)
        extra = ["-W"]
    else:
        pats = [(p, False) for p in EXACT] + [(p, True) for p in LOOSE]
        windows = WINDOWS
        exact, loose, pos = write_files(tmp_path, windows)
        extra = ["-I", loose]
    exp = expected(pats, windows, files, all_patterns, then=then)
    assert 5 < len(exp) < len(expected(pats, {}, files, all_patterns, then=then))
    assert len(exp) < len(expected(pats, windows, files, True))
    hits, stats, _ = run(base_args(path, exact, pos) + extra + (["-A"] if all_patterns else []))
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    same_hits(hits, exp)
