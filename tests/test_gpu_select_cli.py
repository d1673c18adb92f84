"""acm_grep -o: the leftmost-longest non-overlapping matches, selected on the device per buffer.  A worker's files
are one stream (with -S every file is its own text) cut into buffers of G chunks; the printed matches are those of
the model (tests/select_model.py) over the occurrences bytes.find gives, buffer by buffer, and the entries that
began in the buffer in front are what the NOTE on stderr counts."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import select_model as sel
from test_gpu_acm_grep import CLI

pytestmark = pytest.mark.gpu

PATS = [b"a", b"ab", b"abc", b"bc", b"bcd", b"cd", b"dddd", b"Needle", b"ab-cd", b"cd-a"]   # (whole words overlap only over a "-")
TOKENS = [b"abcd", b"ab", b"bcd", b"a", b"dddd", b"ABC", b"abcab", b"cd", b" ", b" ", b"\n", b"x", b"Needle", b"needle", b"_",
          b"ab-cd", b"ab-cd-a", b"-"]
B = 64
WORD = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")

LINE = re.compile(r"^Pattern (-?\d+) \('(.*)'\) found in file '(.*)' at offset (\d+) \[relative: (-?\d+)\]$")


def run(args):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120, errors="replace")
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = [m.groups() for m in (LINE.match(l) for l in p.stdout.splitlines()) if m]
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p


def make_file(seed, size):
    rng = np.random.default_rng(seed)
    out = b""
    while len(out) < size:
        out += TOKENS[int(rng.integers(len(TOKENS)))] + (b" " if rng.random() < 0.5 else b"")   # (words, for -W)
    return out[:size]


def write_inputs(tmp_path, sizes):
    d = tmp_path / "in"
    d.mkdir()
    per_file = {}
    for i, (seed, size) in enumerate(sizes):
        per_file[str(d / ("s%d.txt" % i))] = make_file(seed, size)
        (d / ("s%d.txt" % i)).write_bytes(per_file[str(d / ("s%d.txt" % i))])
    order = [os.path.join(str(d), e) for e in os.listdir(str(d))]    # readdir order, as acm_grep walks it
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"".join(p + b"\n" for p in PATS))
    return str(d), str(pats), [(f, per_file[f]) for f in order]


def entries(texts, nocase, words):
    """(pattern, end in the stream) of every occurrence, each text alone, ordered by end"""
    out, base = [], 0
    for t in texts:
        hay = t.upper() if nocase else t
        for i, p in enumerate(PATS):
            needle = p.upper() if nocase else p
            k = hay.find(needle)
            while k >= 0:
                e = k + len(p) - 1
                if not words or ((k == 0 or t[k - 1] not in WORD) and (e + 1 == len(t) or t[e + 1] not in WORD)):
                    out.append((base + e, i))
                k = hay.find(needle, k + 1)
        base += len(t)
    out.sort()
    return np.array([c for _, c in out], dtype=np.int64), np.array([o for o, _ in out], dtype=np.int64)


def expected(files, G, segmented=False, nocase=False, words=False):
    """(sorted (file, pattern bytes, position in its file modulo B) of every selected match, entries dropped at the
    front of a buffer): the model over every buffer of G chunks of the worker's stream"""
    texts = [t for _, t in files]
    bounds = np.cumsum([0] + [len(t) for t in texts])
    chunk_starts = [int(bounds[f]) + k for f, t in enumerate(texts) for k in range(0, len(t), B)]
    cuts = chunk_starts[::G] + [int(bounds[-1])]
    cells, offs = entries(texts if segmented else [b"".join(texts)], nocase, words)
    model = sel.SelectModel([len(p) for p in PATS])
    out, dropped = [], 0
    for lo, hi in zip(cuts, cuts[1:]):
        inside = (offs >= lo) & (offs < hi)
        ep, eo, es, info = model.run(cells[inside], offs[inside] - lo, 0)
        dropped += info[1]
        for p, o in zip(ep.tolist(), (eo + lo).tolist()):
            f = int(np.searchsorted(bounds, o, side="right")) - 1
            out.append((os.path.basename(files[f][0]), PATS[p].decode(), (o - int(bounds[f])) % B))
    return sorted(out), dropped, len(cuts) - 1


CASES = [[], ["-S"], ["-i"], ["-S", "-W"]]


@pytest.mark.parametrize("flags", CASES, ids=["plain", "-S", "-i", "-S-W"])
def test_select_cli(gpu, tmp_path, flags):
    path, pats, files = write_inputs(tmp_path, [(1, 300), (2, 290), (3, 310)])
    exp, dropped, buffers = expected(files, 16, "-S" in flags, "-i" in flags, "-W" in flags)
    assert buffers == 1 and dropped == 0 and len(exp) > 30 and len({e[1] for e in exp}) >= 5
    every = entries([t for _, t in files] if "-S" in flags else [b"".join(t for _, t in files)], "-i" in flags, "-W" in flags)[0]
    assert every.size > len(exp) + (3 if "-W" in flags else 20)    # the selection drops records
    args = ["-f", path, "-p", pats, "-B", str(B), "-D", "0", "-G", "16", "-L", "64", "-w", "1", "-R", "128", "-v", "-o"] + flags
    hits, stats, p = run(args)
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    assert sorted((os.path.basename(h[2]), h[1], int(h[4]) - 1) for h in hits) == exp
    assert "NOTE" not in p.stderr
    # the planes -A prints hold every record
    args[args.index("-o")] = "-A"
    _, all_stats, _ = run(args)
    assert int(all_stats["Matches"]) == every.size


def test_cut_file_note(gpu, tmp_path):
    """one file of 48 chunks in buffers of 16: matches lie across both cuts; the entries that began in the buffer in
    front are no candidates, and the NOTE counts them"""
    t = bytearray(make_file(7, 3072))
    for cut in (1024, 2048):
        t[cut - 2:cut + 2] = b"abcd"
    d = tmp_path / "in"
    d.mkdir()
    (d / "cut.txt").write_bytes(bytes(t))
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"".join(p + b"\n" for p in PATS))
    files = [(str(d / "cut.txt"), bytes(t))]
    exp, dropped, buffers = expected(files, 16)
    assert buffers == 3 and dropped >= 4
    whole = expected(files, 48)[0]
    assert whole != exp
    hits, stats, p = run(["-f", str(d / "cut.txt"), "-p", str(pats), "-B", str(B), "-D", "0", "-G", "16", "-L", "64", "-w", "1",
                          "-R", "128", "-v", "-o"])
    got = collections.Counter((os.path.basename(h[2]), h[1], int(h[4]) - 1) for h in hits)
    want = collections.Counter(exp)
    assert got == want, "missing %s, not expected %s" % (sorted((want - got).items()), sorted((got - want).items()))
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    notes = [l for l in p.stderr.splitlines() if l.startswith("NOTE:")]
    assert len(notes) == 1 and notes[0].startswith("NOTE: %d matches began in the buffer in front" % dropped) and "-G/-B" in notes[0]
