"""acm_grep -I: a second pattern file whose patterns ignore case, beside the exact patterns of -p.  A
worker's files are one stream (with -S every file is its own text); the printed matches, the -c counts and
the -n line numbers are those of the case model (tests/case_model.py) over that stream, with buffers small
enough that cased matches straddle them."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import case_model as cm
from test_gpu_acm_grep import CLI

pytestmark = pytest.mark.gpu

EXACT = [b"abc", b"ABC", b"Needle", b"cdefabcde", b"fAbcdeFabcdefabcDefabcdefaBcdefabc"[:33]]
LOOSE = [b"aBc", b"HayStack", b"CDEFABCDE"]
PATS = [(p, False) for p in EXACT] + [(p, True) for p in LOOSE]
B, G = 64, 16                 # buffers of 1024 bytes

LINE = re.compile(r"^Pattern (-?\d+) \('(.*)'\) found in file '(.*)' at (?:line (\d+) )?offset (\d+) \[relative: (-?\d+)\]$")
FILE_LINE = re.compile(r"^Count file '(.*)': (\d+)$", re.M)
PAT_LINE = re.compile(r"^Count pattern (-?\d+) \('(.*)'\): (\d+)$", re.M)


def run(args):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120, errors="replace")
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = [m.groups() for m in (LINE.match(l) for l in p.stdout.splitlines()) if m]
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p.stdout


def pattern_files(tmp_path):
    e, l = tmp_path / "exact.txt", tmp_path / "loose.txt"
    e.write_bytes(b"".join(p + b"\n" for p in EXACT))
    l.write_bytes(b"".join(p + b"\n" for p in LOOSE))
    return str(e), str(l)


def make_text(seed, tokens):
    t = cm.planted_text(PATS, tokens, seed, filler=b" .,\n\n  xyz", gap=12).copy()
    # cased matches across the buffer boundaries at 1024, 2048 and 3072: one that holds, two that do not
    t[1010:1043] = np.frombuffer(EXACT[4], dtype=np.uint8)
    t[2044:2050] = np.frombuffer(b"Needle", dtype=np.uint8)
    t[3070:3076] = np.frombuffer(b"NEEDLE", dtype=np.uint8)
    t[4090:4099] = np.frombuffer(b"cdefAbcde", dtype=np.uint8)
    return t


def inputs(tmp_path, which):
    d = tmp_path / "in"
    d.mkdir()
    sizes = {"file": [(3, 420)], "directory": [(4, 440), (5, 470)]}[which]
    per_file = {}
    for i, (seed, tokens) in enumerate(sizes):
        t = make_text(seed, tokens)
        assert t.size > 4200
        (d / ("c%d.txt" % i)).write_bytes(t.tobytes())
        per_file[str(d / ("c%d.txt" % i))] = t
    if which == "file":
        path = next(iter(per_file))
        return path, [(path, per_file[path])]
    order = [os.path.join(str(d), e) for e in os.listdir(str(d))]    # readdir order, as acm_grep walks it
    return str(d), [(f, per_file[f]) for f in order]


def expected(model, files, all_patterns, segmented):
    """(file, pattern bytes, position in the file, 1-based line) of every record over the worker's stream"""
    texts = [t for _, t in files]
    bounds = np.cumsum([0] + [t.size for t in texts])
    if segmented:
        offs, pats, _ = model.per_text([t.tobytes() for t in texts], all_patterns)
    else:
        offs, pats, _ = model.records(np.concatenate(texts), all_patterns)
    k = np.searchsorted(bounds, offs.astype(np.int64), side="right") - 1
    out = []
    for o, p, f in zip(offs.tolist(), pats.tolist(), k.tolist()):
        pos = o - int(bounds[f])
        line = 1 + int(np.count_nonzero(texts[f][:pos] == 0x0A))
        out.append((os.path.basename(files[f][0]), PATS[p][0].decode(), pos, line))
    return out


CASES = [(w, a, s) for w in ("file", "directory") for a in (False, True) for s in (False, True)]


@pytest.mark.parametrize("which,all_patterns,segmented", CASES,
                         ids=["%s%s%s" % (w, "-A" if a else "", "-S" if s else "") for w, a, s in CASES])
def test_case_cli(gpu, tmp_path, which, all_patterns, segmented):
    exact, loose = pattern_files(tmp_path)
    path, files = inputs(tmp_path, which)
    model = cm.CaseModel(PATS)
    exp = expected(model, files, all_patterns, segmented)
    args = ["-f", path, "-p", exact, "-I", loose, "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", "1",
            "-R", "128", "-v"] + (["-A"] if all_patterns else []) + (["-S"] if segmented else [])
    # the fixture tells the rules apart: cased matches across buffers, kept and dropped
    names = [os.path.basename(f) for f, _ in files]
    every = exp if all_patterns else expected(model, files, True, segmented)
    assert any(e[1] == EXACT[4].decode() and e[2] == 1042 for e in every)
    assert any(e[1] == "Needle" and e[2] == 2049 for e in every)
    assert not any(e[1] == "Needle" and e[2] == 3075 for e in every)
    assert any(e[1] == "CDEFABCDE" and e[2] == 4098 for e in every)
    assert not any(e[1] == "cdefabcde" and e[2] == 4098 for e in every)

    hits, stats, _ = run(args)
    assert int(stats["Kernel launches"]) >= 4 * len(files)
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    got = sorted((os.path.basename(h[2]), h[1], int(h[5]) - 1) for h in hits)
    assert got == sorted((f, p, pos % B) for f, p, pos, _ in exp)
    assert all(h[3] is None for h in hits)
    # the candidates were more: the same run with -i reports every pattern whatever its case
    _, loose_stats, _ = run(args + ["-i"])
    assert int(loose_stats["Matches"]) > len(exp)

    # -c and -n: counts tallied on the device from the pass's output, line numbers of the kept records
    hits, stats, out = run(args + ["-c", "-n"])
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    got = sorted((os.path.basename(h[2]), h[1], int(h[5]) - 1, int(h[3])) for h in hits)
    assert got == sorted((f, p, pos % B, line) for f, p, pos, line in exp)
    per_file = collections.Counter(e[0] for e in exp)
    assert {os.path.basename(f): int(n) for f, n in FILE_LINE.findall(out)} == {n: per_file[n] for n in names}
    per_pat = collections.Counter(e[1] for e in exp)
    assert {p: int(n) for _, p, n in PAT_LINE.findall(out)} == dict(per_pat)
    assert int(stats["Processed lines"]) == sum(int(np.count_nonzero(t == 0x0A)) for _, t in files)


def test_rejected_with_words_or_follow(gpu, tmp_path):
    exact, loose = pattern_files(tmp_path)
    p = str(tmp_path / "x.txt")
    open(p, "wb").write(b"abc\n")
    for flag in ("-W", "-F"):
        r = subprocess.run([CLI, "-f", p, "-p", exact, "-I", loose, "-B", "64", "-D", "0", "-G", "16", "-L", "64", flag],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
        assert "-I cannot be combined with -W or -F" in r.stdout + r.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-I file" in r.stdout


def test_nocase_makes_it_a_second_pattern_file(gpu, tmp_path):
    exact, loose = pattern_files(tmp_path)
    both = tmp_path / "both.txt"
    both.write_bytes(open(exact, "rb").read() + open(loose, "rb").read())
    path, files = inputs(tmp_path, "file")
    base = ["-f", path, "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", "1", "-R", "128", "-v", "-i", "-A"]
    h1, s1, _ = run(base + ["-p", exact, "-I", loose])
    h2, s2, _ = run(base + ["-p", str(both)])
    assert s1["Matches"] == s2["Matches"] and int(s1["Matches"]) > 0
    # (the ids of the second file's patterns count from 0 again; everything else is the same line)
    assert sorted(h[1:] for h in h1) == sorted(h[1:] for h in h2)
    model = cm.CaseModel([(p, True) for p, _ in PATS])
    assert int(s1["Matches"]) == model.records(files[0][1], True)[0].size
