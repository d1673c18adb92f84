"""acm_grep -Q: a signature file, the printed matches those of the signatures.  The stdout lines are those of
the brute force of tests/sequence_model.py over the files: one stream without -S, every file its own text with
-S, the parts exact beside the loose patterns of -I; and the flags -Q refuses."""
import os
import re
import subprocess

import pytest

import sequence_model as sm
from test_gpu_acm_grep import CLI

pytestmark = pytest.mark.gpu

B, G = 64, 16                 # buffers of 1024 bytes
SIGS = [(7, "4e6565646c65{1-3}7461696c"),          # Needle{1-3}tail
        (None, "48454144"),                         # HEAD: no id, so the sequence index (1)
        (40, "616263*646566??67"),                  # abc*def??g
        (41, "7878{5-2}7979")]                      # xx{5-2}yy: never
LINE = re.compile(r"^Sequence (-?\d+) found in file '(.*)' at offset (\d+) \[relative: (-?\d+)\]$")

TEXTS = [b"HEAD Needle..tail abc def.g", b"Needle....tail HEAD Needle.tailHEAD", b"abc", b"def.g abcdef-g xx...yy",
         b"", b"NEEDLE--tail Needle--TAIL needle.tail abcdefgg"]


def parts_of():
    """(patterns, sequences with their ids) of SIGS, through the model's own parser"""
    pats, seqs = [], []
    for k, (iid, body) in enumerate(SIGS):
        parts, gaps = sm.parse_body(body)
        seqs.append((list(range(len(pats), len(pats) + len(parts))), gaps, k if iid is None else iid))
        pats += parts
    return pats, seqs


def write_inputs(tmp_path):
    q = tmp_path / "sigs.txt"
    q.write_text("# signatures\n" + "".join(("%d:%s\n" % s) if s[0] is not None else s[1] + "\n" for s in SIGS))
    d = tmp_path / "in"
    d.mkdir()
    for i, t in enumerate(TEXTS):
        (d / ("t%d.txt" % i)).write_bytes(t)
    order = [os.path.join(str(d), "t%d.txt" % i) for i in range(len(TEXTS))]
    return str(q), ",".join(order), [(f, open(f, "rb").read()) for f in order]    # -f a,b,...: the files in this order


def run(args, ok=True):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120, errors="replace")
    if ok:
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = [m.groups() for m in (LINE.match(l) for l in p.stdout.splitlines()) if m]
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p


def base_args(path, sigs):
    return ["-f", path, "-Q", sigs, "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", "1", "-R", "128", "-v"]


def lines_of(hits):
    """(file, id, where in its chunk of B bytes the match ends)"""
    return sorted((os.path.basename(h[1]), int(h[0]), int(h[3]) - 1) for h in hits)


def expected(pats, seqs, files, per_file):
    """the same triples from the brute force: the files one stream (every file is smaller than a buffer), or each alone"""
    texts = [t for _, t in files]
    got = sm.brute_force(pats, seqs, texts if per_file else [b"".join(texts)])
    base, out = 0, []
    bounds = []
    for f, t in files:
        bounds.append((base, base + len(t), os.path.basename(f)))
        base += len(t)
    for o, q in got:
        a, name = next((a, n) for a, b, n in bounds if a <= o < b)
        out.append((name, seqs[q][2], (o - a) % B))
    return sorted(out)


def test_signatures(gpu, tmp_path):
    sigs, path, files = write_inputs(tmp_path)
    pats, seqs = parts_of()
    assert sum(len(t) for _, t in files) < B * G
    stream = expected(pats, seqs, files, False)
    alone = expected(pats, seqs, files, True)
    assert {i for _, i, _ in alone} == {7, 1, 40} and len(stream) > len(alone) > 6     # chains cross files in one stream
    hits, stats, _ = run(base_args(path, sigs))
    assert lines_of(hits) == stream and int(stats["Matches"]) == int(stats["Matches reported"]) == len(stream)
    hits, stats, _ = run(base_args(path, sigs) + ["-S"])
    assert lines_of(hits) == alone and int(stats["Matches"]) == len(alone)
    # -i: every part ignores case
    loose_all = [(p, True) for p in pats]
    exp = expected(loose_all, seqs, files, True)
    assert len(exp) > len(alone)
    hits, _, _ = run(base_args(path, sigs) + ["-S", "-i"])
    assert lines_of(hits) == exp


def test_beside_patterns_and_loose_patterns(gpu, tmp_path):
    """-p and -I beside -Q: their patterns come first and are in no sequence; the automaton is mixed, the parts
    of the signatures stay exact"""
    sigs, path, files = write_inputs(tmp_path)
    pats, seqs = parts_of()
    p, l = tmp_path / "p.txt", tmp_path / "l.txt"
    p.write_bytes(b"abc\nzz\n")
    l.write_bytes(b"needle\nhead\n")
    shifted = [([x + 4 for x in s[0]], s[1], s[2]) for s in seqs]
    allp = [(b"abc", False), (b"zz", False), (b"needle", True), (b"head", True)] + [(x, False) for x in pats]
    exp = expected(allp, shifted, files, True)
    assert exp == expected(pats, seqs, files, True)
    hits, stats, _ = run(base_args(path, sigs) + ["-S", "-p", str(p), "-I", str(l)])
    assert lines_of(hits) == exp and int(stats["Matches"]) == len(exp)


def test_refused_combinations(gpu, tmp_path):
    sigs, path, _ = write_inputs(tmp_path)
    for flag in ("-c", "-n", "-W", "-A"):
        _, _, p = run(base_args(path, sigs) + [flag], ok=False)
        assert p.returncode != 0 and "ERROR: -Q cannot be combined with -c, -n, -W or -A" in p.stdout, flag
    bad = tmp_path / "bad.txt"
    bad.write_text("aabb\naa(bb|cc)\n")
    _, _, p = run(base_args(path, str(bad)), ok=False)
    assert p.returncode != 0 and "bad.txt:2: column 3:" in p.stderr
    _, _, p = run(base_args(path, str(tmp_path / "missing.txt")), ok=False)
    assert p.returncode != 0 and "does not exist" in p.stdout
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-Q file" in r.stdout


def test_with_position_windows(gpu, tmp_path):
    """-P beside -Q: the indices of the parts; "Needle" within the first five bytes of its file, "HEAD" at its end"""
    sigs, path, files = write_inputs(tmp_path)
    pats, seqs = parts_of()
    windows = {0: (0, 5, False), 2: (4, 4, True)}
    pos = tmp_path / "win.pos"
    pos.write_text("0 0 5\n2 4 4 end\n")
    free = expected(pats, seqs, files, True)
    texts = [t for _, t in files]
    got = sm.brute_force(pats, seqs, texts, windows=windows)
    base, kept = 0, []
    for f, t in files:
        kept += [(os.path.basename(f), seqs[q][2], (o - base) % B) for o, q in got if base <= o < base + len(t)]
        base += len(t)
    kept = sorted(kept)
    assert {i for _, i, _ in kept} == {7, 1, 40} and 2 < len(kept) < len(free)
    assert [e for e in kept if e[1] == 7] == [("t0.txt", 7, 16)] and [e for e in kept if e[1] == 1] == [("t1.txt", 1, 34)]
    hits, stats, p = run(base_args(path, sigs) + ["-S", "-P", str(pos)])
    assert lines_of(hits) == kept and int(stats["Matches"]) == len(kept) and "ERROR" not in p.stdout
