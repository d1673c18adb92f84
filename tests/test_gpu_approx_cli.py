"""acm_grep -k N: approximate matching.  The -v lines, as a sorted set, are those of the brute force of
tests/approx_model.py over the files (one stream, or every file its own text with -S; with and without -i and
-I); a pattern too short for N stays exact and the NOTE says how many; a file cut by a small -G is either
reported whole or the undecided candidates are counted on stderr; every refused combination is refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import approx_model as am
from test_gpu_acm_grep import CLI

pytestmark = pytest.mark.gpu

B, G = 64, 16                 # buffers of 1024 bytes
LINE = re.compile(r"^Pattern (-?\d+) \('(.*)'\) found in file '(.*)' at offset (\d+) \[relative: (-?\d+)\] mismatches (\d+)$")
PATS = [(10, b"Needle"), (11, b"haystacks1"), (12, b"abcdefghijkl"), (13, b"xyz"), (14, b"NEEDLEneedle7")]
LOOSE = [(20, b"Tail=Head"), (21, b"qrs")]
UNDECIDED = "approximate candidates reach behind a buffer's end"

TEXTS = [b"a Needle, a Neodle, a needle and a Nexdlo; xyz xyq",
         b"haystacks1 haystackz1 hayztackz1 haYztackz1 xyz",
         b"abcdefghijkl abcdefgh1jkl abcd3fgh1jkl ab0d3fgh1jkl",
         b"", b"abcdefghijk",
         b"NEEDLEneedle7 NEEDLEneedle8 NEEDLEnaedle8 NEEbLEnaedle8 Need",
         b"le tail=head TAIL=HEAD Tail-Head TaiL-HeaT qrs QRS qrz Tail=He",
         b"ad"]


def write_inputs(tmp_path, texts=TEXTS):
    p, l = tmp_path / "p.txt", tmp_path / "l.txt"
    p.write_bytes(b"".join(b"%d %s\n" % x for x in PATS))
    l.write_bytes(b"".join(b"%d %s\n" % x for x in LOOSE))
    d = tmp_path / "in"
    d.mkdir()
    for i, t in enumerate(texts):
        (d / ("t%d.txt" % i)).write_bytes(t)
    order = [os.path.join(str(d), "t%d.txt" % i) for i in range(len(texts))]
    return str(p), str(l), ",".join(order), [(f, open(f, "rb").read()) for f in order]    # -f a,b,...: the files in this order


def run(args, ok=True):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120, errors="replace")
    if ok:
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = [m.groups() for m in (LINE.match(x) for x in p.stdout.splitlines()) if m]
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p


def base_args(path, pats, k):
    return ["-f", path, "-p", pats, "-k", str(k), "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", "1", "-R", "128", "-v"]


def lines_of(hits):
    """(file, id, pattern as printed, where in its chunk of B bytes the match ends, mismatches)"""
    return sorted((os.path.basename(h[2]), int(h[0]), h[1], int(h[4]) - 1, int(h[5])) for h in hits)


def budgets(pats, k):
    """(bytes, budget, nocase) per pattern: k where the pattern has 3 * (k + 1) bytes, else exact"""
    return [(p, k if len(p) >= 3 * (k + 1) else 0, nc) for p, nc in pats]


def expected(pats, ids, k, files, per_file):
    """the same tuples from the brute force: the files one stream, or each alone.  A match is printed for the file
    that holds the last byte of its first exact piece, with the offset of the whole pattern's end"""
    texts = [t for _, t in files]
    aps = am.as_approx(budgets(pats, k))
    got = am.brute_force(aps, texts if per_file else [b"".join(texts)])
    stream = b"".join(texts)
    bounds, base = [], 0
    for f, t in files:
        bounds.append((base, base + len(t), os.path.basename(f)))
        base += len(t)
    out = []
    for x, s, d in got:
        w = aps[x]
        mis = w.mismatches(stream[s:s + w.n])
        j = next(i for i in range(w.k + 1) if not mis[w.bounds[i]:w.bounds[i + 1]].any())
        o = s + w.bounds[j + 1] - 1
        a, name = next((a, n) for a, b, n in bounds if a <= o < b)
        assert s + w.n - 1 - a < B
        out.append((name, ids[x], w.bytes.decode(), s + w.n - 1 - a, d))
    return sorted(out)


def test_k1_and_k2(gpu, tmp_path):
    pats, loose, path, files = write_inputs(tmp_path)
    assert all(len(t) < B for _, t in files) and sum(len(t) for _, t in files) < B * G
    ids = [i for i, _ in PATS]
    exact = [(p, False) for _, p in PATS]
    for k, short in ((1, 1), (2, 2)):
        stream, alone = expected(exact, ids, k, files, False), expected(exact, ids, k, files, True)
        assert len(stream) > len(alone) > 8 and {d for *_, d in alone} == set(range(k + 1))
        assert ("t0.txt", 10, "Needle", 7, 0) in alone and (("t0.txt", 10, "Needle", 17, 1) in alone) == (k == 1)
        # "Need" + "le" across two files of one stream: printed for the file its first exact piece ends in
        assert (("t5.txt", 10, "Needle", 61, 0) if k == 1 else ("t6.txt", 10, "Needle", 1, 0)) in stream
        assert ("t0.txt", 13, "xyz", 45, 0) in alone and not any(i == 13 and d for _, i, _, _, d in stream)
        hits, stats, p = run(base_args(path, pats, k))
        assert lines_of(hits) == stream and int(stats["Matches"]) == int(stats["Matches reported"]) == len(stream)
        assert "NOTE: %d patterns have fewer than %d bytes and stay exact under -k %d" % (short, 3 * (k + 1), k) in p.stderr
        assert UNDECIDED not in p.stderr
        hits, stats, p = run(base_args(path, pats, k) + ["-S"])
        assert lines_of(hits) == alone and int(stats["Matches"]) == len(alone) and UNDECIDED not in p.stderr
        # -i: the whole comparison folds
        fold = expected([(p, True) for _, p in PATS], ids, k, files, True)
        assert len(fold) > len(alone)
        hits, _, _ = run(base_args(path, pats, k) + ["-S", "-i"])
        assert lines_of(hits) == fold
        # -I: its patterns fold, those of -p stay exact -- the short ones too
        both = expected(exact + [(p, True) for _, p in LOOSE], ids + [i for i, _ in LOOSE], k, files, True)
        assert {i for _, i, *_ in both} >= {10, 13, 20, 21} and ("t6.txt", 21, "qrs", 45, 0) in both
        assert ("t0.txt", 13, "xyz", 45, 0) in both
        hits, _, _ = run(base_args(path, pats, k) + ["-S", "-I", loose])
        assert lines_of(hits) == both
    # -t: every line a chunk of one stream
    lines = tmp_path / "lines.txt"
    lines.write_bytes(b"a Needle\na Neodle\nxyz haystackz1\nNee\ndle\n")
    hits, _, _ = run(base_args(str(lines), pats, 1) + ["-t"])
    got = sorted((int(h[0]), int(h[5])) for h in hits)
    assert got == [(10, 0), (10, 1), (11, 1), (13, 0)]                      # "Nee\ndle": 7 bytes, no match of 6 within 1
    hits, _, _ = run(base_args(str(lines), pats, 1) + ["-t", "-S"])
    assert sorted((int(h[0]), int(h[5])) for h in hits) == got


def test_a_file_cut_by_a_small_buffer(gpu, tmp_path):
    """a file of more than one buffer (B * G bytes).  A span across the border whose first exact piece lies behind
    the border is found with the tail of the buffer in front; one whose first exact piece lies in front of the
    border reaches behind the buffer's end: it is not decided, and the note counts it"""
    pats, _, _, _ = write_inputs(tmp_path)
    border = B * G
    big = bytearray(b"." * (border + 300))
    big[200:212] = b"abcdefgh1jkl"                               # whole: inside the first buffer, one mismatch
    big[border - 5:border + 7] = b"abcdefghijkl"                 # cut: piece 0 ("abcdef") ends behind the border: found
    big[border + 100:border + 112] = b"abcdefghijkl"             # whole: inside the second buffer
    d = tmp_path / "big"
    d.mkdir()
    (d / "big.bin").write_bytes(bytes(big))
    hits, _, p = run(base_args(str(d / "big.bin"), pats, 1) + ["-S"])
    found = sorted((int(h[0]), int(h[3]) - 1, int(h[5])) for h in hits)
    assert found == sorted([(12, 211, 1), (12, 6, 0), (12, 111, 0)])
    assert UNDECIDED not in p.stderr                             # complete
    big[border - 5:border + 7] = b"." * 12
    big[border - 8:border + 4] = b"abcdefgh1jkl"                 # cut: piece 0 ends in front of the border, the span behind it
    (d / "big.bin").write_bytes(bytes(big))
    hits, _, p = run(base_args(str(d / "big.bin"), pats, 1) + ["-S"])
    found = sorted((int(h[0]), int(h[3]) - 1, int(h[5])) for h in hits)
    assert found == sorted([(12, 211, 1), (12, 111, 0)])
    assert "NOTE: 1 " + UNDECIDED in p.stderr                    # ... or the loss is reported
    small = bytes(big[border - 40:border + 20])                  # the cut bytes in one small file: decided, no note
    (d / "small.bin").write_bytes(small)
    hits, _, p = run(base_args(str(d / "small.bin"), pats, 1) + ["-S"])
    assert UNDECIDED not in p.stderr and lines_of(hits) == [("small.bin", 12, "abcdefghijkl", 43, 1)]


def test_refused_combinations(gpu, tmp_path):
    pats, loose, path, _ = write_inputs(tmp_path)
    aux = tmp_path / "aux.txt"
    aux.write_text("0 0 *\n")
    sig = tmp_path / "sig.txt"
    sig.write_text("6162\n")
    out = tmp_path / "out"
    for extra, name in ((["-W"], "-W"), (["-S", "-P", str(aux)], "-P"), (["-Q", str(sig)], "-Q"), (["-S", "-K", str(sig)], "-K"),
                        (["-Q", str(sig), "-E"], "-E"), (["-o"], "-o"), (["-r", str(aux), "-O", str(out)], "-r"), (["-c"], "-c"),
                        (["-n"], "-n"), (["-C", "1", "-T", str(out)], "-C"), (["-F"], "-F")):
        _, _, p = run(base_args(path, pats, 1) + extra, ok=False)
        assert p.returncode != 0 and "ERROR: -k cannot be combined with %s:" % name in p.stdout, name
    for bad in ("0", "16", "x", "-1", "1x"):
        _, _, p = run(base_args(path, pats, bad), ok=False)
        assert p.returncode != 0 and "ERROR: -k takes 1 to 15" in p.stdout, bad
    _, _, p = run(base_args(path, pats, 15))                     # the largest budget: every pattern is too short
    assert "NOTE: 5 patterns have fewer than 48 bytes" in p.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-k N   " in r.stdout and "out of offset order" in r.stdout
