"""acm_grep -k N -e: edit-distance matching.  The -v lines, with their edits and lengths, are the records of the
model of tests/edit_model.py over the files (one stream, or every file its own text with -S; with -i, -I and -t)
and have the three properties against brute force; -c counts the unique records; a match whose window crosses a
buffer's end comes out as in a run with one buffer; -e without -k, -k 5 -e and every refused combination are
errors."""
import os
import re
import subprocess

import pytest

import approx_model as am
import edit_model as em
from edit_model import Edit
from test_gpu_acm_grep import CLI

pytestmark = pytest.mark.gpu

B, G = 64, 16                 # buffers of 1024 bytes
LINE = re.compile(r"^Pattern (-?\d+) \('(.*)'\) found in file '(.*)' at offset (\d+) \[relative: (-?\d+)\] edits (\d+) length (\d+)$")
PATS = [(10, b"Needle"), (11, b"haystacks1"), (12, b"abcdefghijkl"), (13, b"xyz"), (14, b"NEEDLEneedle7")]
LOOSE = [(20, b"Tail=Head"), (21, b"qrs")]
UNDECIDED = "approximate candidates reach behind a buffer's end"

TEXTS = [b"a Needle, a Nedle, a Neeedle, a needle and a Nexdlo; xyz xyq",
         b"haystacks1 haystaks1 haysstackz1 hayztackz1 haYztakz1 xyz",
         b"abcdefghijkl abcdefghjkl abcd3fgh1jkl ab0defgh#ijkl bcdefghijk",
         b"", b"abcdefghijk",
         b"NEEDLEneedle7 NEEDLEneedle NEEDLEnaedle78 NEEbLEnedle7 Need",
         b"le tail=head TAIL=HEAD Tail-Head Tal=HeaT qrs QRS qrz Tail=He",
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
    return str(p), str(l), ",".join(order), [(f, open(f, "rb").read()) for f in order]


def run(args, ok=True):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120, errors="replace")
    if ok:
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = [m.groups() for m in (LINE.match(x) for x in p.stdout.splitlines()) if m]
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p


def base_args(path, pats, k, g=G):
    return ["-f", path, "-p", pats, "-k", str(k), "-e", "-B", str(B), "-D", "0", "-G", str(g), "-L", "64", "-w", "1", "-R", "128", "-v"]


def lines_of(hits):
    """(file, id, pattern as printed, where in its file the match ends, edits, length)"""
    return sorted((os.path.basename(h[2]), int(h[0]), h[1], int(h[4]) - 1, int(h[5]), int(h[6])) for h in hits)


def pattern_set(pats, k):
    """an edit pattern where it has 3 * (k + 1) bytes, else exact"""
    return [Edit(p, k, nc) if len(p) >= 3 * (k + 1) else am.Approx(p, 0, nc) for p, nc in pats]


def expected(pats, ids, k, files, per_file):
    """the same tuples from the model: the files one stream, or each alone; a match is printed for the file that
    holds its last byte.  And the (pattern x, offset, edits, length) records for em.check."""
    texts = [t for _, t in files]
    ps = pattern_set(pats, k)
    model = em.EditModel(ps)
    gp, go, gd, gl, und, _ = model.scan(texts if per_file else [b"".join(texts)])
    assert und == 0
    bounds, base = [], 0
    for f, t in files:
        bounds.append((base, base + len(t), os.path.basename(f)))
        base += len(t)
    out, recs = [], []
    for p, o, d, ln in zip(gp.tolist(), go.tolist(), gd.tolist(), gl.tolist()):
        x = model.owner[p]
        a, name = next((a, n) for a, b, n in bounds if a <= o < b)
        out.append((name, ids[x], ps[x].bytes.decode(), o - a, d, ln))
        recs.append((x, o, d, ln))
    return sorted(out), recs, ps


def records_of(lines, ids, ps, files):
    """(pattern x, offset in the concatenation, edits, length) of printed lines, for em.check"""
    at, base = {}, 0
    for f, t in files:
        at[os.path.basename(f)] = base
        base += len(t)
    return [(ids.index(i), at[name] + o, d, ln) for name, i, _, o, d, ln in lines]


def test_k1_and_k2(gpu, tmp_path):
    pats, loose, path, files = write_inputs(tmp_path)
    assert all(len(t) < B for _, t in files) and sum(len(t) for _, t in files) < B * G
    ids = [i for i, _ in PATS]
    exact = [(p, False) for _, p in PATS]
    texts = [t for _, t in files]
    for k, short in ((1, 1), (2, 2)):
        stream, _, ps = expected(exact, ids, k, files, False)
        alone, recs, _ = expected(exact, ids, k, files, True)
        assert len(stream) > len(alone) > 8 and {d for *_, d, _ in alone} == set(range(k + 1))
        assert em.check(ps, texts, recs) > 8
        assert ("t0.txt", 10, "Needle", 7, 0, 6) in alone
        # "Nedle", and "Neeedle", whose shortest span with one error is "eedle" (6 bytes need k = 1: 9 need k = 2)
        assert ((("t0.txt", 10, "Needle", 16, 1, 5) in alone) and (("t0.txt", 10, "Needle", 27, 1, 5) in alone)) == (k == 1)
        assert ("t2.txt", 12, "abcdefghijkl", 23, 1, 11) in alone                                                   # "abcdefghjkl"
        assert ("t0.txt", 13, "xyz", 55, 0, 3) in alone and not any(i == 13 and d for _, i, _, _, d, _ in stream)
        hits, stats, p = run(base_args(path, pats, k))
        assert lines_of(hits) == stream and int(stats["Matches"]) == int(stats["Matches reported"]) == len(stream)
        assert "NOTE: %d patterns have fewer than %d bytes and stay exact under -k %d" % (short, 3 * (k + 1), k) in p.stderr
        assert UNDECIDED not in p.stderr
        hits, stats, p = run(base_args(path, pats, k) + ["-S"])
        assert lines_of(hits) == alone and int(stats["Matches"]) == len(alone) and UNDECIDED not in p.stderr
        # -c: the unique records, per file and per pattern as written
        _, _, p = run(base_args(path, pats, k) + ["-S", "-c"])
        for name in {n for n, *_ in alone}:
            assert re.search(r"^Count file '.*%s': %d$" % (re.escape(name), sum(1 for r in alone if r[0] == name)), p.stdout, flags=re.M)
        for i, pb in PATS:
            n = sum(1 for r in alone if r[1] == i)
            assert ("Count pattern %d ('%s'): %d\n" % (i, pb.decode(), n) in p.stdout) == (n > 0)
        # -i: the whole comparison folds
        fold, _, _ = expected([(p, True) for _, p in PATS], ids, k, files, True)
        assert len(fold) > len(alone)
        hits, _, _ = run(base_args(path, pats, k) + ["-S", "-i"])
        assert lines_of(hits) == fold
        # -I: its patterns fold, those of -p stay exact.  The case pass in front takes the folded candidates of the
        # exact patterns away, so fewer pieces may speak for a match: the properties hold, and every line is the model's
        both_p = exact + [(p, True) for _, p in LOOSE]
        both_i = ids + [i for i, _ in LOOSE]
        both, _, ps2 = expected(both_p, both_i, k, files, True)
        hits, _, _ = run(base_args(path, pats, k) + ["-S", "-I", loose])
        got = lines_of(hits)
        assert set(got) <= set(both) and {i for _, i, *_ in got} >= {10, 13, 20, 21} and ("t6.txt", 21, "qrs", 44, 0, 3) in got
        assert em.check(ps2, texts, records_of(got, both_i, ps2, files)) > 8
    # -t: every line a chunk of one stream
    lines = tmp_path / "lines.txt"
    lines.write_bytes(b"a Needle\na Nedle\nxyz haystakz1\nNee\ndle\n")
    hits, _, _ = run(base_args(str(lines), pats, 1) + ["-t"])
    got = sorted((int(h[0]), int(h[5]), int(h[6])) for h in hits)
    assert got == [(10, 0, 6), (10, 1, 5), (10, 1, 7), (13, 0, 3)]            # "Nee\ndle" is "Needle" with a byte added
    hits, _, _ = run(base_args(str(lines), pats, 1) + ["-t", "-S"])
    alone = sorted((int(h[0]), int(h[5]), int(h[6])) for h in hits)
    assert set(got[:2] + got[3:]) <= set(alone) <= set(got)


def test_a_window_across_a_buffers_end(gpu, tmp_path):
    """a file of more than one buffer: matches whose pieces end behind the border are found with the tail of the
    buffer in front, and the lines are those of a run whose one buffer holds the whole file"""
    pats, _, _, _ = write_inputs(tmp_path)
    border = B * G
    big = bytearray(b"." * (border + 300))
    big[200:211] = b"abcdefghjkl"                                # inside the first buffer, a byte dropped
    big[border - 5:border + 8] = b"abcdef#ghijkl"                # across the border, a byte added: both pieces end behind it
    big[border + 100:border + 112] = b"abcdefghijkl"             # inside the second buffer
    d = tmp_path / "big"
    d.mkdir()
    (d / "big.bin").write_bytes(bytes(big))
    small, _, p1 = run(base_args(str(d / "big.bin"), pats, 1) + ["-S"])
    whole, _, p2 = run(base_args(str(d / "big.bin"), pats, 1, g=2 * G) + ["-S"])
    # (the offset of a -v line counts from its buffer's first byte: the whole file's offsets modulo the small buffer)
    found = sorted((int(h[0]), int(h[3]) - 1, int(h[5]), int(h[6])) for h in small)
    assert found == sorted((int(h[0]), (int(h[3]) - 1) % border, int(h[5]), int(h[6])) for h in whole)
    assert found == [(12, 7, 1, 13), (12, 111, 0, 12), (12, 210, 1, 11)]
    assert sorted(int(h[3]) - 1 for h in whole) == [210, border + 7, border + 111]
    assert UNDECIDED not in p1.stderr and UNDECIDED not in p2.stderr
    # the only exact piece ends in front of the border with its window behind it: not decided, and the note says so
    big[border - 5:border + 8] = b"." * 13
    big[border - 8:border + 4] = b"abcdefgh1jkl"
    (d / "big.bin").write_bytes(bytes(big))
    small, _, p1 = run(base_args(str(d / "big.bin"), pats, 1) + ["-S"])
    assert "NOTE: 1 " + UNDECIDED in p1.stderr
    assert sorted((int(h[0]), int(h[3]) - 1, int(h[5])) for h in small) == [(12, 111, 0), (12, 210, 1)]


def test_errors(gpu, tmp_path):
    pats, loose, path, _ = write_inputs(tmp_path)
    aux = tmp_path / "aux.txt"
    aux.write_text("0 0 *\n")
    sig = tmp_path / "sig.txt"
    sig.write_text("6162\n")
    out = tmp_path / "out"
    for extra, name in ((["-W"], "-W"), (["-S", "-P", str(aux)], "-P"), (["-Q", str(sig)], "-Q"), (["-S", "-K", str(sig)], "-K"),
                        (["-Q", str(sig), "-E"], "-E"), (["-o"], "-o"), (["-r", str(aux), "-O", str(out)], "-r"),
                        (["-n"], "-n"), (["-C", "1", "-T", str(out)], "-C"), (["-F"], "-F")):
        _, _, p = run(base_args(path, pats, 1) + extra, ok=False)
        assert p.returncode != 0 and "ERROR: -k cannot be combined with %s:" % name in p.stdout, name
    for bad in ("5", "15"):
        _, _, p = run(base_args(path, pats, bad), ok=False)
        assert p.returncode != 0 and "ERROR: -e needs -k N with N from 1 to 4" in p.stdout, bad
    args = base_args(path, pats, 1)
    _, _, p = run(args[:4] + args[6:], ok=False)                 # -e without -k
    assert p.returncode != 0 and "ERROR: -e needs -k N" in p.stdout
    _, _, p = run(base_args(path, pats, 4))                      # the largest budget: every pattern is too short
    assert "NOTE: 5 patterns have fewer than 15 bytes" in p.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "  -e     " in r.stdout and "edits <d> length <l>" in r.stdout
