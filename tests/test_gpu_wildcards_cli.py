"""acm_grep -Q FILE -E: signatures in the extended syntax.  The stdout lines are those of the brute force of
tests/wildcard_model.py over the files (every file its own text with -S; the printed offset is where the match
ends, the post context of the last part included); -E without -Q and with -W is refused; the note on stderr
appears exactly when a candidate's positions are cut by a buffer border."""
import os
import subprocess

import pytest

import wildcard_model as wm
from test_gpu_acm_grep import CLI
from test_gpu_sequences_cli import B, G, base_args, lines_of, run

pytestmark = pytest.mark.gpu

SIGS = [(7, "4e65(65|45)646c65{1-3}7461696c??21"),      # Ne[eE]dle{1-3}tail.!
        (None, "48454144"),                              # HEAD: no id, so the sequence index (1)
        (40, "616263*64??66!(2e)67"),                    # abc*d.f[^.]g
        (41, "3?3?78{0-2}79?a"),                         # two digits, x, {0-2}, y, [*:JZjz..]
        (42, "!(41)4242")]                               # [^A]BB
NOTE = "wildcard candidates reach over a buffer border"

TEXTS = [b"HEAD Needle..tail_! abc d-f.g", b"NeEdle....tail HEAD NeEdle.tailX!HEAD", b"abc", b"d.fgg abcdefgg 42x.yz 07xyj",
         b"", b"NEEDLE--tail Needle--tailX? 1xyz 12xyz BBB ABB xBB", b"BB", b"NeEDLE.TAIL.! head neEDLE.TAIL.!"]


def parts_of(nocase=False):
    pats, seqs = [], []
    for k, (iid, body) in enumerate(SIGS):
        parts, gaps = wm.parse_body_ex(body)
        seqs.append((list(range(len(pats), len(pats) + len(parts))), gaps, k if iid is None else iid))
        pats += [wm.Pattern(p, nocase) for p in parts]
    return pats, seqs


def write_inputs(tmp_path, texts=TEXTS):
    q = tmp_path / "sigs.txt"
    q.write_text("# signatures\n" + "".join(("%d:%s\n" % s) if s[0] is not None else s[1] + "\n" for s in SIGS))
    d = tmp_path / "in"
    d.mkdir()
    for i, t in enumerate(texts):
        (d / ("t%d.txt" % i)).write_bytes(t)
    order = [os.path.join(str(d), "t%d.txt" % i) for i in range(len(texts))]
    return str(q), ",".join(order), [(f, open(f, "rb").read()) for f in order]


def expected(pats, seqs, files):
    """(file, id, where in its file the match ends): every file alone, each smaller than a chunk"""
    out, base = [], 0
    got = wm.span_sequences(pats, seqs, [t for _, t in files])
    for f, t in files:
        assert len(t) < B
        out += [(os.path.basename(f), seqs[q][2], o - base) for o, q in got if base <= o < base + len(t)]
        base += len(t)
    return sorted(out)


def test_extended_signatures(gpu, tmp_path):
    sigs, path, files = write_inputs(tmp_path)
    pats, seqs = parts_of()
    exp = expected(pats, seqs, files)
    assert {i for _, i, _ in exp} == {7, 1, 40, 41, 42} and len(exp) > 10
    assert ("t0.txt", 7, 18) in exp and ("t5.txt", 42, 49) in exp and ("t5.txt", 42, 45) not in exp
    hits, stats, p = run(base_args(path, sigs) + ["-E", "-S"])
    assert lines_of(hits) == exp and int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    assert NOTE not in p.stderr
    # -i: the exact runs ignore case, the positions around them do not
    loose, _ = parts_of(nocase=True)
    exp_i = expected(loose, seqs, files)
    assert len(exp_i) > len(exp) and ("t7.txt", 7, 12) in exp_i and ("t7.txt", 7, 31) not in exp_i
    hits, _, p = run(base_args(path, sigs) + ["-E", "-S", "-i"])
    assert lines_of(hits) == exp_i and NOTE not in p.stderr
    # without -E the same file is refused where it uses a new token
    _, _, p = run(base_args(path, sigs) + ["-S"], ok=False)
    assert p.returncode != 0 and "sigs.txt:2: column 7:" in p.stderr


def test_refused_combinations(gpu, tmp_path):
    sigs, path, _ = write_inputs(tmp_path)
    pat = tmp_path / "p.txt"
    pat.write_bytes(b"abc\n")
    p = subprocess.run([CLI, "-f", path.split(",")[0], "-p", str(pat), "-E", "-B", str(B), "-D", "0", "-G", str(G), "-L", "64"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "ERROR: -E needs -Q" in p.stdout
    _, _, p = run(base_args(path, sigs) + ["-E", "-W"], ok=False)
    assert p.returncode != 0 and "ERROR: -E cannot be combined with -W" in p.stdout
    bad = tmp_path / "bad.txt"
    bad.write_text("aa?b\naa(bbcc|dd)\n")
    _, _, p = run(base_args(path, str(bad)) + ["-E"], ok=False)
    assert p.returncode != 0 and "bad.txt:2: column 6:" in p.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-E   " in r.stdout and "-Q file" in r.stdout


def test_note_when_a_buffer_border_cuts_a_candidate(gpu, tmp_path):
    """a file of more than one buffer (B * G bytes): "07x" with the x first in the second buffer has its two
    digits in the first.  The candidate is not decided, the note says so; the same bytes inside a buffer match."""
    border = B * G
    big = bytearray(b"." * (border + 300))
    big[border - 2:border + 5] = b"07x.yz."                      # cut: the digits lie in front of the border
    big[border + 100:border + 107] = b"42x.yz."                  # whole: inside the second buffer
    big[200:207] = b"13xy:.."                                    # whole: inside the first
    d = tmp_path / "big"
    d.mkdir()
    (d / "big.bin").write_bytes(bytes(big))
    sigs, _, _ = write_inputs(tmp_path)
    hits, stats, p = run(base_args(str(d / "big.bin"), sigs) + ["-E", "-S"])
    assert NOTE in p.stderr and p.stderr.count(NOTE) == 1 and "NOTE: 1 wildcard" in p.stderr
    assert lines_of(hits) == [("big.bin", 41, 204 % B), ("big.bin", 41, (border + 105) % B)]
    small = bytes(big[border - 40:border + 20])                  # the cut bytes in one small file: decided, no note
    (d / "small.bin").write_bytes(small)
    hits, _, p = run(base_args(str(d / "small.bin"), sigs) + ["-E", "-S"])
    assert NOTE not in p.stderr and lines_of(hits) == [("small.bin", 41, 43)]
