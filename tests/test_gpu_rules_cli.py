"""acm_grep -K: a logical signature file, the printed lines the rules that hold, per file (with -t: per line).  The
stdout lines are those of the model of tests/rule_model.py over counts found without an automaton; -E bodies, -t,
beside -p and -Q, the flags -K refuses, and a file larger than a buffer: reported as cut, no rule line."""
import os
import re
import subprocess

import pytest

import rule_model as rm
import sequence_model as sm
from test_gpu_acm_grep import CLI

pytestmark = pytest.mark.gpu

B, G = 64, 16                 # buffers of 1024 bytes
#        id    expression   bodies
RULES = [(7, "0&1", ["4e6565646c65", "7461696c{1-3}656e64"]),      # Needle & tail{1-3}end
         (None, "0|1>1", ["48454144", "787879"]),                  # HEAD | xxy > 1: no id, so the rule index (1)
         (40, "(0|1)>2", ["6162", "6364"]),                        # more than two of ab and cd together
         (41, "0&1=0", ["6f6e6c79", "6e65766572"])]                # only, and never not
LINE = re.compile(r"^Rule (-?\d+) matched in file '(.*)' \[text at offset (\d+)\]$")

TEXTS = [b"HEAD Needle and tail..end", b"Needle tail....end tail.end", b"tail.end Needle", b"xxy HEAD", b"xxyxxy xxxy", b"xxy",
         b"ab cd", b"ab cd ab", b"abababcd", b"", b"only", b"only never", b"never", b"only only HEAD Needle tail---end abcdabcd"]


def parsed(rules=RULES):
    """(patterns, sequences, rules over sequence indices with their ids) through the models' own parsers"""
    pats, seqs, out = [], [], []
    for k, (iid, expr, bodies) in enumerate(rules):
        ops = []
        for body in bodies:
            parts, gaps = sm.parse_body(body)
            ops.append(len(seqs))
            seqs.append((list(range(len(pats), len(pats) + len(parts))), gaps))
            pats += parts
        out.append((ops, expr, k if iid is None else iid))
    return pats, seqs, out


def holds(text, pats, seqs, rules, nocase=False):
    """ids of the rules that hold in one text: every sequence counted by brute force, then the model's evaluation"""
    p = [(x, nocase) for x in pats]
    hits = [q for _, q in sm.brute_force(p, seqs, [text])]
    out = []
    for ops, expr, iid in rules:
        counts = [hits.count(q) for q in ops]
        if sum(counts) and rm.evaluate(rm.parse(expr, len(ops)), counts)[1]:
            out.append(iid)
    return out


def write_rules(path, rules=RULES):
    path.write_text("# rules\n\n" + "".join(("" if iid is None else "%d:" % iid) + ";".join([e] + b) + "\n" for iid, e, b in rules))
    return str(path)


def write_inputs(tmp_path, texts=TEXTS):
    d = tmp_path / "in"
    d.mkdir()
    for i, t in enumerate(texts):
        (d / ("t%02d.txt" % i)).write_bytes(t)
    order = [os.path.join(str(d), "t%02d.txt" % i) for i in range(len(texts))]
    return ",".join(order), [(f, open(f, "rb").read()) for f in order]


def run(args, ok=True):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120, errors="replace")
    if ok:
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = sorted((os.path.basename(m.group(2)), int(m.group(1)), int(m.group(3)))
                  for m in (LINE.match(l) for l in p.stdout.splitlines()) if m)
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p


def base_args(path, rules):
    return ["-f", path, "-K", rules, "-S", "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", "1", "-R", "128", "-v"]


def test_rules_per_file(gpu, tmp_path):
    rules = write_rules(tmp_path / "rules.ldb")
    path, files = write_inputs(tmp_path)
    pats, seqs, rs = parsed()
    assert sum(len(t) for _, t in files) < B * G
    exp = sorted((os.path.basename(f), iid, 0) for f, t in files for iid in holds(t, pats, seqs, rs))
    assert {i for _, i, _ in exp} == {7, 1, 40, 41} and [n for n, i, _ in exp if i == 7] == ["t00.txt", "t01.txt", "t02.txt", "t13.txt"]
    assert len(exp) == 13
    hits, stats, p = run(base_args(path, rules))
    assert hits == exp and int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp) and "NOTE" not in p.stderr
    # two workers, buffers of two files or so
    hits, _, _ = run(base_args(path, rules)[:-5] + ["-w", "2", "-R", "128", "-v"])
    assert hits == exp
    # -i: every body ignores case
    expi = sorted((os.path.basename(f), iid, 0) for f, t in files for iid in holds(t.swapcase(), pats, seqs, rs, nocase=True))
    swapped = tmp_path / "swapped"
    swapped.mkdir()
    for f, t in files:
        (swapped / os.path.basename(f)).write_bytes(t.swapcase())
    hits, _, _ = run(base_args(str(swapped), rules) + ["-i"])
    assert hits == exp == expi
    hits, _, _ = run(base_args(str(swapped), rules))
    assert hits == []


def test_beside_patterns_and_signatures(gpu, tmp_path):
    """-p and -Q beside -K: their patterns and signatures come first and are operands of nothing"""
    rules = write_rules(tmp_path / "rules.ldb")
    path, files = write_inputs(tmp_path)
    pats, seqs, rs = parsed()
    exp = sorted((os.path.basename(f), iid, 0) for f, t in files for iid in holds(t, pats, seqs, rs))
    p, q = tmp_path / "p.txt", tmp_path / "q.txt"
    p.write_bytes(b"Needle\nab\n")
    q.write_text("9:48454144*787879\n6162\n")
    hits, stats, _ = run(base_args(path, rules) + ["-p", str(p), "-Q", str(q)])
    assert hits == exp and int(stats["Matches"]) == len(exp)


def test_extended_bodies(gpu, tmp_path):
    """-E: nibble wildcards and one-byte alternatives in the bodies"""
    ext = [(5, "0&1", ["6?6264", "(31|32)7879"]), (6, "0>1", ["7a!(7a)7a"])]           # [`-o]bd & [12]xy; z[^z]z twice
    rules = write_rules(tmp_path / "ext.ldb", ext)
    texts = [b"abd 1xy", b"Abd 2xy", b"obd 3xy 2xy", b"zaz", b"zaz zbz", b"zzzz.zz", b"zazaz"]
    path, files = write_inputs(tmp_path, texts)
    rx = [re.compile(rb"(?=[\x60-\x6f]bd)"), re.compile(rb"(?=[12]xy)"), re.compile(rb"(?=z[^z]z)", re.S)]
    exp = []
    for f, t in files:
        c = [len(r.findall(t)) for r in rx]
        exp += [(os.path.basename(f), 5, 0)] * (c[0] > 0 and c[1] > 0) + [(os.path.basename(f), 6, 0)] * (c[2] > 1)
    assert exp == [("t00.txt", 5, 0), ("t02.txt", 5, 0), ("t04.txt", 6, 0), ("t06.txt", 6, 0)]
    hits, _, _ = run(base_args(path, rules) + ["-E"])
    assert hits == exp
    _, _, p = run(base_args(path, rules), ok=False)                                     # the syntax needs -E
    assert p.returncode != 0 and "ext.ldb:3: column" in p.stderr


def test_text_mode(gpu, tmp_path):
    """-t: every line is a text; the offset printed is where the line begins in its file"""
    rules = write_rules(tmp_path / "rules.ldb")
    pats, seqs, rs = parsed()
    lines = [b"Needle\n", b"tail.end Needle\n", b"\n", b"HEAD\n", b"tail.end\n", b"ab cd ab\n", b"only never\n", b"only"]
    f = tmp_path / "lines.txt"
    f.write_bytes(b"".join(lines))
    exp, at = [], 0
    for l in lines:
        exp += [("lines.txt", iid, at) for iid in holds(l, pats, seqs, rs)]
        at += len(l)
    assert exp == [("lines.txt", 7, 7), ("lines.txt", 1, 24), ("lines.txt", 40, 38), ("lines.txt", 41, 58)]
    hits, stats, p = run(base_args(str(f), rules) + ["-t"])
    assert hits == sorted(exp) and int(stats["Matches"]) == 4 and "NOTE" not in p.stderr


def test_refused_combinations(gpu, tmp_path):
    rules = write_rules(tmp_path / "rules.ldb")
    path, _ = write_inputs(tmp_path)
    for flag in ("-c", "-n", "-W", "-A"):
        _, _, p = run(base_args(path, rules) + [flag], ok=False)
        assert p.returncode != 0 and "ERROR: -K cannot be combined with -c, -n, -W or -A" in p.stdout, flag
    _, _, p = run(base_args(path, rules) + ["-F"], ok=False)
    assert p.returncode != 0 and "ERROR: -K cannot be combined with -F" in p.stdout
    _, _, p = run([a for a in base_args(path, rules) if a != "-S"], ok=False)
    assert p.returncode != 0 and "ERROR: -K needs -S" in p.stdout
    bad = tmp_path / "bad.ldb"
    bad.write_text("0;aabb\n0&1|0;aabb;ccdd\n")
    _, _, p = run(base_args(path, str(bad)), ok=False)
    assert p.returncode != 0 and "bad.ldb:2: column 4:" in p.stderr
    _, _, p = run(base_args(path, str(tmp_path / "missing.ldb")), ok=False)
    assert p.returncode != 0 and "does not exist" in p.stdout
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-K file" in r.stdout and "NOT evaluated" in r.stdout


def test_file_larger_than_a_buffer(gpu, tmp_path):
    """a file of three buffers is cut: it is counted on stderr and gives no rule line, wherever its hits lie; the
    small files around it are whole, also the one that fills a buffer to its last chunk"""
    rules = write_rules(tmp_path / "rules.ldb")
    big = (b"Needle tail.end " + b"." * 1100 + b"HEAD Needle tail..end " + b"." * 1700 + b" only Needle tail.end")
    big += b"." * (2048 + 14 * B - 10 - len(big))
    small = b"HEAD only"
    assert len(small) <= B and len(big) == 2048 + 14 * B - 10
    path, files = write_inputs(tmp_path, [small, big, small, b"Needle tail.end"])
    hits, stats, p = run(base_args(path, rules))
    assert hits == [("t00.txt", 1, 0), ("t00.txt", 41, 0), ("t02.txt", 1, 0), ("t02.txt", 41, 0), ("t03.txt", 7, 0)]
    assert "NOTE: 1 texts are cut by a buffer border" in p.stderr and int(stats["Matches"]) == 5
    # with buffers that hold it, it is evaluated
    args = base_args(path, rules)
    args[args.index("-G") + 1] = "64"
    hits, _, p = run(args)
    assert ("t01.txt", 7, 0) in hits and ("t01.txt", 1, 0) in hits and ("t01.txt", 41, 0) in hits and "NOTE" not in p.stderr
