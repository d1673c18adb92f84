"""acm_grep -Q FILE -E -X and -K FILE -E -X: alternatives of more than one byte.  The stdout lines are those that
Python's re finds in the files through the translation of tests/group_model.py (every file its own text with -S;
the printed offset is where the match ends); the same files without -X are refused, naming line and column; -X
without -E is refused; -h shows -X."""
import os
import subprocess

import pytest

import group_model as gm
import test_gpu_rules_cli as rc
from test_gpu_acm_grep import CLI
from test_gpu_sequences_cli import B, base_args, lines_of, run
from test_gpu_wildcards_cli import write_inputs as write_texts

pytestmark = pytest.mark.gpu

SIGS = [(7, "aa(bbcc|ddee)ff*!(0102|0304)11"),           # the body of the issue
        (None, "4e65(6564|4544)6c65"),                   # Ne(ed|ED)le: no id, so the sequence index (1)
        (40, "(6162|6263)63{1-2}64!(2e2e2e)67"),         # (ab|bc)c {1-2} d, not "...", g
        (41, "48454144")]                                # HEAD
TEXTS = [bytes.fromhex("aabbccff00010311") + b" Needle NeEDle NeEdle", bytes.fromhex("aaddeeff010211aabbccff03041111"),
         b"abc.d...g abc..d.-.g bcc.d,,,g abcd___g", b"", b"HEAD abcc.dxyzg NeEDle" + bytes.fromhex("aabbcdff0000000011"),
         bytes.fromhex("aabbccff0102110304110103") + b"HEAD", b"bcc..d1.2g abc...d123g"]


def expected(files):
    out = []
    for f, t in files:
        assert len(t) < B
        for k, (iid, body) in enumerate(SIGS):
            out += [(os.path.basename(f), k if iid is None else iid, o) for o in gm.regex_ends(body, t)]
    return sorted(out)


def test_signatures_with_groups(gpu, tmp_path):
    _, path, files = write_texts(tmp_path, TEXTS)
    q = tmp_path / "groups.sig"
    q.write_text("# signatures\n" + "".join(("%d:%s\n" % s) if s[0] is not None else s[1] + "\n" for s in SIGS))
    exp = expected(files)
    assert {i for _, i, _ in exp} == {7, 1, 40, 41} and len(exp) >= 10
    assert ("t0.txt", 7, 7) in exp and ("t1.txt", 7, 14) in exp and ("t1.txt", 7, 13) not in exp
    hits, stats, p = run(base_args(path, str(q)) + ["-E", "-X", "-S"])
    assert lines_of(hits) == exp and int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    assert "NOTE" not in p.stderr
    # the same file without -X is refused whole, naming the line and the column
    _, _, p = run(base_args(path, str(q)) + ["-E", "-S"], ok=False)
    assert p.returncode != 0 and "groups.sig:2: column 8:" in p.stderr
    # -X is the syntax of -E
    _, _, p = run(base_args(path, str(q)) + ["-X", "-S"], ok=False)
    assert p.returncode != 0 and "ERROR: -X needs -E" in p.stdout
    _, _, p = run(base_args(path, str(q)) + ["-E", "-X", "-W"], ok=False)
    assert p.returncode != 0 and "ERROR: -E cannot be combined with -W" in p.stdout
    bad = tmp_path / "bad.txt"
    bad.write_text("aa(0102|0304)\naa(bbcc|dd)\n")
    _, _, p = run(base_args(path, str(bad)) + ["-E", "-X"], ok=False)
    assert p.returncode != 0 and "bad.txt:2: column 9:" in p.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-X   " in r.stdout and "(aabb|ccdd)" in r.stdout


def test_rules_with_groups(gpu, tmp_path):
    rules = [(5, "0&1", ["aa(bbcc|ddee)ff", "!(0102|0304)11"]), (None, "0>1", ["4e65(6564|4544)6c65"]),
             (9, "0&1=0", ["(6162|6263)63", "48454144"])]
    ldb = rc.write_rules(tmp_path / "rules.ldb", rules)
    path, files = rc.write_inputs(tmp_path, TEXTS)
    truth = [lambda c: c[0] > 0 and c[1] > 0, lambda c: c[0] > 1, lambda c: c[0] > 0 and c[1] == 0]
    exp = []
    for f, t in files:
        for k, (iid, _, bodies) in enumerate(rules):
            if truth[k]([len(gm.regex_ends(b, t)) for b in bodies]):
                exp.append((os.path.basename(f), k if iid is None else iid, 0))
    exp.sort()
    assert {i for _, i, _ in exp} == {5, 1, 9} and len(exp) >= 5
    hits, stats, p = rc.run(rc.base_args(path, ldb) + ["-E", "-X"])
    assert hits == exp and int(stats["Matches"]) == len(exp) and "NOTE" not in p.stderr
    _, _, p = rc.run(rc.base_args(path, ldb) + ["-E"], ok=False)            # the syntax needs -X
    assert p.returncode != 0 and "rules.ldb:3: column" in p.stderr
    _, _, p = rc.run(rc.base_args(path, ldb) + ["-X"], ok=False)
    assert p.returncode != 0 and "ERROR: -X needs -E" in p.stdout
