"""acm_grep -C N[,M] -T dir [-V]: the lines that hold a record (-V: that hold none) with their context, found, grouped
and packed on the device per buffer, every input file's lines written under the directory of -T.  The files are
those of the model (tests/extract_model.py) over each file's own lines and, where grep is installed, what
grep -F -f prints for the file; stdout is what the run without the three flags prints."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import extract_model as xm
from test_gpu_acm_grep import CLI
from test_gpu_rewrite_cli import read_dir, stable
from test_gpu_select_cli import run

pytestmark = pytest.mark.gpu

PATS = [b"needle", b"hay", b"pin"]
WORDS = [b"needle", b"hay", b"straw", b"pin", b"x", b"", b"nee dle", b"chaff chaff", b"pi n"]
GREP = shutil.which("grep")


def make_lines(seed, lines, hit=0.12):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(lines):
        words = [WORDS[int(i)] for i in rng.integers(4, len(WORDS), size=int(rng.integers(0, 5)))]
        if rng.random() < hit:
            words.insert(int(rng.integers(0, len(words) + 1)), PATS[int(rng.integers(len(PATS)))])
        out.append(b" ".join(words))
    return out


def write_inputs(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    files = {
        "a.txt": b"\n".join(make_lines(1, 40)) + b"\n",
        "b_open.txt": b"\n".join(make_lines(2, 30)) + b"\nthe last line has a needle and no newline",
        "c_empty.txt": b"",
        "d_none.txt": b"\n".join(make_lines(3, 25, hit=0)) + b"\n",
        "e_open.txt": b"hay first\n" + b"\n".join(make_lines(4, 35)) + b"\nno match here, no newline",
        "f.txt": b"\n\n\n" + b"\n".join(make_lines(5, 20, hit=0.5)) + b"\n\n",
        "g_one.txt": b"pin",
    }
    for name, data in files.items():
        (d / name).write_bytes(data)
    assert sum(len(x) for x in files.values()) < 4096
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"".join(p + b"\n" for p in PATS))
    order = os.listdir(str(d))                        # readdir order, as acm_grep walks it
    return str(d), str(pats), [(name, files[name]) for name in order]


def occurrences(t):
    out = set()
    for p in PATS:
        at = t.find(p)
        while at >= 0:
            out.add(at + len(p) - 1)
            at = t.find(p, at + 1)
    return sorted(out)


def expected(files, before, after, invert):
    """{file name: its lines}: the model over every file alone, the records those of the worker's stream"""
    stream = b"".join(t for _, t in files)
    offs = np.asarray(occurrences(stream), dtype=np.int64)
    out, base = {}, 0
    for name, t in files:
        mine = offs[(offs >= base) & (offs < base + len(t))] - base
        assert mine.tolist() == occurrences(t), "a match spans two files: the files of this test must not make one"
        out[name] = xm.grep_like(t, mine, before, after, invert)[0]
        base += len(t)
    return out


def grep_file(path, pats, before, after, invert):
    cmd = [GREP, "-a", "-F", "-f", pats]
    if before + after > 0:
        cmd += ["-B", str(before), "-A", str(after)]
    if invert:
        cmd.append("-v")
    r = subprocess.run(cmd + [path], capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=60)
    assert r.returncode in (0, 1), r.stderr
    return r.stdout


CASES = [("0", 0, 0, False), ("2", 2, 2, False), ("1,3", 1, 3, False), ("0", 0, 0, True), ("2,1", 2, 1, True)]


@pytest.mark.parametrize("arg,before,after,invert", CASES, ids=["-C0", "-C2", "-C1,3", "-C0-V", "-C2,1-V"])
def test_extract_cli(gpu, tmp_path, arg, before, after, invert):
    path, pats, files = write_inputs(tmp_path)
    exp = expected(files, before, after, invert)
    assert exp["c_empty.txt"] == b"" and (exp["d_none.txt"] == b"") != invert
    assert sum(1 for v in exp.values() if v) >= 4
    if before + after and not invert:
        assert any(b"\n--\n" in v for v in exp.values())
    out = tmp_path / "out" / "deep"
    base = ["-f", path, "-p", pats, "-B", "64", "-D", "0", "-G", "256", "-L", "64", "-w", "1", "-R", "128", "-v"]
    hits, stats, p = run(base + ["-C", arg, "-T", str(out)] + (["-V"] if invert else []))
    got = read_dir(str(out))
    assert sorted(got) == sorted(exp)
    for name in exp:
        assert got[name] == exp[name], name
        if GREP:
            assert got[name] == grep_file(os.path.join(path, name), pats, before, after, invert), name
    _, _, plain = run(base)
    assert stable(p.stdout) == stable(plain.stdout) and len(hits) > 10 and p.stderr == plain.stderr
    # a second run over the same directory replaces the files
    run(base + ["-C", arg, "-T", str(out)] + (["-V"] if invert else []))
    assert read_dir(str(out)) == got


def test_composes_with_the_passes_in_front(gpu, tmp_path):
    """-S, -n and -o change the records, not the lines that hold one: the same files"""
    path, pats, files = write_inputs(tmp_path)
    exp = expected(files, 1, 1, False)
    base = ["-f", path, "-p", pats, "-B", "64", "-D", "0", "-G", "256", "-L", "64", "-w", "1", "-R", "128"]
    for k, flags in enumerate((["-S"], ["-n"], ["-o"], ["-A", "-c"])):
        out = tmp_path / ("out%d" % k)
        run(base + flags + ["-C", "1", "-T", str(out)])
        assert read_dir(str(out)) == exp, flags


def test_a_file_cut_across_buffers_is_an_error(gpu, tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    (d / "long.txt").write_bytes(b"\n".join(make_lines(9, 400)) + b"\n")
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"".join(p + b"\n" for p in PATS))
    out = tmp_path / "out"
    p = subprocess.run([CLI, "-f", str(d), "-p", str(pats), "-B", "64", "-D", "0", "-G", "16", "-L", "64", "-w", "1",
                        "-C", "1", "-T", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "ERROR: -C:" in p.stderr and "long.txt" in p.stderr and "is cut across two buffers" in p.stderr
    assert "-G/-B" in p.stderr
