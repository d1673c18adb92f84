"""acm_grep -C N[,M] -T dir [-V] with -H, -N and -b: the file's name, the line's number and its offset in front of every
extracted line, made on the device per buffer by the per-line context pass and the format pass.  The files are those
of the model (tests/format_model.py) over each file's own lines and, where grep is installed, what grep -H -n -b prints
for the file; without the three flags the files are the extract's (tests/extract_model.py), byte for byte."""
import os
import subprocess

import pytest

import format_model as fm
from test_gpu_acm_grep import CLI
from test_gpu_extract_cli import GREP, expected, occurrences, write_inputs
from test_gpu_rewrite_cli import read_dir, stable
from test_gpu_select_cli import run

pytestmark = pytest.mark.gpu

SUBSETS = [[f for k, f in enumerate(("-H", "-N", "-b")) if s >> k & 1] for s in range(8)]


def expected_prefixed(path, files, before, after, invert, flags):
    out = {}
    for name, t in files:
        out[name] = fm.grep_like(t, occurrences(t), before, after, invert, names=[os.path.join(path, name).encode()],
                                 with_name="-H" in flags, line_number="-N" in flags, byte_offset="-b" in flags)[0]
    return out


def grep_file(path, pats, before, after, invert, flags):
    cmd = [GREP, "-a", "-F", "-f", pats] + [{"-H": "-H", "-N": "-n", "-b": "-b"}[f] for f in flags] + ([] if "-H" in flags else ["-h"])
    if before + after > 0:
        cmd += ["-B", str(before), "-A", str(after)]
    if invert:
        cmd.append("-v")
    r = subprocess.run(cmd + [path], capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=60)
    assert r.returncode in (0, 1), r.stderr
    return r.stdout


CASES = [("0", 0, 0, False), ("2", 2, 2, False), ("1,3", 1, 3, False), ("0", 0, 0, True), ("2", 2, 2, True), ("1,3", 1, 3, True)]


@pytest.mark.parametrize("arg,before,after,invert", CASES, ids=["-C0", "-C2", "-C1,3", "-C0-V", "-C2-V", "-C1,3-V"])
def test_prefixes_cli(gpu, tmp_path, arg, before, after, invert):
    path, pats, files = write_inputs(tmp_path)
    plain = expected(files, before, after, invert)
    base = ["-f", path, "-p", pats, "-B", "64", "-D", "0", "-G", "256", "-L", "64", "-w", "1", "-R", "128", "-v"]
    _, _, bare = run(base)
    for k, flags in enumerate(SUBSETS):
        exp = expected_prefixed(path, files, before, after, invert, flags) if flags else plain
        out = tmp_path / ("out%d" % k)
        hits, stats, p = run(base + ["-C", arg, "-T", str(out)] + flags + (["-V"] if invert else []))
        got = read_dir(str(out))
        assert sorted(got) == sorted(exp)
        for name in exp:
            assert got[name] == exp[name], (name, flags)
            if GREP:
                assert got[name] == grep_file(os.path.join(path, name), pats, before, after, invert, flags), (name, flags)
        assert got["c_empty.txt"] == b"" and (got["d_none.txt"] == b"") != invert
        assert stable(p.stdout) == stable(bare.stdout) and p.stderr == bare.stderr, flags
    full = read_dir(str(tmp_path / "out7"))
    name = os.path.join(path, "g_one.txt").encode()
    assert full["g_one.txt"] == (b"" if invert else name + b":1:0:pin\n")
    if before + after and not invert:
        assert any(b"\n--\n" in v for v in full.values()) and any(b".txt-" in v for v in full.values())


def test_a_list_of_files_keeps_the_names_given(gpu, tmp_path):
    """the name is the path as -f resolved it, also when the working directory makes it a relative one"""
    path, pats, files = write_inputs(tmp_path)
    out = tmp_path / "out"
    p = subprocess.run([CLI, "-f", "in", "-p", pats, "-B", "64", "-D", "0", "-G", "256", "-L", "64", "-w", "1", "-C", "0", "-T", str(out),
                        "-H", "-N"], capture_output=True, cwd=str(tmp_path), timeout=120)
    assert p.returncode == 0, p.stderr
    got = read_dir(str(out))
    for name, t in files:
        exp = fm.grep_like(t, occurrences(t), names=[b"in/" + name.encode()], with_name=True, line_number=True)[0]
        assert got[name] == exp, name
    assert got["g_one.txt"] == b"in/g_one.txt:1:pin\n"
