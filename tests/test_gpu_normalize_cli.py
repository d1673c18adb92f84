"""acm_grep -S -z SPEC: every buffer normalised on the device, scanned normalised, the records mapped back.  The
expectation is acm_grep -S itself over the same files normalised by the model (tests/normalize_model.py), its offsets
carried through the model's map; the counts of -c are equal as they are."""
import os
import re

import numpy as np
import pytest

import normalize_model as nm
from test_gpu_select_cli import CLI, LINE, run

pytestmark = pytest.mark.gpu

PATS = [b"a href", b"href", b"a b", b"A", b" b", b"%41", b"javascript:"]
TOKENS = [b"a", b" ", b"  ", b"\t", b"\n", b"%20", b"%09", b"%41", b"%4", b"%", b"href", b"b", b"A", b"a href", b"a%20href",
          b"Java", b"script:", b"java\tscript:", b"x", b"%2541", b"\r\n"]
SPECS = {"url": (nm.PERCENT, None), "ws": (nm.SQUEEZE, None), "strip": (nm.STRIP, None), "nul": (nm.STRIP, b"\0"),
         "url,ws": (nm.PERCENT | nm.SQUEEZE, None), "strip,url": (nm.PERCENT | nm.STRIP, None)}
COUNT = re.compile(r"^Count (file|pattern) (.*): (\d+)$")


def make_file(seed, size):
    rng = np.random.default_rng(seed)
    out = b""
    while len(out) < size:
        out += TOKENS[int(rng.integers(len(TOKENS)))]
    return out[:size]


def write_dir(d, files):
    d.mkdir()
    for name, data in files.items():
        (d / name).write_bytes(data)
    return str(d)


def base_args(path, pats, extra):
    # (a chunk holds a whole file: the relative offset of the -v line is the offset in the file)
    return ["-f", path, "-p", pats, "-x", "-B", "1024", "-D", "0", "-G", "16", "-L", "64", "-w", "1", "-R", "1024", "-S"] + extra


def hit_set(hits):
    """(pattern id, file, the offset behind the match's last byte in its file)"""
    return sorted((int(iid), os.path.basename(f), int(rel)) for iid, _, f, _, rel in hits)


def counts(p, names):
    out = []
    for kind, what, n in (m.groups() for m in (COUNT.match(l) for l in p.stdout.splitlines()) if m):
        out.append((kind, os.path.basename(what.strip("'")) if kind == "file" else what.split(" ")[0], int(n)))
    return sorted(out)


@pytest.mark.parametrize("spec", sorted(SPECS))
@pytest.mark.parametrize("extra", [["-v"], ["-v", "-A"], ["-v", "-i"], ["-v", "-c", "-A"]], ids=["-v", "-A", "-i", "-c-A"])
def test_normalized_cli(gpu, tmp_path, spec, extra):
    flags, blanks = SPECS[spec]
    files = {"s%d.txt" % i: make_file(10 + i, 280 + 7 * i) for i in range(3)}
    files["wide.txt"] = "x a href A a b".encode("utf-16-le")
    norm = {k: nm.normalize(v, flags, blanks) for k, v in files.items()}
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"".join(p.hex().encode() + b"\n" for p in PATS))
    raw = write_dir(tmp_path / "raw", files)
    flat = write_dir(tmp_path / "flat", {k: x.out for k, x in norm.items()})
    hits, _, p = run(base_args(raw, str(pats), ["-z", spec] + extra))
    xhits, _, xp = run(base_args(flat, str(pats), extra))
    exp = sorted((iid, f, int(norm[f].last[off - 1]) + 1) for iid, f, off in hit_set(xhits))
    assert hit_set(hits) == exp and len(exp) > 10
    if "-c" in extra:
        assert counts(p, files) == counts(xp, files) and len(counts(p, files)) > 4


def test_nul_finds_ascii_in_utf16(gpu, tmp_path):
    files = {"wide.txt": "say needle twice: needle".encode("utf-16-le"), "plain.txt": b"a needle"}
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"needle".hex().encode() + b"\n")
    raw = write_dir(tmp_path / "raw", files)
    hits, _, _ = run(base_args(raw, str(pats), ["-v"]))
    assert hit_set(hits) == [(0, "plain.txt", 8)]
    hits, _, _ = run(base_args(raw, str(pats), ["-v", "-z", "nul"]))
    assert hit_set(hits) == [(0, "plain.txt", 8), (0, "wide.txt", 19), (0, "wide.txt", 47)]


# (the flag the ERROR line must name, the arguments that go with -z)
REFUSED = [("-n", ["-n"]), ("-C", ["-C", "1", "-T", "out"]), ("-T", ["-T", "out"]), ("-o", ["-o"]),
           ("-r", ["-r", "pats.txt", "-O", "out"]), ("-O", ["-O", "out"]), ("-H", ["-H"]), ("-N", ["-N"]), ("-b", ["-b"]),
           ("-k", ["-k", "1"]), ("-e", ["-k", "1", "-e"]), ("-P", ["-P", "pats.txt"]), ("-Q", ["-Q", "pats.txt"]),
           ("-K", ["-K", "pats.txt"]), ("-E", ["-Q", "pats.txt", "-E"]), ("-X", ["-Q", "pats.txt", "-E", "-X"]),
           ("-V", ["-C", "1", "-T", "out", "-V"]), ("-F", ["-F"])]
BAD_SPECS = ("", "ws,strip", "url,url", "url,", "nul,ws", "html", "ws,nul,url")


def refusals(tmp_path):
    """(the start of the ERROR line that must be printed, returncode, stdout) of every refused combination, of the bad
    SPECs and of a missing -S"""
    import subprocess
    (tmp_path / "pats.txt").write_bytes(b"6162\n")
    base = base_args(str(tmp_path / "pats.txt"), str(tmp_path / "pats.txt"), ["-z", "url,ws"])
    out = []
    for flag, extra in REFUSED:
        args = base + [a if a not in ("pats.txt", "out") else str(tmp_path / a) for a in extra]
        p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        out.append(("ERROR: -z cannot be combined with %s:" % flag, p.returncode, p.stdout))
    for spec in BAD_SPECS:
        args = base[:base.index("-z") + 1] + [spec]
        p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
        out.append(("ERROR: -z takes a comma list", p.returncode, p.stdout))
    args = [a for a in base if a != "-S"]
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
    out.append(("ERROR: -z needs -S:", p.returncode, p.stdout))
    return out


def check_refusals(seen):
    assert len(seen) == len(REFUSED) + len(BAD_SPECS) + 1
    for line_start, rc, stdout in seen:
        assert rc != 0, line_start
        assert any(l.startswith(line_start) for l in stdout.splitlines()), (line_start, stdout[-600:])


def test_refused_combinations(gpu, tmp_path):
    check_refusals(refusals(tmp_path))
