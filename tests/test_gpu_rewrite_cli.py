"""acm_grep -r -O: the matches -o selects replaced on the device, buffer by buffer, and every input file written,
rewritten, under the directory of -O.  The files are those of the model (tests/rewrite_model.py) over the records the
select model leaves for every buffer of the worker's stream; stdout is what -o alone prints."""
import os

import numpy as np
import pytest

import rewrite_model as rw
import select_model as sel
from test_gpu_select_cli import B, PATS, entries, make_file, run, write_inputs

pytestmark = pytest.mark.gpu

#        a    ab         abc          bc    bcd            cd    dddd  Needle        ab-cd     cd-a
REPL = [b"", b"<AB>", ("fill", 0x2A), None, b"0123456789", b"C", b"#", ("fill", 0x58), b"ab+cd", None]


def repl_file(tmp_path):
    lines = [b"# pattern, replacement"]
    for i, r in enumerate(REPL):
        if isinstance(r, tuple):
            lines.append(b"%d fill %02x" % (i, r[1]))
        elif r is not None:
            lines.append(b"%d %s" % (i, r.hex().encode()))
    f = tmp_path / "repl.txt"
    f.write_bytes(b"\n".join(lines) + b"\n")
    return str(f)


def expected_files(files, G, segmented=False, nocase=False, words=False):
    """{file name: rewritten bytes}: every buffer of G chunks of the worker's stream selected and rewritten alone, its
    output cut where another file begins; and the number of buffers"""
    texts = [t for _, t in files]
    stream = b"".join(texts)
    bounds = np.cumsum([0] + [len(t) for t in texts])
    chunk_starts = [int(bounds[f]) + k for f, t in enumerate(texts) for k in range(0, len(t), B)]
    cuts = chunk_starts[::G] + [int(bounds[-1])]
    cells, offs = entries(texts if segmented else [stream], nocase, words)
    lens = [len(p) for p in PATS]
    select = sel.SelectModel(lens)
    model = rw.RewriteModel(lens, [None if r is None else (bytes([r[1]]), True) if isinstance(r, tuple) else (r, False)
                                   for r in REPL])
    out = {os.path.basename(f): b"" for f, _ in files}
    for lo, hi in zip(cuts, cuts[1:]):
        inside = (offs >= lo) & (offs < hi)
        ep, eo, _, _ = select.run(cells[inside], offs[inside] - lo, 0)
        first = int(np.searchsorted(bounds, lo, side="right")) - 1
        starts = [lo] + [int(x) for x in bounds[first + 1:-1] if x < hi]
        data, info, _, seg = model.run(stream[lo:hi], ep, eo, seg_start=[s - lo for s in starts])
        for k, s in enumerate(starts):
            f = int(np.searchsorted(bounds, s, side="right")) - 1
            out[os.path.basename(files[f][0])] += data[seg[k]:seg[k + 1] if k + 1 < len(seg) else len(data)]
    return out, len(cuts) - 1


def stable(stdout):
    return [l for l in stdout.splitlines() if not l.startswith(("Time (secs)", "Throughput"))]


def read_dir(d):
    return {e: open(os.path.join(d, e), "rb").read() for e in os.listdir(d)}


CASES = [[], ["-S"], ["-i"], ["-S", "-W"]]


@pytest.mark.parametrize("flags", CASES, ids=["plain", "-S", "-i", "-S-W"])
def test_rewrite_cli(gpu, tmp_path, flags):
    path, pats, files = write_inputs(tmp_path, [(1, 300), (2, 290), (3, 310)])
    exp, buffers = expected_files(files, 16, "-S" in flags, "-i" in flags, "-W" in flags)
    assert buffers == 1 and all(exp[os.path.basename(f)] != t for f, t in files)
    out = tmp_path / "out" / "deep"
    base = ["-f", path, "-p", pats, "-B", str(B), "-D", "0", "-G", "16", "-L", "64", "-w", "1", "-R", "128", "-v", "-o"] + flags
    hits, stats, p = run(base + ["-r", repl_file(tmp_path), "-O", str(out)])
    assert read_dir(str(out)) == exp
    _, only_stats, only = run(base)
    assert stable(p.stdout) == stable(only.stdout) and len(hits) > 30 and p.stderr == only.stderr
    # -o is implied
    out2 = tmp_path / "out2"
    base.remove("-o")
    _, _, q = run(base + ["-r", repl_file(tmp_path), "-O", str(out2)])
    assert read_dir(str(out2)) == exp and stable(q.stdout) == stable(p.stdout)


def test_cut_file_and_empty_file(gpu, tmp_path):
    """one file of 48 chunks in buffers of 16, matches across both cuts: it is rewritten piece by piece, the match
    across a cut is not rewritten and the NOTE counts it; a file of no bytes comes out as one"""
    t = bytearray(make_file(7, 3072))
    for cut in (1024, 2048):
        t[cut - 2:cut + 2] = b"abcd"
    d = tmp_path / "in"
    d.mkdir()
    (d / "cut.txt").write_bytes(bytes(t))
    (d / "none.txt").write_bytes(b"")
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"".join(p + b"\n" for p in PATS))
    files = [(str(d / "cut.txt"), bytes(t))]
    exp, buffers = expected_files(files, 16)
    whole = expected_files(files, 48)[0]
    assert buffers == 3 and whole != exp
    exp["none.txt"] = b""
    out = tmp_path / "out"
    args = ["-f", str(d), "-p", str(pats), "-B", str(B), "-D", "0", "-G", "16", "-L", "64", "-w", "1", "-R", "128",
            "-r", repl_file(tmp_path), "-O", str(out)]
    _, stats, p = run(args)
    assert read_dir(str(out)) == exp
    assert len([l for l in p.stderr.splitlines() if l.startswith("NOTE:")]) == 1
    # a second run over the same directory replaces the files
    run(args)
    assert read_dir(str(out)) == exp


def test_output_that_does_not_fit(gpu, tmp_path):
    """a buffer whose output outgrows the device buffer is an error that names the file, never a cut file"""
    d = tmp_path / "in"
    d.mkdir()
    (d / "grow.txt").write_bytes(b"a" * 4096)
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"a\n")
    repl = tmp_path / "repl.txt"
    repl.write_bytes(b"0 " + b"41" * 200 + b"\n")
    import subprocess
    from test_gpu_acm_grep import CLI
    p = subprocess.run([CLI, "-f", str(d), "-p", str(pats), "-B", "64", "-D", "0", "-G", "64", "-L", "64", "-w", "1",
                        "-r", str(repl), "-O", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "ERROR: -r:" in p.stderr and "grow.txt" in p.stderr
