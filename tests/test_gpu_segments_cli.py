"""acm_grep -S: every input unit is its own text (a file; with -t a line).  Without -S a worker scans
its files as one stream and reports a signature that straddles two of them; with -S the matches are
those of the oracle scanning every file (line) alone."""
import os

import numpy as np
import pytest

import fixtures
import orc
from test_gpu_acm_grep import CLI, run

pytestmark = pytest.mark.gpu


def keys(hits):
    """file, pattern id, offset in the chunk: the same whether a file is scanned alone or after another"""
    return sorted((os.path.basename(h[2]), h[0], int(h[4])) for h in hits)


def alone(args, files):
    """-v lines of acm_grep run on every file by itself, without -S: the serial scan of that file"""
    out = []
    for p, _ in files:
        hits, _, _ = run(CLI, ["-f", p] + args)
        out += hits
    return keys(out)


def write_pair(tmp_path, sig, cut, seed):
    pats = fixtures.patterns_of("clamav2000_m12")
    t = fixtures.text_for({"kind": "clamav", "n": 50000, "seed": seed, "n_plant": 30}, pats)
    a = np.concatenate([t[:20000], np.frombuffer(sig[:cut], dtype=np.uint8)])
    b = np.concatenate([np.frombuffer(sig[cut:], dtype=np.uint8), t[20000:]])
    pa, pb = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    open(pa, "wb").write(a.tobytes())
    open(pb, "wb").write(b.tobytes())
    return [(pa, a), (pb, b)]


def test_files_are_separate_texts(gpu, tmp_path):
    name = "clamav2000_m12"
    o = fixtures.oracle_for(name)
    sigs = orc.clamav_file(2000, str(tmp_path))
    sig = o.pattern(5)[0]
    files = write_pair(tmp_path, sig, len(sig) // 2, 3)
    args = ["-f", ",".join(f for f, _ in files), "-p", sigs, "-x", "-m", "12", "-B", "4096", "-D", "0", "-G", "32",
            "-L", "256", "-w", "1", "-R", "64", "-v"]
    joined = np.concatenate([t for _, t in files])
    serial = o.scan(joined)[0].size
    per_file = sum(o.scan(t)[0].size for _, t in files)
    assert serial > per_file   # the straddling signature
    hits, stats, _ = run(CLI, args)
    assert int(stats["Matches"]) == serial   # the default is unchanged
    hits, stats, _ = run(CLI, args + ["-S"])
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == per_file
    assert keys(hits) == alone(args[2:], files)


def test_file_larger_than_a_buffer(gpu, tmp_path):
    name = "clamav2000_m12"
    o = fixtures.oracle_for(name)
    sigs = orc.clamav_file(2000, str(tmp_path))
    pats = fixtures.patterns_of(name)
    t = fixtures.text_for({"kind": "clamav", "n": 200000, "seed": 9, "n_plant": 60}, pats)
    sig = np.frombuffer(o.pattern(7)[0], dtype=np.uint8)
    buf = 16 * 4096   # (-G is rounded up to a multiple of 16)
    for cut in (buf, 2 * buf, 3 * buf):   # a signature across the buffer cuts
        t[cut - 5:cut - 5 + sig.size] = sig
    files = [(str(tmp_path / "big.bin"), t), (str(tmp_path / "small.bin"), t[:5000].copy())]
    for p, x in files:
        open(p, "wb").write(x.tobytes())
    args = ["-f", ",".join(p for p, _ in files), "-p", sigs, "-x", "-m", "12", "-B", "4096", "-D", "0", "-G", "4",
            "-L", "256", "-w", "1", "-R", "64", "-v", "-S"]
    hits, stats, _ = run(CLI, args)
    assert int(stats["Kernel launches"]) >= 4
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == sum(o.scan(x)[0].size for _, x in files)
    assert keys(hits) == alone(args[2:-1], files)


def test_text_mode_lines(gpu, tmp_path):
    pats = [b"abc", b"c\nx", b"b\n", b"\nab", b"qwertyuiop", b"\n"]
    pfile = tmp_path / "pats.txt"
    pfile.write_bytes(b"".join(p.hex().encode() + b"\n" for p in pats))
    o = orc.Oracle()
    for i, p in enumerate(pats):
        o.add(p, i)
    o.compile()
    rng = np.random.default_rng(2)
    lines = []
    for i in range(400):
        n = int(rng.integers(0, 40))
        body = bytes(rng.choice(list(b"abcxyz "), n).tolist())
        if i % 50 == 7:   # longer than -B: split over chunks, the signature across the split
            body = b"z" * 58 + b"qwertyuiop" + b"y" * 150
        lines.append(body + b"\n")
    text = b"".join(lines)
    path = str(tmp_path / "lines.txt")
    open(path, "wb").write(text)
    args = ["-f", path, "-p", str(pfile), "-x", "-B", "64", "-D", "0", "-G", "32", "-L", "64", "-w", "1",
            "-R", "16", "-t", "-v"]
    per_line = sum(o.scan(np.frombuffer(ln, dtype=np.uint8))[0].size for ln in lines)
    serial = o.scan(np.frombuffer(text, dtype=np.uint8))[0].size
    assert serial > per_line
    _, stats, _ = run(CLI, args)
    assert int(stats["Matches"]) == serial
    hits, stats, _ = run(CLI, args + ["-S"])
    assert int(stats["Matches"]) == per_line
    assert int(stats["Matches reported"]) == per_line
    # (lines quoting a pattern with a newline in it do not parse; the one across the chunk split does)
    assert sum(h[1] == "qwertyuiop" for h in hits) == text.count(b"qwertyuiop")


def test_every_pattern(gpu, tmp_path):
    name = "sentiment"
    o = fixtures.oracle_for(name)
    path, hx, max_len = fixtures.set_source(name)
    files = []
    for i in range(3):
        t = fixtures.text_for({"kind": "words", "n": 30000 + 77 * i, "seed": 12 + i}, [])
        p = str(tmp_path / ("w%d.txt" % i))
        open(p, "wb").write(t.tobytes())
        files.append((p, t))
    args = ["-f", ",".join(p for p, _ in files), "-p", path, "-B", "4096", "-D", "0", "-G", "4", "-L", "256",
            "-w", "1", "-R", "64", "-A", "-S"]
    _, stats, _ = run(CLI, args)
    assert int(stats["Matches"]) == sum(o.scan_all(t)[0].size for _, t in files)
