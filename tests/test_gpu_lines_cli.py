"""acm_grep -n: the -v line names the 1-based line of the match's last byte in its file, STATS counts
the newlines.  The expected lines come from the oracle's records over every worker's stream and the file
bytes; the lines are found on the device, buffer by buffer, chained through d_prev_info."""
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import fixtures
import word_model as wm
from test_gpu_acm_grep import CLI, run

pytestmark = pytest.mark.gpu

NLINE = re.compile(r"^Pattern (-?\d+) \('(.*)'\) found in file '(.*)' at line (\d+) offset (\d+) \[relative: (-?\d+)\]$")
NAME = "sentiment"


def make_files(tmp_path):
    """a directory: a file larger than a buffer, files with and without a trailing newline, an empty one"""
    d = tmp_path / "inputs"
    d.mkdir()
    files = {}
    sizes = (150000, 30011, 0, 20000, 7, 41000, 12345)
    for i, n in enumerate(sizes):
        t = fixtures.text_for({"kind": "words", "n": max(n, 16), "seed": 60 + i}, [])[:n].copy()
        sp = np.flatnonzero(t == 0x20)
        t[sp[np.random.default_rng(i).random(sp.size) < 0.06]] = 0x0A
        if n:
            t[n - 1] = 0x0A if i % 2 else 0x61
        (d / ("f%d.txt" % i)).write_bytes(t.tobytes())
        files[str(d / ("f%d.txt" % i))] = t
    order = [os.path.join(str(d), e) for e in os.listdir(str(d))]   # readdir order: how acm_grep deals them
    return str(d), files, order


def expected(files, order, workers, records):
    """Counter of (file, iid, line): records(stream) -> (offsets, pattern indices) over each worker's stream"""
    o = fixtures.oracle_for(NAME)
    out = Counter()
    for w in range(workers):
        mine = order[w::workers]
        if not mine:
            continue
        stream = np.concatenate([files[f] for f in mine])
        begins = np.cumsum([0] + [files[f].size for f in mine])
        offs, pats = records(stream, begins[:-1])
        for x, p in zip(np.asarray(offs, dtype=np.int64).tolist(), np.asarray(pats).tolist()):
            k = int(np.searchsorted(begins, x, side="right")) - 1
            f = mine[k]
            out[(f, o.pattern(p)[1], 1 + bytes(files[f][:x - begins[k]]).count(b"\n"))] += 1
    return out


def grep(args):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=180, errors="replace")
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    hits = Counter((m.group(3), int(m.group(1)), int(m.group(4))) for m in map(NLINE.match, p.stdout.splitlines()) if m)
    stats = dict(re.findall(r"^([A-Za-z ()]+):\s+([\d.]+)$", p.stdout, flags=re.M))
    return hits, stats, p.stdout


def base_args(d, workers):
    path, _, _ = fixtures.set_source(NAME)
    return ["-f", d, "-p", path, "-B", "4096", "-D", "0", "-G", "16", "-L", "256", "-w", str(workers), "-R", "2048"]


@pytest.mark.parametrize("workers", [1, 3])
def test_line_numbers(gpu, tmp_path, workers):
    d, files, order = make_files(tmp_path)
    o = fixtures.oracle_for(NAME)
    newlines = sum(bytes(t).count(b"\n") for t in files.values())
    args = base_args(d, workers)
    hits, stats, out = grep(args + ["-n", "-v"])
    exp = expected(files, order, workers, lambda s, b: o.scan(s)[:2])
    assert sum(exp.values()) > 5000
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == sum(exp.values())
    assert hits == exp
    assert int(stats["Processed lines"]) == newlines
    assert int(stats["Kernel launches"]) >= sum(t.size for t in files.values()) // (16 * 4096)   # files span buffers
    # every file on its own text
    hits, stats, _ = grep(args + ["-n", "-v", "-S"])
    assert hits == expected(files, order, workers, lambda s, b: fixtures_segments(o, s, b))
    assert int(stats["Processed lines"]) == newlines
    # whole words
    model = wm.WordModel(NAME)
    hits, stats, _ = grep(args + ["-n", "-v", "-W"])
    assert hits == expected(files, order, workers, lambda s, b: model.words(s)[:2])
    assert int(stats["Processed lines"]) == newlines
    # counts: the lines of -c are those of a run without -n, the match lines carry the line numbers
    hits, stats, out = grep(args + ["-n", "-v", "-c"])
    assert hits == exp and int(stats["Processed lines"]) == newlines
    _, _, plain = grep(args + ["-c"])
    count_lines = lambda text: sorted(l for l in text.splitlines() if l.startswith("Count "))
    assert count_lines(out) == count_lines(plain) and len(count_lines(out)) > len(order)


def fixtures_segments(o, stream, begins):
    from test_host_segments import oracle_segments
    r = oracle_segments(o, stream, begins)
    return r[0], r[1]


def test_text_mode_is_refused(gpu, tmp_path):
    d, files, order = make_files(tmp_path)
    p = subprocess.run([CLI] + base_args(d, 1) + ["-n", "-t"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "ERROR: -n needs binary mode: -t already makes every line a chunk" in p.stdout
    assert "Usage:" in p.stdout


def test_without_n_stdout_is_unchanged(gpu, tmp_path):
    """the strings the existing CLI tests pin: the -v line without a line number, no Processed lines"""
    d, files, order = make_files(tmp_path)
    o = fixtures.oracle_for(NAME)
    hits, stats, out = run(CLI, base_args(d, 1) + ["-v"])
    stream = np.concatenate([files[f] for f in order])
    offs, pats, _ = o.scan(stream)
    assert len(hits) == offs.size == int(stats["Matches"]) == int(stats["Matches reported"])
    assert " at line " not in out and "Processed lines" not in out
    # the STATS block: the keys of a binary-mode run as test_gpu_acm_grep.py reads them, in order, nothing else
    block = out[out.index("-------------- STATS --------------"):]
    assert re.findall(r"^([A-Za-z ()]+):", block, flags=re.M) == [
        "Matches", "Matches reported", "Time (secs)", "Automaton states", "Automaton size (MB)", "Processed bytes",
        "Processed files", "Kernel launches", "Throughput (Mbps)"]
    assert int(stats["Processed bytes"]) == stream.size and int(stats["Processed files"]) == len(order)
    begins = np.cumsum([0] + [files[f].size for f in order])
    want = []
    for x, p in zip(offs.astype(np.int64).tolist(), pats.tolist()):
        k = int(np.searchsorted(begins, x, side="right")) - 1
        in_file = x - begins[k]
        want.append((str(o.pattern(p)[1]), o.pattern(p)[0].decode(), order[k], in_file % 4096 + 1))
    # (offset: in the worker's buffer, pinned by test_gpu_acm_grep.py; relative: in the chunk)
    assert [(h[0], h[1], h[2], int(h[4])) for h in hits] == want
