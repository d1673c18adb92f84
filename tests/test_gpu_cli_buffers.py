"""acm_grep's file-writing modes (-o, -r -O, -C -T [-V], -H -N -b) over several buffers per worker, several workers and
the deferred passes of -W: the feeder loop, prepare(), submit(), finish() and the collect functions of csrc/acm_grep.cpp
in the shapes a real run has.  Chunks of 64 bytes and buffers of 16 chunks (acm_grep rounds -G up to a multiple of 16, as
the reference does: 16 is the smallest buffer there is): every worker fills four buffers, so each of its two buffer
objects is used twice and the second use has fewer file starts than the first.

The layout of every run is computed on the host (tests/cli_layout.py) and the files are those of the models over it; for
-C, -V, -H, -N and -b GNU grep over each file alone is the reference too, where it is installed (test_host_cli_layout.py
proves the model against it for these inputs on the host)."""
import collections
import os
import subprocess

import pytest

import cli_layout as lay
import test_gpu_extract_cli as xc
import test_gpu_format_cli as fc
import test_gpu_select_cli as sc
from test_gpu_acm_grep import CLI
from test_gpu_lines_cli import NLINE
from test_gpu_rewrite_cli import REPL, read_dir, repl_file, stable
from test_gpu_select_cli import run

pytestmark = pytest.mark.gpu

B, G = 64, 16
GREP = xc.GREP
LPATS = xc.PATS      # set L: needle, hay, pin
RPATS = sc.PATS      # set R: the overlapping patterns of the select and rewrite tests


def sized(seed, size, open_end, first=None, last=None, hit=0.12):
    """size bytes of lines of xc.make_lines (cut, or filled with 'z'): first in front, last behind; open_end: no newline
    at the end"""
    tail = (b"\n" + last if last else b"") + (b"" if open_end else b"\n")
    head = b"\n".join(([first] if first else []) + xc.make_lines(seed, size // 4 + 4, hit))[:size - len(tail)]
    head = head.ljust(size - len(tail), b"z")
    if open_end and not last and head.endswith(b"\n"):
        head = head[:-1] + b"z"
    t = head + tail
    assert len(t) == size and t.endswith(b"\n") != open_end
    return t


def groups_L(w):
    """worker w's four buffers of set L, (name, bytes) per file; sizes in chunks: 6 + 10, 16, sixteen of 1, 0 + 2"""
    s, n = 100 * (w + 1), "w%d_" % w
    g1 = [(n + "a6_open.txt", sized(s + 1, 5 * B + 22, True, first=b"hay first")),          # short tail in front of another file: unpacked, d_ex_text
          (n + "b10_open.txt", sized(s + 2, 9 * B + 44, True, first=b"pin in front", last=b"chaff straw\nchaff pin"))]
    g2 = [(n + "c16_full.txt", sized(s + 3, G * B, False, first=b"hay first", last=b"x straw\nthe last pin"))]   # packed, one start, no d_ex_text
    g3 = [(n + "d_byte.txt", b"z"),
          (n + "e_one.txt", b"pin"),
          (n + "f_64.txt", sized(s + 4, 64, False)),
          (n + "g_nl.txt", b"\n\n\n"),
          (n + "h_open.txt", sized(s + 5, 50, True, first=b"needle up front")),
          (n + "i_open_none.txt", sized(s + 6, 40, True, hit=0)),
          (n + "j_behind.txt", b"chaff x\nhay\nx")] + \
         [(n + "k%d.txt" % i, sized(s + 10 + i, 9 + 7 * i, i % 2 == 1, hit=0.3)) for i in range(8)] + \
         [(n + "l_open.txt", sized(s + 7, 60, True, first=b"pin one", last=b"x x\nstraw hay"))]
    g4 = [(n + "m_empty.txt", b""),
          (n + "n2_last.txt", sized(s + 8, 100, False, first=b" hay first", last=b"last needle"))]
    return [g1, g2, g3, g4]


def set_L(workers, single=False):
    """set L for that many workers, in the order of -f: worker w's list is its three full buffers, rotated by w so that
    the workers are not in step, and the short one last; the lists interleaved.  single: the same files in an order
    that one worker reads without cutting a file: every full buffer, then the short ones"""
    per = []
    for w in range(workers):
        g = groups_L(w)
        per.append(g[w % 3:3] + g[:w % 3] + g[3:])
    if single:
        return [f for g in per for grp in g[:3] for f in grp] + [f for g in per for f in g[3]]
    lists = [[f for grp in g for f in grp] for g in per]
    assert len({len(l) for l in lists}) == 1
    return [l[i] for i in range(len(lists[0])) for l in lists]


def groups_R(w):
    """worker w's files of set R: A of 10 chunks, B of 14 (6 in buffer 1, 8 in buffer 2), C of 24 (8 in buffer 2, all of
    buffer 3), an empty one, D of 3 alone in buffer 4.  "abcd" lies across both cuts, with a space in front: "ab" is a
    word but for the byte behind buffer 1; C ends in " ab" and D begins with a space: "ab" is a word for that byte"""
    s, n = 200 * (w + 1), "w%d_" % w
    a = sc.make_file(s + 1, 9 * B + 17)
    b = bytearray(sc.make_file(s + 2, 13 * B + 30))
    c = bytearray(sc.make_file(s + 3, 24 * B))
    d = bytearray(sc.make_file(s + 4, 2 * B + 5))
    b[6 * B - 3:6 * B + 2] = b" abcd"
    c[8 * B - 3:8 * B + 2] = b" abcd"
    c[-3:] = b" ab"
    d[:1] = b" "
    return [(n + "A.txt", a), (n + "B.txt", bytes(b)), (n + "C.txt", bytes(c)), (n + "E_empty.txt", b""), (n + "D.txt", bytes(d))]


def set_R(workers):
    lists = [groups_R(w) for w in range(workers)]
    return [l[i] for i in range(len(lists[0])) for l in lists]


def write_set(tmp_path, named, pats):
    """the files under tmp_path/in, the patterns in a file: ([(path, bytes)] in the order given, the pattern file)"""
    d = tmp_path / "in"
    d.mkdir(parents=True, exist_ok=True)
    files = []
    for name, t in named:
        (d / name).write_bytes(t)
        files.append((str(d / name), t))
    p = tmp_path / "pats.txt"
    p.write_bytes(b"".join(x + b"\n" for x in pats))
    assert sum(len(t) for _, t in files) < 16384
    return files, str(p)


def base_args(files, pats, workers, g=G):
    return ["-f", ",".join(p for p, _ in files), "-p", pats, "-B", str(B), "-D", "0", "-G", str(g), "-L", "64", "-w", str(workers),
            "-R", "128"]


def check_L(files, workers):
    """set L lies as the test means it to: four buffers a worker, no file cut, no match over two files; one buffer of a
    worker is unpacked, one has G starts, the last has fewer starts than the buffer its object held before"""
    bufs = lay.layout(files, B, G, workers)
    assert [len(b) for b in bufs] == [4] * workers
    assert lay.cut_files(files, B, G, workers) == [] and lay.no_match_spans_files(files, workers, LPATS)
    for mine in bufs:
        assert sorted(len(b.starts) for b in mine[:3]) == [1, 2, G] and sum(not b.packed for b in mine) >= 2
        assert len(mine[3].chunks) == 2 and len(mine[3].starts) == 1 < len(mine[1].chunks)
    return bufs


def check_files(got, exp, grep_of=None):
    assert sorted(got) == sorted(exp)
    for name in sorted(exp):
        assert got[name] == exp[name], name
        if GREP and grep_of:
            assert got[name] == grep_of(name), name


def multiset(stdout):
    return sorted(stable(stdout))


@pytest.mark.parametrize("workers", [1, 2, 3])
def test_extract_over_buffers(gpu, tmp_path, workers):
    files, pats = write_set(tmp_path, set_L(workers), LPATS)
    check_L(files, workers)
    paths = {os.path.basename(p): p for p, _ in files}
    base = base_args(files, pats, workers) + ["-v"]
    _, _, plain = run(base)
    for k, (arg, before, after, invert) in enumerate((("1,2", 1, 2, False), ("0", 0, 0, True))):
        exp = lay.lines_expected(files, B, G, workers, LPATS, before, after, invert)
        assert sum(1 for v in exp.values() if v) >= 8 * workers and sum(1 for p, t in files if t and not exp[os.path.basename(p)]) >= workers
        out = tmp_path / ("out%d" % k)
        _, stats, p = run(base + ["-C", arg, "-T", str(out)] + (["-V"] if invert else []))
        check_files(read_dir(str(out)), exp, lambda name: xc.grep_file(paths[name], pats, before, after, invert))
        assert multiset(p.stdout) == multiset(plain.stdout) and p.stderr == plain.stderr
        assert int(stats["Kernel launches"]) >= 4 * workers


@pytest.mark.parametrize("workers", [1, 3])
def test_prefixes_over_buffers(gpu, tmp_path, workers):
    files, pats = write_set(tmp_path, set_L(workers), LPATS)
    bufs = check_L(files, workers)
    paths = {os.path.basename(p): p for p, _ in files}
    base = base_args(files, pats, workers)
    third_ok = 0
    for k, (arg, n, invert, flags) in enumerate((("2", 2, False, ["-H", "-N", "-b"]), ("0", 0, True, ["-N", "-b"]))):
        exp = lay.lines_expected(files, B, G, workers, LPATS, n, n, invert, flags)
        out = tmp_path / ("out%d" % k)
        _, stats, _ = run(base + ["-C", arg, "-T", str(out)] + flags + (["-V"] if invert else []))
        got = read_dir(str(out))
        check_files(got, exp, lambda name: fc.grep_file(paths[name], pats, n, n, invert, flags))
        assert int(stats["Kernel launches"]) >= 4 * workers
        for mine in bufs:
            # numbers and offsets are the file's: in the worker's third buffer a line is line 1 at offset 0 of its file,
            # also in a file that is not the buffer's first; in its fourth buffer the numbers begin again
            heads = []
            for at, f in mine[2].starts:
                path = files[f][0]
                want = (path.encode() + b":" if "-H" in flags else b"") + b"1:0:"
                if exp[os.path.basename(path)].startswith(want):
                    assert got[os.path.basename(path)].startswith(want), path
                    heads.append(at)
            if not invert:
                assert heads and (len(mine[2].starts) == 1 or max(heads) > 0)
            third_ok += bool(heads)
            path, t = files[mine[3].starts[0][1]]
            lines = got[os.path.basename(path)].splitlines()
            numbers = [int(l[len(path) + 1 if "-H" in flags else 0:].replace(b"-", b":").split(b":")[0]) for l in lines if l != b"--"]
            assert numbers and numbers == sorted(set(numbers)) and numbers[-1] <= t.count(b"\n")
            if not invert:
                assert numbers[0] == 1
    assert third_ok > workers


def test_outputs_do_not_depend_on_the_layout(gpu, tmp_path):
    """with -S no text crosses a file: the files written are the same for every layout of the same input files"""
    files, pats = write_set(tmp_path, set_L(3), LPATS)
    check_L(files, 3)
    single, _ = write_set(tmp_path, set_L(3, single=True), LPATS)
    assert sorted(single) == sorted(files) and lay.cut_files(single, B, G, 1) == [] and len(lay.layout(single, B, G, 1)[0]) == 10
    assert len(lay.layout(single, B, 256, 1)[0]) == 1
    for k, flags in enumerate(([], ["-H", "-N", "-b"])):
        dirs = []
        for j, (order, g, workers) in enumerate(((single, G, 1), (files, G, 3), (single, 256, 1))):
            out = tmp_path / ("out%d_%d" % (k, j))
            _, stats, _ = run(base_args(order, pats, workers, g) + ["-S", "-C", "1", "-T", str(out)] + flags)
            assert int(stats["Kernel launches"]) == (10, 12, 1)[j]
            dirs.append(read_dir(str(out)))
        assert dirs[0] == dirs[1] == dirs[2] and sum(1 for v in dirs[0].values() if v) >= 18
        if flags:
            assert any(b".txt:1:0:" in v for v in dirs[0].values()) and any(b".txt-" in v for v in dirs[0].values())


@pytest.mark.parametrize("workers", [1, 2])
def test_words_over_buffers(gpu, tmp_path, workers):
    """-W: the passes of a buffer are enqueued once the first byte of the next one is known, and that byte decides the
    record at the buffer's very end"""
    files, pats = write_set(tmp_path / "L", set_L(workers), LPATS)
    check_L(files, workers)
    base = base_args(files, pats, workers) + ["-W"]
    for k, flags in enumerate(([], ["-H", "-N"])):
        exp = lay.lines_expected(files, B, G, workers, LPATS, 1, 1, False, flags, words=True)
        # (the expectation bites: a word pass that took every buffer's end for the end of the text would keep "chaff pin")
        assert exp != lay.lines_expected(files, B, G, workers, LPATS, 1, 1, False, flags, words=True, blind=True)
        assert exp != lay.lines_expected(files, B, G, workers, LPATS, 1, 1, False, flags)
        out = tmp_path / ("out%d" % k)
        _, stats, _ = run(base + ["-C", "1", "-T", str(out)] + flags)
        check_files(read_dir(str(out)), exp)
        assert int(stats["Kernel launches"]) >= 4 * workers
    # the last line of w0's ten-chunk file is "chaff pin" and the next buffer begins with a word byte: not selected;
    # w0's third buffer ends in "straw hay" and the next begins with a space: selected
    assert not exp["w0_b10_open.txt"].endswith(b"pin\n") and exp["w0_l_open.txt"].endswith(b":straw hay\n")
    files, pats = write_set(tmp_path / "R", set_R(workers), RPATS)
    exp, dropped, buffers = lay.rewrite_expected(files, B, G, workers, RPATS, REPL, words=True)
    assert buffers == 4 * workers
    assert exp != lay.rewrite_expected(files, B, G, workers, RPATS, REPL, words=True, blind=True)[0]
    assert b" abcd" in exp["w0_B.txt"] and exp["w0_C.txt"].endswith(b" <AB>")
    out = tmp_path / "outR"
    _, stats, p = run(base_args(files, pats, workers) + ["-W", "-o", "-r", repl_file(tmp_path), "-O", str(out)])
    check_files(read_dir(str(out)), exp)
    assert int(stats["Kernel launches"]) == buffers


def check_R(files, workers):
    bufs = lay.layout(files, B, G, workers)
    for mine in bufs:
        assert [(len(b.chunks), len(b.starts), b.cut) for b in mine] == [(G, 2, False), (G, 2, True), (G, 1, True), (3, 1, False)]
        assert [b.packed for b in mine] == [False, False, True, True]
    return bufs


@pytest.mark.parametrize("flags", [[], ["-S"], ["-i"]], ids=["plain", "-S", "-i"])
@pytest.mark.parametrize("workers", [1, 2])
def test_rewrite_over_buffers(gpu, tmp_path, workers, flags):
    files, pats = write_set(tmp_path, set_R(workers), RPATS)
    check_R(files, workers)
    exp, dropped, buffers = lay.rewrite_expected(files, B, G, workers, RPATS, REPL, "-S" in flags, "-i" in flags)
    assert buffers == 4 * workers and dropped >= 2 * workers and all(exp[os.path.basename(p)] != t for p, t in files if t)
    out = tmp_path / "out" / "deep"
    base = base_args(files, pats, workers) + ["-v", "-o"] + flags
    args = base + ["-r", repl_file(tmp_path), "-O", str(out)]
    hits, stats, p = run(args)
    check_files(read_dir(str(out)), exp)
    assert int(stats["Kernel launches"]) == buffers
    # one NOTE for the run: the entries every worker's buffers dropped, summed
    notes = [l for l in p.stderr.splitlines() if l.startswith("NOTE:")]
    assert len(notes) == 1 and notes[0].startswith("NOTE: %d matches began in the buffer in front" % dropped) and "-G/-B" in notes[0]
    _, _, only = run(base)
    assert multiset(p.stdout) == multiset(only.stdout) and len(hits) > 30 * workers and p.stderr == only.stderr
    run(args)
    assert read_dir(str(out)) == exp


def test_select_over_buffers(gpu, tmp_path):
    workers = 2
    files, pats = write_set(tmp_path, set_R(workers), RPATS)
    check_R(files, workers)
    exp, dropped, buffers = lay.select_expected(files, B, G, workers, RPATS)
    assert buffers == 8 and dropped >= 4 and len(exp) > 100
    hits, stats, p = run(base_args(files, pats, workers) + ["-v", "-o"])
    got = collections.Counter((os.path.basename(h[2]), h[1], int(h[4]) - 1) for h in hits)
    want = collections.Counter(exp)
    assert got == want, "missing %s, not expected %s (the first ten)" % (sorted((want - got).items())[:10], sorted((got - want).items())[:10])
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp) and int(stats["Kernel launches"]) == buffers
    notes = [l for l in p.stderr.splitlines() if l.startswith("NOTE:")]
    assert len(notes) == 1 and notes[0].startswith("NOTE: %d matches began in the buffer in front" % dropped)


def test_composes_over_buffers(gpu, tmp_path):
    """-n, -A -c and -o in front of -C: the same files, and what they print is what they print without -C"""
    workers = 2
    files, pats = write_set(tmp_path, set_L(workers), LPATS)
    check_L(files, workers)
    exp = lay.lines_expected(files, B, G, workers, LPATS, 1, 1, False)
    base = base_args(files, pats, workers)
    _, stats, p = run(base + ["-n", "-v", "-C", "1", "-T", str(tmp_path / "out_n")])
    check_files(read_dir(str(tmp_path / "out_n")), exp)
    numbered = collections.Counter((m.group(3), m.group(2), int(m.group(4))) for m in map(NLINE.match, p.stdout.splitlines()) if m)
    want = lay.numbered_expected(files, workers, LPATS)
    assert numbered == want and sum(want.values()) > 30 and max(k[2] for k in want) > 10
    assert int(stats["Processed lines"]) == sum(t.count(b"\n") for _, t in files)
    _, _, p = run(base + ["-A", "-c", "-C", "1", "-T", str(tmp_path / "out_c")])
    check_files(read_dir(str(tmp_path / "out_c")), exp)
    _, _, plain = run(base + ["-A", "-c"])
    counts = lambda text: sorted(l for l in text.splitlines() if l.startswith("Count "))
    assert counts(p.stdout) == counts(plain.stdout) and len(counts(p.stdout)) == len(files) + len(LPATS)
    run(base + ["-o", "-C", "1", "-T", str(tmp_path / "out_o")])
    check_files(read_dir(str(tmp_path / "out_o")), exp)


def test_exact_fits_and_cuts(gpu, tmp_path):
    pats = None
    # a file that fills a buffer to its last byte, with and without a newline there: the next buffer begins a new file
    for k, open_end in enumerate((False, True)):
        named = [("fit.txt", sized(11, G * B, open_end, first=b"hay first", last=b"the last pin")), ("next.txt", sized(12, 90, False, first=b"pin"))]
        files, pats = write_set(tmp_path / ("fit%d" % k), named, LPATS)
        assert [(len(b.chunks), b.packed, b.cut) for b in lay.layout(files, B, G, 1)[0]] == [(G, True, False), (2, True, False)]
        out = tmp_path / ("out_fit%d" % k)
        _, stats, _ = run(base_args(files, pats, 1) + ["-C", "1", "-T", str(out)])
        check_files(read_dir(str(out)), lay.lines_expected(files, B, G, 1, LPATS, 1, 1, False),
                    lambda name: xc.grep_file(dict((os.path.basename(p), p) for p, _ in files)[name], pats, 1, 1, False))
        assert int(stats["Kernel launches"]) == 2
    # one byte more is cut, and the error names the file, here the second worker's second
    named = [("w0_a.txt", sized(13, 100, False)), ("w1_a.txt", sized(14, G * B, False)), ("w0_b.txt", sized(15, 100, False)),
             ("w1_b_cut.txt", sized(16, G * B + 1, False))]
    files, pats = write_set(tmp_path / "cut", named, LPATS)
    assert lay.cut_files(files, B, G, 2) == [3] and [b.cut for b in lay.layout(files, B, G, 2)[1]] == [False, False, True]
    p = subprocess.run([CLI] + base_args(files, pats, 2) + ["-C", "1", "-T", str(tmp_path / "out_cut")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "ERROR: -C: file '%s' is cut across two buffers" % files[3][0] in p.stderr
    # more workers than files; a worker whose only file is empty; nothing but empty files
    for k, (named, workers) in enumerate((([("a.txt", sized(17, 200, False, first=b"hay")), ("b.txt", sized(18, 70, True, last=b"pin"))], 3),
                                          ([("a.txt", sized(19, 200, False, first=b"hay")), ("empty.txt", b"")], 2),
                                          ([("e0.txt", b""), ("e1.txt", b"")], 2))):
        files, pats = write_set(tmp_path / ("few%d" % k), named, LPATS)
        out = tmp_path / ("out_few%d" % k)
        run(base_args(files, pats, workers) + ["-C", "1", "-T", str(out)])
        exp = lay.lines_expected(files, B, G, workers, LPATS, 1, 1, False)
        check_files(read_dir(str(out)), exp)
        assert all(exp[n] for n, t in named if t) and len(exp) == 2


def digits_upto(n):
    """the decimal digits of 0 .. n - 1, summed"""
    return sum(len(str(i)) for i in range(n))


def test_prefix_output_that_does_not_fit(gpu, tmp_path):
    """a file of newlines only under -V -H -N -b: line i of n comes out as "<name>:<i>:<i - 1>:\\n".  buffer_alloc gives the
    output of a buffer of size = G * B bytes
        ex_cap = size * 5 / 2 + 4 * G + 64 + (size / 4 + 4096) * fmt_width,  fmt_width = (longest path + 1) + 11 + 11
    bytes: with -G 256 -B 64 and a name of 8 bytes 16384 * 5 / 2 + 1024 + 64 + 8192 * 31 = 296000.  n lines need
        n * (8 + 4) + digits(1 .. n) + digits(0 .. n - 1)
    bytes: 295992 for n = 14464, which fits, and 296014 for n = 14465, which does not"""
    size, name_len = 256 * B, 8
    cap = size * 5 // 2 + 4 * 256 + 64 + (size // 4 + 4096) * (name_len + 1 + 11 + 11)
    need = lambda n: n * (name_len + 4) + digits_upto(n + 1) - 1 + digits_upto(n)
    fits, over = 14464, 14465
    assert cap == 296000 and need(fits) == 295992 <= cap < need(over) == 296014 and over <= size
    (tmp_path / "fits.txt").write_bytes(b"\n" * fits)
    (tmp_path / "over.txt").write_bytes(b"\n" * over)
    pats = tmp_path / "pats.txt"
    pats.write_bytes(b"".join(x + b"\n" for x in LPATS))
    args = ["-p", str(pats), "-B", str(B), "-D", "0", "-G", "256", "-L", "64", "-w", "1", "-C", "0", "-V", "-H", "-N", "-b"]
    p = subprocess.run([CLI, "-f", "over.txt"] + args + ["-T", "out_over"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert p.returncode != 0 and "ERROR: -C:" in p.stderr and "over.txt" in p.stderr and "the output buffer holds %d" % cap in p.stderr
    p = subprocess.run([CLI, "-f", "fits.txt"] + args + ["-T", "out_fits"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    got = read_dir(str(tmp_path / "out_fits"))
    exp = b"".join(b"fits.txt:%d:%d:\n" % (i + 1, i) for i in range(fits))
    assert len(exp) == need(fits) and list(got) == ["fits.txt"] and got["fits.txt"] == exp
    if GREP:
        r = subprocess.run([GREP, "-a", "-F", "-f", str(pats), "-H", "-n", "-b", "-v", "fits.txt"], capture_output=True, cwd=str(tmp_path),
                           env=dict(os.environ, LC_ALL="C"), timeout=60)
        assert r.returncode == 0 and got["fits.txt"] == r.stdout
