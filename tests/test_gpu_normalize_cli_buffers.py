"""acm_grep -S -z over several buffers per worker, several workers, unpacked buffers, -W, -I, -t, -c and files that a
buffer cuts: prepare(), submit() and finish() of csrc/acm_grep.cpp with the normalise call in front of the scan and the
remap behind the passes, in the shapes a real run has.  The expectation is tests/cli_layout.normalized_hits: the layout
computed on the host, every piece of a file normalised alone by tests/normalize_model.py, bytes.find over the joined
pieces of a text, the model's last[] to map back.  A -v line is compared whole: the pattern, the file, the offset in the
buffer ("at offset": the chunk's place in the buffer and the place in the chunk) and the place in the chunk ("relative").

The file sets and what they are meant to show (layouts, hits across cuts, word borders that exist only on one side of
the normalisation, exact patterns dropped where folding ones are kept) need no device: tests/test_host_cli_layout.py
checks the same functions on the host."""
import collections
import functools
import os
import re

import numpy as np
import pytest

import cli_layout as lay
import normalize_model as nm
from test_gpu_normalize_cli import SPECS
from test_gpu_select_cli import run

pytestmark = pytest.mark.gpu

B = 64
G_WHOLE = 48                       # buffers of 3072 bytes, the groups of whole_set() fill them exactly
G_CUT = 16                         # what acm_grep makes of -G 2 and -G 3: it rounds up to a multiple of 16
TOKENS = [b"a", b" ", b"  ", b"\t", b"\n", b"%20", b"%09", b"%41", b"%4", b"%", b"href", b"HREF", b"b", b"B", b"A", b"a href",
          b"a%20href", b"A HREF", b"x", b"0A", b"%2541", b"\r\n", b"\0", b"a b", b" b ", b"script:", b"SCRIPT:", b"a\0 \0b\0"]
# without -A a run reports one pattern per end: no pattern of ONE is a suffix of another, folded or not
ONE = [b"a href", b"a b", b"0A ", b" b ", b"x A", b"script:", b"%41", b"ahref", b"bA"]
EVERY = ONE + [b"href", b"A", b" b", b"ref"]
# (searched for, not matched from a line's start: in text mode the output may go on behind a line without a newline)
COUNT = re.compile(r"Count (file|pattern) (.*?): (\d+)$", re.M)
EXTRAS = {"-v": ["-v"], "-A": ["-v", "-A"], "-i": ["-v", "-i"], "-c": ["-v", "-c"], "-c-A": ["-v", "-c", "-A"]}


def make(seed, size, tokens=TOKENS):
    rng = np.random.default_rng(seed)
    return b"".join(tokens[i] for i in rng.integers(0, len(tokens), size))[:size]


def write_inputs(tmp_path, named, pats, name="pats.txt"):
    """the files under tmp_path/in, the patterns as hex lines: ([(path, bytes)] in the order given, the pattern file)"""
    d = tmp_path / "in"
    d.mkdir(parents=True, exist_ok=True)
    files = []
    for fname, t in named:
        (d / fname).write_bytes(t)
        files.append((str(d / fname), t))
    p = tmp_path / name
    p.write_bytes(b"".join(x.hex().encode() + b"\n" for x in pats))
    return files, str(p)


def args_of(files, pats, workers, g, spec, extra, b=B):
    return ["-f", ",".join(p for p, _ in files), "-p", pats, "-x", "-B", str(b), "-D", "0", "-G", str(g), "-L", "64", "-w", str(workers),
            "-R", "1024", "-S", "-z", spec] + extra


def lines_of(hits, pats):
    """the -v lines as (pattern index, file name, "at offset", "relative")"""
    index = {p.decode("latin-1"): i for i, p in enumerate(pats)}
    return sorted((index[text], os.path.basename(f), int(off), int(rel)) for _, text, f, off, rel in hits)


def lines_expected(exp, files, b=B):
    return sorted((h.pattern, os.path.basename(files[h.file][0]), h.slot * b + h.offset % b + 1, h.offset % b + 1) for h in exp)


def counts_of(p, pats):
    index = {x.decode("latin-1"): i for i, x in enumerate(pats)}
    out = []
    for kind, what, n in COUNT.findall(p.stdout):
        out.append((kind, os.path.basename(what.strip("'")) if kind == "file" else index[re.search(r"\('(.*)'\)$", what).group(1)], int(n)))
    return sorted(out, key=str)


def counts_expected(exp, files, pats):
    per_file, per_pat = collections.Counter(h.file for h in exp), collections.Counter(h.pattern for h in exp)
    return sorted([("file", os.path.basename(path), per_file[f]) for f, (path, _) in enumerate(files)] +
                  [("pattern", i, n) for i, n in per_pat.items()], key=str)


def check_run(files, pats_path, pats, workers, g, spec, extra, exp, b=B):
    hits, stats, p = run(args_of(files, pats_path, workers, g, spec, extra, b))
    got, want = lines_of(hits, pats), lines_expected(exp, files, b)
    assert got == want, "%d lines, %d expected; missing %s, not expected %s (the first five)" % (
        len(got), len(want), sorted(set(want) - set(got))[:5], sorted(set(got) - set(want))[:5])
    assert int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp)
    assert "NOTE" not in p.stderr and "ERROR" not in p.stdout
    if "-c" in extra:
        assert counts_of(p, pats) == counts_expected(exp, files, pats)
    return stats


# ------------------------------------------------------------------ files whole: workers, buffers, unpacked buffers

GROUPS = ((47, 1), (24, 11, 13), (2, 4, 30, 12), (5,))      # chunks per file; a group fills a buffer of G_WHOLE chunks, the last is short


@functools.lru_cache(maxsize=None)
def whole_set(workers, packed=False, tokens=tuple(TOKENS), ends=b""):
    """(name, bytes) in the order of -f: per worker four buffers of whole files, the workers' lists interleaved.  packed:
    every file a multiple of B, else short chunks lie in the middle of the buffers.  ends: what every file ends in"""
    per = []
    for w in range(workers):
        rng = np.random.default_rng(50 + w)
        mine = []
        for g, group in enumerate(GROUPS):
            for k, c in enumerate(group):
                size = B * c if packed else B * (c - 1) + int(rng.integers(len(ends) + 1, B))
                t = make(1000 * w + 10 * g + k, size, tokens)
                mine.append(("w%d_g%d_%d.txt" % (w, g, k), t[:size - len(ends)] + ends))
        per.append(mine)
    return [l[i] for i in range(len(per[0])) for l in per]


def check_whole(files, workers, packed=False):
    """the set lies as meant: four buffers a worker, no file cut, short chunks in the middle of buffers (or none)"""
    bufs = lay.layout(files, B, G_WHOLE, workers)
    assert [len(b) for b in bufs] == [4] * workers and lay.cut_files(files, B, G_WHOLE, workers) == []
    for mine in bufs:
        assert [len(b.starts) for b in mine] == [len(g) for g in GROUPS]
        assert [b.packed for b in mine] == ([True] * 4 if packed else [False, False, False, True])
    return bufs


def whole_expected(workers, spec, extra, packed=False):
    """(the files as (name, bytes), the patterns, the Hits) of a run over whole_set"""
    flags, blanks = SPECS[spec]
    named = whole_set(workers, packed)
    pats = EVERY if "-A" in extra else ONE
    exp = lay.normalized_hits(named, pats, B, G_WHOLE, workers, flags, blanks, nocase="-i" in extra)
    assert len(exp) > 100 * workers and len({h.pattern for h in exp}) >= 4 and not any(h.spans for h in exp)
    if "-A" not in extra:
        assert len({(h.file, h.offset) for h in exp}) == len(exp)     # one pattern per end
    return named, pats, exp


@pytest.mark.parametrize("extra", sorted(EXTRAS))
@pytest.mark.parametrize("spec", ["url,ws", "strip,url", "nul"])
@pytest.mark.parametrize("workers", [1, 2, 3])
def test_workers_and_buffers(gpu, tmp_path, workers, spec, extra):
    named, pats, exp = whole_expected(workers, spec, EXTRAS[extra])
    files, path = write_inputs(tmp_path, named, pats)
    check_whole(files, workers)
    stats = check_run(files, path, pats, workers, G_WHOLE, spec, EXTRAS[extra], exp)
    assert int(stats["Kernel launches"]) == 4 * workers


def test_packed_and_unpacked_buffers(gpu, tmp_path):
    """the same run over buffers that are all packed (every file a multiple of the chunk) and over the set above, where
    acm_pack_chunks runs in front of the normalise call"""
    for packed in (True, False):
        named, pats, exp = whole_expected(2, "url,ws", ["-v", "-c"], packed)
        files, path = write_inputs(tmp_path / str(packed), named, pats)
        bufs = check_whole(files, 2, packed)
        assert all(b.packed for mine in bufs for b in mine) == packed
        check_run(files, path, pats, 2, G_WHOLE, "url,ws", ["-v", "-c"], exp)


# ------------------------------------------------------------------ -W

WTOKENS = [b"a%20href", b"xa href", b"a hrefx", b"%41 href", b"%20a href", b"a href%41", b"a href", b" ", b"\n", b"b", b"a b", b"_", b"%5f",
           b"a%09b", b"x", b"A href", b"%2e", b"."]
WONE = [b"a href", b"A href", b"a b"]
WEVERY = WONE + [b"href", b"ref"]


def word_set(workers):
    return whole_set(workers, False, tuple(WTOKENS), b" a href")


def word_flips(named, pats, flags):
    """occurrences in the normalised files whose word borders differ from those of the bytes around them in the file as it
    is: (bordered only after the normalisation, bordered only before it)"""
    after = before = 0
    for _, t in named:
        x = nm.normalize(t, flags)
        for p, e in zip(*(a.tolist() for a in lay.entries([x.out], pats))):
            k = e - len(pats[p]) + 1
            norm = (k == 0 or x.out[k - 1] not in lay.WORD) and (e + 1 == x.m or x.out[e + 1] not in lay.WORD)
            f, l = int(x.first[k]), int(x.last[e])
            raw = (f == 0 or t[f - 1] not in lay.WORD) and (l + 1 == len(t) or t[l + 1] not in lay.WORD)
            after += int(norm and not raw)
            before += int(raw and not norm)
    return after, before


def word_expected(workers, every):
    named, pats = word_set(workers), WEVERY if every else WONE
    flags = nm.PERCENT | nm.SQUEEZE
    exp = lay.normalized_hits(named, pats, B, G_WHOLE, workers, flags, words=True)
    loose = lay.normalized_hits(named, pats, B, G_WHOLE, workers, flags)
    assert 30 * workers < len(exp) < len(loose) - 30 * workers           # the word test drops records
    after, before = word_flips(named, pats, flags)
    assert after >= 5 and before >= 5, (after, before)
    assert all(t.endswith(b" a href") for _, t in named)                  # a file that ends in the pattern: its end is a border
    assert sum(1 for h in exp if h.pattern == 0 and h.offset == len(named[h.file][1]) - 1) == len(named)
    return named, pats, exp


@pytest.mark.parametrize("every", [False, True], ids=["first", "-A"])
@pytest.mark.parametrize("workers", [1, 2])
def test_words(gpu, tmp_path, workers, every):
    """-W: the word pass reads the normalised stream and the worker's normalised tail, and is enqueued once the next
    buffer's first byte is known"""
    named, pats, exp = word_expected(workers, every)
    files, path = write_inputs(tmp_path, named, pats)
    check_whole(files, workers)
    check_run(files, path, pats, workers, G_WHOLE, "url,ws", ["-v", "-W"] + (["-A"] if every else []), exp)


# ------------------------------------------------------------------ -I

EXACT = [b"a href", b"x A", b"0A "]
FOLDING = [b"a b", b"script:", b" b%4"]


def case_expected(workers):
    named, pats = whole_set(workers), EXACT + FOLDING
    fold = [False] * len(EXACT) + [True] * len(FOLDING)
    flags = nm.PERCENT | nm.SQUEEZE
    exp = lay.normalized_hits(named, pats, B, G_WHOLE, workers, flags, nocase=fold)
    folded = lay.normalized_hits(named, pats, B, G_WHOLE, workers, flags, nocase=True)
    exact = lay.normalized_hits(named, pats, B, G_WHOLE, workers, flags)
    assert len(exact) + 10 < len(exp) < len(folded) - 10                  # folding patterns kept in another case, exact ones dropped there
    assert len({(h.file, h.offset) for h in folded}) == len(folded)
    return named, pats, exp


@pytest.mark.parametrize("extra", [["-v"], ["-v", "-c"]], ids=["-v", "-c"])
@pytest.mark.parametrize("workers", [1, 2])
def test_mixed_case(gpu, tmp_path, workers, extra):
    """-I: the case pass runs over the normalised stream, its `before` the worker's normalised tail"""
    named, pats, exp = case_expected(workers)
    files, path = write_inputs(tmp_path, named, EXACT)
    fold_path = tmp_path / "fold.txt"
    fold_path.write_bytes(b"".join(x.hex().encode() + b"\n" for x in FOLDING))
    check_whole(files, workers)
    check_run(files, path, pats, workers, G_WHOLE, "url,ws", ["-I", str(fold_path)] + extra, exp)


# ------------------------------------------------------------------ -t

TB, TB_MODEL = 256, 4096           # -B of the run (a line is a chunk); the model's: a file is a chunk, so the layout cuts no line
TLINE = re.compile(r"Pattern (-?\d+) \('(.*?)'\) found in file '(.*?)' at offset (\d+) \[relative: (-?\d+)\]$", re.M)
LTOKENS = [t for t in TOKENS if b"\0" not in t and b"\n" not in t] + [b"%0a", b"%0A"]      # (text mode reads lines as C strings)


@functools.lru_cache(maxsize=None)
def line_set(workers):
    """files of lines of at most 100 bytes: lines of blanks only, %0a inside a line, CRLF, a last line without LF"""
    rng = np.random.default_rng(77)
    named = []
    for k in range(6 * workers):
        lines = [make(int(rng.integers(1 << 30)), int(rng.integers(1, 100)), LTOKENS) for _ in range(int(rng.integers(8, 30)))]
        lines[1:1] = [b"   \t ", b"", b"a%0ab a%0a b", b"x a href\r", b" b \r", b"x a", b"href a", b"b x"]   # (a|href, a|b: no match over a line end)
        t = b"\n".join(lines) + (b"\n" if k % 2 else b" a href")
        named.append(("t%d.txt" % k, t))
    return named


def line_expected(workers, spec, extra):
    flags, blanks = SPECS[spec]
    named, pats = line_set(workers), EVERY if "-A" in extra else ONE
    assert all(len(l) <= 100 for _, t in named for l in t.split(b"\n")) and max(len(t) for _, t in named) <= TB_MODEL
    assert not lay.cut_files(named, TB_MODEL, 16, workers)
    exp = lay.normalized_hits(named, pats, TB_MODEL, 16, workers, flags, blanks, lines=True)
    per_file = lay.normalized_hits(named, pats, TB_MODEL, 16, workers, flags, blanks)
    assert len(exp) > 50 * workers and {(h.pattern, h.file, h.offset) for h in exp} != {(h.pattern, h.file, h.offset) for h in per_file}
    return named, pats, exp


@pytest.mark.parametrize("extra", ["-v", "-A", "-c"])
@pytest.mark.parametrize("spec", ["url,ws", "strip,url"])
@pytest.mark.parametrize("workers", [1, 2])
def test_lines_are_the_texts(gpu, tmp_path, workers, spec, extra):
    """-t: a line is a chunk and a text.  The -v line's "relative" is the place in the line; its "at offset" depends on
    how text mode pads the chunks and is not compared.  In text mode -v prints the line itself too: behind a last line
    without a newline the next "Pattern" line goes on on the same output line, so they are searched for, not taken from
    the starts of the output's lines"""
    named, pats, exp = line_expected(workers, spec, EXTRAS[extra])
    files, path = write_inputs(tmp_path, named, pats)
    hits, stats, p = run(args_of(files, path, workers, 16, spec, EXTRAS[extra] + ["-t"], TB))
    index = {x.decode("latin-1"): i for i, x in enumerate(pats)}
    hits = TLINE.findall(p.stdout)
    got = collections.Counter((index[text], os.path.basename(f), int(rel)) for _, text, f, _, rel in hits)
    want = collections.Counter((h.pattern, named[h.file][0], h.offset - named[h.file][1].rfind(b"\n", 0, h.offset)) for h in exp)
    assert got == want, "missing %s, not expected %s (the first five)" % (sorted((want - got).items())[:5], sorted((got - want).items())[:5])
    assert int(stats["Matches"]) == len(exp) and "NOTE" not in p.stderr
    if "-c" in EXTRAS[extra]:
        assert counts_of(p, pats) == counts_expected(exp, files, pats)


# ------------------------------------------------------------------ files that a buffer cuts

CUT_SIZES = (700, 3000, 150, 2200, 1024, 90, 2900, 1500, 333, 2048, 100, 1800)
PLANTS = (b"a h|ref", b"a%2|0href", b"a | href", b"a| b", b"a hre|f", b"scr|ipt:", b" |b ")


def file_cuts(named, workers):
    """(file, offset in it) of every place a buffer cuts a file"""
    out, done = [], collections.Counter()
    for bufs in lay.layout(named, B, G_CUT, workers):
        for b in bufs:
            if b.cut:
                out.append((b.chunks[0][0], done[b.chunks[0][0]]))
            for f, n in b.chunks:
                done[f] += n
    return out


@functools.lru_cache(maxsize=None)
def cut_set(workers):
    """a dozen files of 90 to 3000 bytes in buffers of 1024, and across every cut one of PLANTS, the '|' on the cut"""
    named = [("c%02d.txt" % k, bytearray(make(300 + k, n))) for k, n in enumerate(CUT_SIZES)]
    planted = []
    for k, (f, at) in enumerate(file_cuts(named, workers)):
        left, right = PLANTS[k % len(PLANTS)].split(b"|")
        if at >= len(left) + 1 and at + len(right) + 1 <= len(named[f][1]):
            named[f][1][at - len(left) - 1:at + len(right) + 1] = b"x" + left + right + b"x"
            planted.append((f, at, PLANTS[k % len(PLANTS)]))
    return [(n, bytes(t)) for n, t in named], planted


def cut_expected(workers, every):
    (named, planted), pats = cut_set(workers), EVERY if every else ONE
    flags = nm.PERCENT | nm.SQUEEZE
    bufs = lay.layout(named, B, G_CUT, workers)
    assert len(planted) >= 8 and {p for _, _, p in planted} == set(PLANTS)
    assert sum(1 for mine in bufs for b in mine if b.cut and len(b.starts) == 1) >= 3        # buffers without a text start
    exp = lay.normalized_hits(named, pats, B, G_CUT, workers, flags)
    whole = lay.normalized_hits(named, pats, B, 1 << 10, workers, flags)
    assert not any(h.spans for h in whole) and sum(1 for h in exp if h.spans) >= 5          # matches across a cut
    here, there = {(h.pattern, h.file, h.offset) for h in exp}, {(h.pattern, h.file, h.offset) for h in whole}
    for f, at, plant in planted:                                                            # a%2|0href, a | href: whole only
        end = (0, f, at + len(plant.split(b"|")[1]) - 1)
        assert (end in there) == (plant in (b"a h|ref", b"a%2|0href", b"a | href", b"a hre|f")), (plant, end)
        assert (end in here) == (plant in (b"a h|ref", b"a hre|f")), (plant, end)
    return named, pats, exp


@pytest.mark.parametrize("extra", ["-v", "-A", "-c"])
@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("workers", [1, 2])
def test_cut_files(gpu, tmp_path, workers, g, extra):
    """a file that a buffer cuts is normalised piece by piece and the scan goes on across the cut: a match whose
    normalised bytes lie on both sides is found, a triple or a run that the cut divides is not joined"""
    named, pats, exp = cut_expected(workers, "-A" in EXTRAS[extra])
    files, path = write_inputs(tmp_path, named, pats)
    check_run(files, path, pats, workers, g, "url,ws", EXTRAS[extra], exp)
