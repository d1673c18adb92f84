"""The context and extract passes on the host, no GPU needed: the model the GPU tests compare with
(tests/extract_model.py) against an independent brute force, per line and per byte, and against GNU grep
(-A/-B/-C/-v) where it is installed; hand cases for text barriers; the exported symbols, the workspace queries and
every argument error of the two entry points; the CLI's new ERROR: lines."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import extract_model as xm
import line_model as lm
from gpu_pattern_matching_amd import _lib
from test_host_lines import brute_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpu_pattern_matching_amd", "acm_grep")
ACM_ERR_ARG = -1
INT32_MAX = 0x7FFFFFFF
CONTEXTS = (0, 1, 2, 3, 7, INT32_MAX)


# ---- brute force

def brute_context(text, d, origin, offsets, invert, before, after, seg):
    """groups [(line, begin, next, lines)] and (selected, kept, groups) by loops over lines"""
    lines = [(b + origin, e + origin) for b, e in brute_lines(text, d, True)]
    sel = []
    for b, e in lines:
        holds = any(b <= o < e for o in offsets)
        sel.append(holds != invert)
    tid = [sum(1 for s in seg if s <= b) for b, _ in lines]
    kept = []
    for j in range(len(lines)):
        k = False
        for i in range(len(lines)):
            if sel[i] and tid[i] == tid[j] and j - after <= i <= j + before:
                k = True
        kept.append(k)
    groups, j = [], 0
    while j < len(lines):
        if not kept[j]:
            j += 1
            continue
        h = j
        while j + 1 < len(lines) and kept[j + 1] and tid[j + 1] == tid[h]:
            j += 1
        groups.append((h, lines[h][0], lines[j][1], j - h + 1))
        j += 1
    return groups, (sum(sel), sum(kept), len(groups))


def brute_extract(text, origin, ranges, glue, term, seg):
    """(out, at, seg_out, used, skipped, terminators, text bytes) byte by byte"""
    out, at, contrib = bytearray(), [], []
    used = skipped = terms = src = 0
    last_tid = None
    for b, e in ranges:
        if b < origin or b >= e or e > origin + len(text):
            skipped += 1
            continue
        tid = 0
        for s in seg:
            if s <= b:
                tid += 1
        before = len(out)
        if last_tid == tid:
            for g in glue:
                out.append(g)
        at.append(len(out))
        for x in range(b, e):
            out.append(text[x - origin])
            src += 1
        if term >= 0 and text[e - 1 - origin] != term:
            out.append(term)
            terms += 1
        contrib.append((b, len(out) - before))
        used += 1
        last_tid = tid
    seg_out = [sum(c for b, c in contrib if b < s) for s in seg]
    return bytes(out), at, seg_out, used, skipped, terms, src


def random_text(rng, n, d):
    t = rng.integers(97, 101, size=n).astype(np.uint8)
    t[rng.random(n) < (0.15, 0.4)[int(rng.integers(2))]] = d
    return bytes(t)


def test_model_context_matches_brute_force():
    rng = np.random.default_rng(31)
    cases = 0
    for n in list(range(0, 40)) * 10:
        d = (0x0A, 0x00)[cases % 2]
        t = random_text(rng, n, d)
        origin = (0, 500)[cases % 3 == 0]
        offs = np.unique(rng.integers(0, max(n, 1), size=int(rng.integers(0, 5)))) + origin if n else np.zeros(0, dtype=np.int64)
        seg = np.sort(rng.integers(origin - 2, origin + n + 4, size=int(rng.integers(0, 4)))) if cases % 2 else []
        before, after = (CONTEXTS[int(rng.integers(len(CONTEXTS)))] for _ in range(2))
        invert = bool(cases % 5 == 0)
        _, info, st = lm.index(t, origin, d)
        got, ctx_info = xm.context(st, info, origin, origin + n, offs, invert, before, after, seg)
        exp, figures = brute_context(t, d, origin, list(offs), invert, before, after, list(seg))
        assert list(zip(*[g.tolist() for g in got])) == exp, (t, offs, seg, before, after, invert)
        assert ctx_info.tolist() == list(figures) + [0] and ctx_info.dtype == np.int32
        cases += 1
    assert cases >= 300


def test_model_context_without_context_covers_the_selected_lines():
    """before == after == 0, no segments: the groups are the runs of adjacent selected lines, the same bytes"""
    rng = np.random.default_rng(32)
    for n in range(0, 60):
        t = random_text(rng, n, 0x0A)
        offs = np.unique(rng.integers(0, max(n, 1), size=4)) if n else np.zeros(0, dtype=np.int64)
        _, info, st = lm.index(t)
        for inv in (False, True):
            (rel, beg, nxt, cnt), ctx_info = xm.context(st, info, 0, n, offs, inv)
            srel, sbeg, snxt = lm.select(st, info, 0, n, offs, inv)
            assert b"".join(t[b:e] for b, e in zip(beg, nxt)) == b"".join(t[b:e] for b, e in zip(sbeg, snxt))
            assert int(cnt.sum()) == srel.size == ctx_info[0] == ctx_info[1]
            assert all(int(b) in set(sbeg.tolist()) for b in beg)


def test_model_extract_matches_brute_force():
    rng = np.random.default_rng(33)
    cases = 0
    for n in list(range(1, 31)) * 11:
        t = random_text(rng, n, 0x0A)
        origin = (0, -7, 1000)[cases % 3]
        k = int(rng.integers(0, 7))
        b = rng.integers(origin - 2, origin + n + 2, size=k)
        e = b + rng.integers(-1, 9, size=k)
        if cases % 4 == 0:      # ascending and disjoint, as the passes in front leave them
            cuts = np.sort(rng.integers(origin, origin + n + 1, size=2 * k))
            b, e = cuts[0::2], cuts[1::2]
        incl = bool(cases % 7 == 0)
        glue = (b"", b"-", b"--\n", b"0123456789abcdef")[cases % 4]
        term = (-1, 0x0A, 0x61)[cases % 3]
        seg = np.sort(rng.integers(origin - 1, origin + n + 2, size=int(rng.integers(1, 4)))) if cases % 2 else None
        count = (k, k + 3, -2, max(k - 1, 0))[cases % 4]        # the header cell may hold anything
        max_ranges = (k, max(k - 2, 0))[cases % 5 == 0]
        bp, ep = xm.plane_of(b, count), xm.plane_of(e - (1 if incl else 0), count)
        got = xm.extract(t, origin, bp, ep, max_ranges, incl, glue, term, seg)
        looked = min(max(count, 0), max_ranges)
        exp = brute_extract(t, origin, list(zip(b.tolist(), e.tolist()))[:looked], glue, term, [] if seg is None else list(seg))
        assert got["out"] == exp[0] and got["m"] == len(exp[0]) and got["at"] == exp[1]
        assert (got["seg_out"] is None) == (seg is None)
        if seg is not None:
            assert got["seg_out"].tolist() == exp[2]
        assert got["info"].tolist() == [exp[3], exp[4], len(exp[0]), 0, exp[6], 0, 0, exp[5]]
        for limit in (0, 1, len(exp[0]) // 2, len(exp[0])):
            cut = xm.extract(t, origin, bp, ep, max_ranges, incl, glue, term, seg, limit=limit)
            assert cut["out"] == exp[0][:limit] and cut["info"][6] == int(len(exp[0]) > limit)
        cases += 1
    assert cases >= 300


def test_model_extract_saturates():
    t = b"x" * 1000
    k = 3000
    got = xm.extract(t * 1000, 0, xm.plane_of([0] * k), xm.plane_of([1000000] * k), k, limit=1 << 20)
    m = k * 1000000
    assert got["m"] == m and m > 1 << 31 and got["info"][6] == 1 and len(got["out"]) == 1 << 20
    assert (int(np.uint32(got["info"][3])) << 32 | int(np.uint32(got["info"][2]))) == m
    assert got["at"][:3] == [0, 1000000, 2000000] and got["at"][-1] == INT32_MAX and got["at"][2147] == 2147000000


# ---- GNU grep

GREP = shutil.which("grep")

GREP_TEXTS = [
    b"",
    b"abc",
    b"abc\n",
    b"x\nabc",                                   # the last line without a newline, and it matches
    b"abc\nx",                                   # ... and it does not
    b"\n\n\nabc\n\n\n",                          # empty lines
    b"abc\n1\n2\n3\n4\nabc\n5\n6\n7\n8\n9\nabc\n",   # first and last line match; contexts adjacent, overlapping or apart
    b"1\n2\nabc\nabc\n3\n4\n5\n6\nabc\n7\n8",
    b"abcabc\nzabcz\n\nq\nq\nq\nq\nq\nabc",
    b"1\n2\n3\n4\n5\n",                          # no match
    b"".join(b"line %d %s\n" % (i, b"abc" if i % 7 == 3 or i % 11 == 0 else b"-") for i in range(60)),
]


def grep_output(text, pat, before, after, invert):
    cmd = [GREP, "-a", "-F", "-e", pat.decode()]
    if before + after > 0:
        cmd += ["-B", str(before), "-A", str(after)]
    if invert:
        cmd.append("-v")
    r = subprocess.run(cmd, input=text, capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=60)
    assert r.returncode in (0, 1), r.stderr
    return r.stdout


def occurrences(text, pat):
    """the offset every occurrence of pat ends at: the records a scan leaves"""
    out, at = [], text.find(pat)
    while at >= 0:
        out.append(at + len(pat) - 1)
        at = text.find(pat, at + 1)
    return out


@pytest.mark.skipif(GREP is None, reason="grep is not installed")
def test_model_matches_gnu_grep():
    runs = 0
    for t in GREP_TEXTS:
        for pat in (b"abc", b"c", b"1"):
            offs = occurrences(t, pat)
            for before, after in ((0, 0), (1, 1), (2, 2), (0, 2), (3, 0), (1, 3), (100, 100)):
                for invert in (False, True):
                    got = xm.grep_like(t, offs, before, after, invert)[0]
                    assert got == grep_output(t, pat, before, after, invert), (t, pat, before, after, invert)
                    runs += 1
    assert runs > 400


# ---- text barriers, by hand

def test_context_stops_at_a_text_start():
    #     0    1    2    3    4    5
    t = b"a\nb\nX\nc\nd\ne\n"
    _, info, st = lm.index(t)
    # texts [0, 6) and [6, 12): the match is the last line of the first
    (rel, beg, nxt, cnt), ctx = xm.context(st, info, 0, len(t), [4], False, 1, 2, [6])
    assert (rel.tolist(), beg.tolist(), nxt.tolist(), cnt.tolist()) == ([1], [2], [6], [2]) and ctx.tolist() == [1, 2, 1, 0]
    # a match either side of the start: two groups although the lines are adjacent
    (rel, beg, nxt, cnt), ctx = xm.context(st, info, 0, len(t), [4, 6], False, 0, 0, [6])
    assert (rel.tolist(), beg.tolist(), nxt.tolist(), cnt.tolist()) == ([2, 3], [4, 6], [6, 8], [1, 1])
    assert ctx.tolist() == [2, 2, 2, 0]
    # ... and one without the start
    (rel, beg, nxt, cnt), _ = xm.context(st, info, 0, len(t), [4, 6], False, 0, 0)
    assert (rel.tolist(), beg.tolist(), nxt.tolist(), cnt.tolist()) == ([2], [4], [8], [2])
    # "to the ends of the text", equal starts, and a start beyond the end
    (rel, beg, nxt, cnt), _ = xm.context(st, info, 0, len(t), [8], False, INT32_MAX, INT32_MAX, [6, 6, 100])
    assert (rel.tolist(), beg.tolist(), nxt.tolist(), cnt.tolist()) == ([3], [6], [12], [3])


def test_a_line_that_straddles_a_start_goes_with_the_text_it_begins_in():
    t = b"a\nbXc\nd\n"        # the first text is "a\nb": it does not end in the delimiter
    _, info, st = lm.index(t)
    (rel, beg, nxt, cnt), _ = xm.context(st, info, 0, len(t), [0], False, 0, 5, [0, 3])
    assert (rel.tolist(), beg.tolist(), nxt.tolist(), cnt.tolist()) == ([0], [0], [6], [2])
    (rel, beg, nxt, cnt), _ = xm.context(st, info, 0, len(t), [7], False, 5, 0, [0, 3])
    assert (rel.tolist(), beg.tolist(), nxt.tolist(), cnt.tolist()) == ([2], [6], [8], [1])


def test_no_glue_between_texts_and_seg_out_per_text():
    t = b"aa\nbb\ncc\ndd\nee"
    begin, end = [0, 6, 9, 12], [3, 9, 12, 14]
    ex = xm.extract(t, 0, xm.plane_of(begin), xm.plane_of(end), 4, glue=b"--\n", terminator=0x0A, seg_start=[0, 9, 9, 12, 50])
    assert ex["out"] == b"aa\n--\ncc\n" + b"dd\n" + b"ee\n"
    assert ex["seg_out"].tolist() == [0, 9, 9, 12, 15] and ex["at"] == [0, 6, 9, 12]
    assert ex["info"].tolist() == [4, 0, 15, 0, 11, 0, 0, 1]
    # descending ranges: the output follows the input, seg_out stays the sum of the ranges in front of each start
    ex = xm.extract(t, 0, xm.plane_of(begin[::-1]), xm.plane_of(end[::-1]), 4, glue=b"+", terminator=-1, seg_start=[0, 9, 9, 12, 50])
    assert ex["out"] == b"ee" + b"dd\n" + b"cc\n+aa\n" and ex["seg_out"].tolist() == [0, 7, 7, 10, 12]


# ---- the C ABI

def test_symbols_exported(lib):
    for name in ("acm_line_context_workspace_bytes", "acm_line_context_async", "acm_extract_workspace_bytes",
                 "acm_extract_async"):
        assert hasattr(lib, name), name
        assert name in _lib.NATIVE_API


SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 20) + 3, 1 << 25, (1 << 31) - 17)


def test_workspace_queries(lib):
    for fn in (lib.acm_line_context_workspace_bytes, lib.acm_extract_workspace_bytes):
        for seg in (0, 1, 1000, 1 << 20):
            prev = 0
            for n in SIZES:
                b = fn(n, seg)
                assert b > 0 and b % 256 == 0 and b >= prev
                prev = b
        for n in (0, 1000, 1 << 20):
            prev = 0
            for seg in SIZES:
                b = fn(n, seg)
                assert b % 256 == 0 and b >= prev
                prev = b


def _err(lib, rc):
    assert rc == ACM_ERR_ARG
    assert lib.acm_last_error()


def test_context_argument_errors(lib):
    buf = (C.c_char * 16384)()
    a = (C.addressof(buf) + 15) & ~15     # never dereferenced: every call fails before anything is enqueued
    ws = lib.acm_line_context_workspace_bytes(8, 2)
    ok = dict(ls=a, cap=8, info=a + 64, origin=0, end=64, off=a + 128, maxr=4, inv=0, before=1, after=1, seg=a + 192, nseg=2,
              rel=a + 256, beg=a + 512, nxt=a + 768, cnt=a + 1024, ocap=8, cinfo=a + 1280, ws=a + 2048, wsb=ws)

    def call(**kw):
        k = dict(ok, **kw)
        return lib.acm_line_context_async(k["ls"], k["cap"], k["info"], k["origin"], k["end"], k["off"], k["maxr"], k["inv"],
                                          k["before"], k["after"], k["seg"], k["nseg"], k["rel"], k["beg"], k["nxt"], k["cnt"],
                                          k["ocap"], k["cinfo"], k["ws"], k["wsb"], None)
    for name in ("ls", "info", "off", "rel", "beg", "nxt", "cinfo", "ws"):
        _err(lib, call(**{name: None}))
    _err(lib, call(cap=0))
    _err(lib, call(ocap=1))
    _err(lib, call(wsb=ws - 1))
    _err(lib, call(end=-1))
    _err(lib, call(before=-1))
    _err(lib, call(after=-1))
    _err(lib, call(seg=None))             # segments without their starts
    _err(lib, call(nseg=0))               # starts without segments
    _err(lib, call(cap=1 << 20))          # the workspace is short for this capacity


def test_extract_argument_errors(lib):
    buf = (C.c_char * 16384)()
    a = (C.addressof(buf) + 15) & ~15
    ws = lib.acm_extract_workspace_bytes(8, 2)
    ok = dict(text=a, n=64, origin=0, bp=a + 128, ep=a + 256, maxr=8, flags=0, glue=b"--\n", glen=3, term=10, out=a + 512,
              ocap=256, at=a + 1024, acap=10, seg=a + 1280, nseg=2, sout=a + 1344, info=a + 1408, ws=a + 2048, wsb=ws)

    def call(**kw):
        k = dict(ok, **kw)
        return lib.acm_extract_async(k["text"], k["n"], k["origin"], k["bp"], k["ep"], k["maxr"], k["flags"], k["glue"], k["glen"],
                                     k["term"], k["out"], k["ocap"], k["at"], k["acap"], k["seg"], k["nseg"], k["sout"], k["info"],
                                     k["ws"], k["wsb"], None)
    for name in ("bp", "ep", "info", "text", "out", "ws"):
        _err(lib, call(**{name: None}))
    _err(lib, call(text=a + 4))
    _err(lib, call(out=a + 516))
    _err(lib, call(n=(1 << 31) - 16))
    _err(lib, call(ocap=(1 << 31) - 16))
    _err(lib, call(acap=1))
    _err(lib, call(maxr=(1 << 31) - 1))
    _err(lib, call(origin=1 << 31))
    _err(lib, call(origin=-(1 << 31) - 1))
    _err(lib, call(seg=None))
    _err(lib, call(sout=None))
    _err(lib, call(nseg=0))
    _err(lib, call(nseg=1 << 31))
    _err(lib, call(flags=2))
    _err(lib, call(flags=0x80000001))
    _err(lib, call(glen=-1))
    _err(lib, call(glen=17))
    _err(lib, call(glue=None))
    _err(lib, call(term=-2))
    _err(lib, call(term=256))
    _err(lib, call(wsb=ws - 1))
    _err(lib, call(maxr=1 << 20))         # the workspace is short for these ranges


# ---- the CLI

def test_usage_names_the_extract_options(lib):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "  -C " in r.stdout and "  -T " in r.stdout and "  -V " in r.stdout and "context" in r.stdout


def test_cli_refuses_bad_combinations(lib, tmp_path):
    """every refused combination is a usage error: its ERROR: line, the usage text and a failure, no device needed"""
    pats = tmp_path / "p.txt"
    pats.write_text("ab\n")
    data = tmp_path / "d.txt"
    data.write_text("ab\ncd\n")
    repl = tmp_path / "r.txt"
    repl.write_text("0 41\n")
    out = tmp_path / "out"
    base = [CLI, "-f", str(data), "-p", str(pats), "-B", "64", "-D", "0", "-G", "16", "-L", "64"]
    cases = [
        (["-C", "1"], "ERROR: -C needs -T: the directory the extracted lines go to"),
        (["-V"], "ERROR: -V needs -C and -T: it inverts the selection of the lines that are extracted"),
        (["-V", "-C", "1"], "ERROR: -V needs -C and -T"),
        (["-T", str(out)], "ERROR: -T needs -C: the lines of context around a selected line (-C 0: none)"),
        (["-C", "x", "-T", str(out)], "ERROR: -C takes N or N,M: the lines in front and behind, both >= 0"),
        (["-C", "-1", "-T", str(out)], "ERROR: -C takes N or N,M"),
        (["-C", "1,", "-T", str(out)], "ERROR: -C takes N or N,M"),
        (["-C", "1,2,3", "-T", str(out)], "ERROR: -C takes N or N,M"),
    ]
    refused = "ERROR: -C, -V and -T cannot be combined with -t, -F, -r, -O, -Q or -K"
    for extra in (["-t"], ["-F"], ["-r", str(repl), "-O", str(tmp_path / "o2")], ["-Q", str(pats)], ["-S", "-K", str(pats)]):
        cases.append((["-C", "1", "-T", str(out)] + extra, refused))
    cases.append((["-V", "-t"], refused))
    for extra, msg in cases:
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, extra
        assert msg in r.stdout, (extra, r.stdout[:400])
        assert "Usage:" in r.stdout, extra
    assert not out.exists()
