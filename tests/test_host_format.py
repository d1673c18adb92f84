"""The per-line context pass and the format pass on the host, no GPU needed: the model the GPU tests compare with
(tests/format_model.py) against an independent brute force, per line and per byte, and against GNU grep (-H -n -b with
-A/-B/-C/-v, and -H -n -b -o) where it is installed; the exported symbols, the workspace queries and every argument
error of the two entry points; the CLI's new ERROR: lines."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import extract_model as xm
import format_model as fm
import line_model as lm
from gpu_pattern_matching_amd import _lib
from test_host_extract import CLI, CONTEXTS, GREP_TEXTS, brute_context, occurrences, random_text
from test_host_lines import brute_lines

ACM_ERR_ARG = -1
INT32_MAX = 0x7FFFFFFF


# ---- brute force

def brute_context_lines(text, d, origin, offsets, invert, before, after, seg):
    """[(line, begin, next, kind)] and (selected, kept, groups) by loops over lines"""
    lines = [(b + origin, e + origin) for b, e in brute_lines(text, d, True)]
    sel = [any(b <= o < e for o in offsets) != invert for b, e in lines]
    tid = [sum(1 for s in seg if s <= b) for b, _ in lines]
    kept = [any(sel[i] and tid[i] == tid[j] and j - after <= i <= j + before for i in range(len(lines))) for j in range(len(lines))]
    out, groups = [], 0
    for j, (b, e) in enumerate(lines):
        if not kept[j]:
            continue
        head = j == 0 or not kept[j - 1] or tid[j - 1] != tid[j]
        groups += head
        out.append((j, b, e, (1 if sel[j] else 0) + (2 if head else 0)))
    return out, (sum(sel), sum(kept), groups)


def decimal(v):
    """the digits of v >= 0, one division at a time"""
    out = bytearray()
    while True:
        out.insert(0, 0x30 + v % 10)
        v //= 10
        if not v:
            return bytes(out)


def brute_format(text, origin, ranges, kinds, nums, flags, seg, seg_num, nbase, obase, sel_sep, ctx_sep, names, name_off,
                 names_bytes, glue, term):
    """(out, at, seg_out, used, skipped, terminators, text bytes) byte by byte"""
    out, at, contrib = bytearray(), [], []
    used = skipped = terms = src = 0
    last_tid = None
    for i, (b, e) in enumerate(ranges):
        if b < origin or b >= e or e > origin + len(text):
            skipped += 1
            continue
        tid = 0
        for s in seg:
            if s <= b:
                tid += 1
        kind = kinds[i] if kinds is not None else 1
        sep = sel_sep if kind & 1 else ctx_sep
        before = len(out)
        if kind & 2 and last_tid == tid:
            for g in glue:
                out.append(g)
        if flags & fm.NAME:
            lo, hi = name_off[tid], name_off[tid + 1]
            if not (lo < 0 or hi < lo or hi > names_bytes or hi - lo > 4096):
                for x in range(lo, hi):
                    out.append(names[x])
            out.append(sep)
        if flags & fm.NUMBER:
            v = nbase + nums[i] - (seg_num[tid - 1] if tid > 0 and seg_num is not None else 0)
            out += decimal(v if v > 0 else 0)
            out.append(sep)
        if flags & fm.OFFSET:
            v = obase + b - (seg[tid - 1] if tid > 0 else origin)
            out += decimal(v if v > 0 else 0)
            out.append(sep)
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


def test_model_context_lines_matches_brute_force():
    rng = np.random.default_rng(41)
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
        got, ctx_info = fm.context_lines(st, info, origin, origin + n, offs, invert, before, after, seg)
        exp, figures = brute_context_lines(t, d, origin, list(offs), invert, before, after, list(seg))
        assert list(zip(*[g.tolist() for g in got])) == exp, (t, offs, seg, before, after, invert)
        assert ctx_info.tolist() == list(figures) + [0] and ctx_info.dtype == np.int32
        # the group form's entries, by its own brute force, from the kind bits
        groups, _ = brute_context(t, d, origin, list(offs), invert, before, after, list(seg))
        assert list(zip(*[g.tolist() for g in fm.groups_of(got)])) == groups
        cases += 1
    assert cases >= 300


def test_model_format_matches_brute_force():
    rng = np.random.default_rng(43)
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
        flags = int(rng.integers(0, 16))
        incl = bool(flags & 1)
        glue = (b"", b"-", b"--\n", b"0123456789abcdef")[cases % 4]
        term = (-1, 0x0A, 0x61)[cases % 3]
        seg = np.sort(rng.integers(origin - 1, origin + n + 2, size=int(rng.integers(1, 4)))) if cases % 2 else None
        nseg = 0 if seg is None else len(seg)
        count = (k, k + 3, -2, max(k - 1, 0))[cases % 4]        # the header cell may hold anything
        max_ranges = (k, max(k - 2, 0))[cases % 5 == 0]
        kinds = rng.integers(-8, 8, size=k) if cases % 3 else None
        nums = rng.integers(-3, 1000, size=k)
        seg_num = rng.integers(0, 20, size=nseg) if seg is not None and cases % 4 < 2 else None
        nbase, obase = int(rng.integers(0, 3)), (0, 10 ** 18)[cases % 6 == 0]
        names = bytes(rng.integers(0x41, 0x5B, size=40).astype(np.uint8))
        name_off = np.sort(rng.integers(0, 41, size=nseg + 2)) if cases % 7 else rng.integers(-5, 60, size=nseg + 2)
        names_bytes = (40, 20)[cases % 9 == 0]
        bp, ep = fm.plane_of(b, count), fm.plane_of(e - (1 if incl else 0), count)
        args = (t, origin, bp, ep, max_ranges, flags, fm.plane_of(kinds, count) if kinds is not None else None, fm.plane_of(nums, count),
                seg_num, nbase, obase, 0x3A, 0x2D, names, name_off, names_bytes, glue, term, seg)
        got = fm.format(*args)
        looked = min(max(count, 0), max_ranges)
        exp = brute_format(t, origin, list(zip(b.tolist(), e.tolist()))[:looked], None if kinds is None else kinds.tolist(),
                           nums.tolist(), flags, [] if seg is None else seg.tolist(), None if seg_num is None else seg_num.tolist(),
                           nbase, obase, 0x3A, 0x2D, names, name_off.tolist(), names_bytes, glue, term)
        assert got["out"] == exp[0] and got["m"] == len(exp[0]) and got["at"] == exp[1], (cases, got["out"], exp[0])
        assert (got["seg_out"] is None) == (seg is None)
        if seg is not None:
            assert got["seg_out"].tolist() == exp[2]
        assert got["info"].tolist() == [exp[3], exp[4], len(exp[0]), 0, exp[6], 0, 0, exp[5]]
        for limit in (0, 1, len(exp[0]) // 2, len(exp[0])):
            cut = fm.format(*args, limit=limit)
            assert cut["out"] == exp[0][:limit] and cut["info"][6] == int(len(exp[0]) > limit)
        if flags & ~1 == 0 and kinds is None:       # no prefix, no kinds: the extract without a glue
            ex = xm.extract(t, origin, bp, ep, max_ranges, incl, b"", term, seg)
            assert ex["out"] == got["out"] and ex["at"] == got["at"] and ex["info"].tolist() == got["info"].tolist()
        cases += 1
    assert cases >= 300


def test_lines_with_a_glue_give_the_group_forms_bytes():
    rng = np.random.default_rng(44)
    for n in range(0, 80):
        t = random_text(rng, n, 0x0A) + b"\n"           # every line keeps its delimiter
        offs = np.unique(rng.integers(0, n + 1, size=3))
        seg = [0, int(rng.integers(0, n + 2))]
        _, info, st = lm.index(t)
        for before, after in ((0, 0), (1, 0), (1, 2)):
            lines, _ = fm.context_lines(st, info, 0, len(t), offs, False, before, after, seg)
            groups, _ = xm.context(st, info, 0, len(t), offs, False, before, after, seg)
            a = fm.format(t, 0, fm.plane_of(lines[1]), fm.plane_of(lines[2]), len(lines[1]), 0, fm.plane_of(lines[3]), glue=b"--\n",
                          terminator=0x0A, seg_start=seg)
            b = xm.extract(t, 0, xm.plane_of(groups[1]), xm.plane_of(groups[2]), len(groups[1]), glue=b"--\n", terminator=0x0A,
                           seg_start=seg)
            assert a["out"] == b["out"] and a["seg_out"].tolist() == b["seg_out"].tolist()


# ---- GNU grep

GREP = shutil.which("grep")


def grep_output(text, pat, name, before=0, after=0, invert=False, only=False):
    cmd = [GREP, "-a", "-F", "-H", "-n", "-b", "--label=" + name, "-e", pat.decode()]
    if before + after > 0:
        cmd += ["-B", str(before), "-A", str(after)]
    if invert:
        cmd.append("-v")
    if only:
        cmd.append("-o")
    r = subprocess.run(cmd, input=text, capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=60)
    assert r.returncode in (0, 1), r.stderr
    return r.stdout


@pytest.mark.skipif(GREP is None, reason="grep is not installed")
def test_model_matches_gnu_grep():
    runs = 0
    for t in GREP_TEXTS:
        for pat in (b"abc", b"c", b"1"):
            offs = occurrences(t, pat)
            for before, after in ((0, 0), (1, 1), (2, 2), (0, 2), (3, 0), (1, 3), (100, 100)):
                for invert in (False, True):
                    got = fm.grep_like(t, offs, before, after, invert, names=[b"some/file"], with_name=True, line_number=True,
                                       byte_offset=True)[0]
                    assert got == grep_output(t, pat, "some/file", before, after, invert), (t, pat, before, after, invert)
                    runs += 1
    assert runs > 400


@pytest.mark.skipif(GREP is None, reason="grep is not installed")
def test_model_matches_gnu_grep_only_matching():
    """grep -H -n -b -o: the prefix in front of every match, the line and the offset of the match itself"""
    runs = 0
    for t in GREP_TEXTS:
        for pat in (b"abc", b"c", b"1", b"cc"):
            starts, at = [], t.find(pat)
            while at >= 0:                       # leftmost, non-overlapping
                starts.append(at)
                at = t.find(pat, at + len(pat))
            s = np.asarray(starts, dtype=np.int64)
            _, info, st = lm.index(t)
            names, off = fm.name_table([b"f"], 0)
            got = fm.format(t, 0, fm.plane_of(s), fm.plane_of(s + len(pat) - 1), len(s), fm.END_INCLUSIVE | fm.NAME | fm.NUMBER | fm.OFFSET,
                            None, fm.plane_of(lm.number(st, info, s)), None, 1, 0, 0x3A, 0x2D, names, off, terminator=0x0A)
            assert got["out"] == grep_output(t, pat, "f", only=True), (t, pat)
            runs += 1
    assert runs > 40


def test_each_text_is_numbered_alone():
    texts = [b"a\nabc\nb\n", b"", b"abc", b"x\ny\nabc\nz\n"]          # the third has no final newline: the index gets one there
    names = [b"one", b"two", b"three", b"dir/four"]
    starts = np.cumsum([0] + [len(x) for x in texts[:-1]])
    whole = b"".join(texts)
    assert whole[starts[3] - 1:starts[3]] == b"c"
    # as the callers do: the lines are found over a copy in which every text ends in the delimiter
    fixed = bytearray(whole)
    fixed[starts[3] - 1] = 0x0A
    _, info, st = lm.index(bytes(fixed))
    offs = occurrences(whole, b"abc")
    lines, _ = fm.context_lines(st, info, 0, len(whole), offs, False, 1, 1, starts)
    tab, off = fm.name_table([b""] + names, 4)
    got = fm.format(whole, 0, fm.plane_of(lines[1]), fm.plane_of(lines[2]), len(lines[1]), fm.NAME | fm.NUMBER | fm.OFFSET,
                    fm.plane_of(lines[3]), fm.plane_of(lines[0]), lm.number(st, info, starts), 1, 0, 0x3A, 0x2D, tab, off, None,
                    b"--\n", 0x0A, [int(x) for x in starts])
    assert got["out"] == (b"one-1-0-a\none:2:2:abc\none-3-6-b\n" + b"three:1:0:abc\n" + b"dir/four-2-2-y\ndir/four:3:4:abc\ndir/four-4-8-z\n")
    if GREP:
        assert got["out"] == b"".join(grep_output(t, b"abc", n.decode(), 1, 1) for t, n in zip(texts, names))


# ---- the C ABI

def test_symbols_exported(lib):
    for name in ("acm_line_context_lines_workspace_bytes", "acm_line_context_lines_async", "acm_format_workspace_bytes",
                 "acm_format_async"):
        assert hasattr(lib, name), name
        assert name in _lib.NATIVE_API
    assert (_lib.FORMAT_NAME, _lib.FORMAT_NUMBER, _lib.FORMAT_OFFSET, _lib.FORMAT_MAX_NAME) == (2, 4, 8, 4096)
    assert (_lib.LINE_SELECTED, _lib.LINE_GROUP_HEAD) == (1, 2)


SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 20) + 3, 1 << 25, (1 << 31) - 17)


def test_workspace_queries(lib):
    for fn in (lib.acm_line_context_lines_workspace_bytes, lib.acm_format_workspace_bytes):
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


def test_context_lines_argument_errors(lib):
    buf = (C.c_char * 16384)()
    a = (C.addressof(buf) + 15) & ~15     # never dereferenced: every call fails before anything is enqueued
    ws = lib.acm_line_context_lines_workspace_bytes(8, 2)
    ok = dict(ls=a, cap=8, info=a + 64, origin=0, end=64, off=a + 128, maxr=4, inv=0, before=1, after=1, seg=a + 192, nseg=2,
              rel=a + 256, beg=a + 512, nxt=a + 768, kind=a + 1024, ocap=8, cinfo=a + 1280, ws=a + 2048, wsb=ws)

    def call(**kw):
        k = dict(ok, **kw)
        return lib.acm_line_context_lines_async(k["ls"], k["cap"], k["info"], k["origin"], k["end"], k["off"], k["maxr"], k["inv"],
                                                k["before"], k["after"], k["seg"], k["nseg"], k["rel"], k["beg"], k["nxt"],
                                                k["kind"], k["ocap"], k["cinfo"], k["ws"], k["wsb"], None)
    for name in ("ls", "info", "off", "rel", "beg", "nxt", "kind", "cinfo", "ws"):
        _err(lib, call(**{name: None}))
    _err(lib, call(cap=0))
    _err(lib, call(ocap=1))
    _err(lib, call(wsb=ws - 1))
    _err(lib, call(end=-1))
    _err(lib, call(before=-1))
    _err(lib, call(after=-1))
    _err(lib, call(maxr=(1 << 31) - 1))
    _err(lib, call(seg=None))             # segments without their starts
    _err(lib, call(nseg=0))               # starts without segments
    _err(lib, call(cap=1 << 20))          # the workspace is short for this capacity


def test_format_argument_errors(lib):
    buf = (C.c_char * 16384)()
    a = (C.addressof(buf) + 15) & ~15     # never dereferenced: every call fails before anything is enqueued
    ws = lib.acm_format_workspace_bytes(8, 2)
    ok = dict(text=a, n=64, origin=0, bp=a + 128, ep=a + 256, maxr=8, flags=14, kind=a + 384, num=a + 448, segnum=a + 480, nbase=1,
              obase=0, sel=0x3A, ctx=0x2D, names=a + 3000, noff=a + 3100, nbytes=50, glue=b"--\n", glen=3, term=10, out=a + 512,
              ocap=256, at=a + 1024, acap=10, seg=a + 1280, nseg=2, sout=a + 1344, info=a + 1408, ws=a + 4096, wsb=ws)

    def call(**kw):
        k = dict(ok, **kw)
        return lib.acm_format_async(k["text"], k["n"], k["origin"], k["bp"], k["ep"], k["maxr"], k["flags"], k["kind"], k["num"],
                                    k["segnum"], k["nbase"], k["obase"], k["sel"], k["ctx"], k["names"], k["noff"], k["nbytes"],
                                    k["glue"], k["glen"], k["term"], k["out"], k["ocap"], k["at"], k["acap"], k["seg"], k["nseg"],
                                    k["sout"], k["info"], k["ws"], k["wsb"], None)
    # the extract's list
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
    _err(lib, call(glen=-1))
    _err(lib, call(glen=17))
    _err(lib, call(glue=None))
    _err(lib, call(term=-2))
    _err(lib, call(term=256))
    _err(lib, call(wsb=ws - 1))
    _err(lib, call(maxr=1 << 20))         # the workspace is short for these ranges
    # its own
    _err(lib, call(flags=16))
    _err(lib, call(flags=0x80000002))
    _err(lib, call(names=None))           # ACM_FORMAT_NAME without both name arrays
    _err(lib, call(noff=None))
    _err(lib, call(nbytes=1 << 31))
    _err(lib, call(num=None))             # ACM_FORMAT_NUMBER without its plane
    _err(lib, call(nbase=-1))
    _err(lib, call(nbase=10 ** 18 + 1))
    _err(lib, call(obase=-1))
    _err(lib, call(obase=10 ** 18 + 1))
    for sep in ("sel", "ctx"):
        _err(lib, call(**{sep: -1}))
        _err(lib, call(**{sep: 256}))


# ---- the CLI

def test_usage_names_the_format_options(lib):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "  -H " in r.stdout and "  -N " in r.stdout and "  -b " in r.stdout and "name:line:offset:" in r.stdout


def test_cli_refuses_prefixes_without_the_extract(lib, tmp_path):
    """-H, -N and -b need -C and -T: an ERROR: line, the usage text and a failure, no device needed"""
    pats = tmp_path / "p.txt"
    pats.write_text("ab\n")
    data = tmp_path / "d.txt"
    data.write_text("ab\ncd\n")
    out = tmp_path / "out"
    base = [CLI, "-f", str(data), "-p", str(pats), "-B", "64", "-D", "0", "-G", "16", "-L", "64"]
    msg = "ERROR: -H, -N and -b need -C and -T: they put a prefix in front of the lines that are extracted"
    for flag in ("-H", "-N", "-b"):
        for extra in ([], ["-C", "1"], ["-T", str(out)], ["-V"]):
            r = subprocess.run(base + [flag] + extra, capture_output=True, text=True, timeout=60)
            assert r.returncode != 0, (flag, extra)
            assert msg in r.stdout, (flag, extra, r.stdout[:400])
            assert "Usage:" in r.stdout
    r = subprocess.run(base + ["-H", "-N", "-b", "-C", "1", "-T", str(out), "-t"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "ERROR: -C, -V and -T cannot be combined with -t" in r.stdout
    assert not out.exists()
