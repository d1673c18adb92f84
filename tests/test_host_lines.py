"""The line index on the host, no GPU needed: the numpy model the GPU tests compare with, checked against
an independent brute force (bytes.split and a per-byte loop); the exported symbols, the workspace queries
and every argument error of the three passes; the CLI's usage text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import line_model as lm
from gpu_pattern_matching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpu_pattern_matching_amd", "acm_grep")
ACM_ERR_ARG = -1
DELIMS = (0x0A, 0x00, 0xFF)


def brute_index(text, origin, d, begins):
    """(starts, delimiters, origin is a start, next origin is a start) by a per-byte loop"""
    text = bytes(text)
    starts = [origin] if text and begins else []
    delims = 0
    for i, b in enumerate(text):
        if b == d:
            delims += 1
            if i + 1 < len(text):
                starts.append(origin + i + 1)
    nxt = (text[-1] == d) if text else begins
    return starts, delims, int(bool(text) and begins), int(nxt)


def brute_lines(text, d, begins):
    """the lines of a piece with bytes.split: (begin, next) relative to the piece, delimiter kept"""
    text = bytes(text)
    parts = text.split(bytes([d]))
    out, pos = [], 0
    for j, p in enumerate(parts):
        size = len(p) + (1 if j + 1 < len(parts) else 0)
        if size:
            out.append((pos, pos + size))
        pos += size
    return out


def texts():
    rng = np.random.default_rng(11)
    out = []
    for n in range(0, 49):
        for d in DELIMS:
            out.append((bytes([d]) * n, d))                                        # only delimiters
            out.append((bytes(rng.choice([1, 65, 66], size=n).astype(np.uint8)), d))   # none
            for dens in (0.03, 0.3, 0.8):
                t = rng.integers(1, 255, size=n).astype(np.uint8)
                t[t == d] = 7
                t[rng.random(n) < dens] = d
                out.append((bytes(t), d))
    return out


TEXTS = texts()


def prev_cases(d):
    return [(-1, True), (d, True), ((d + 1) % 256, False), (0x41, d == 0x41)]


def test_model_index_matches_brute_force():
    for t, d in TEXTS:
        for prev, begins in prev_cases(d):
            for origin in (0, 1000):
                ls, info, starts = lm.index(t, origin, d, prev)
                bs, bd, b2, b3 = brute_index(t, origin, d, begins)
                assert starts.tolist() == bs
                assert info.tolist() == [len(bs), bd, b2, b3, 0, 0, 0, 0] and info.dtype == np.int32
                assert ls.tolist() == bs
                for cap in (1, 3, len(bs) + 5):
                    ls2 = lm.index(t, origin, d, prev, capacity=cap)[0]
                    assert ls2.dtype == np.int32 and ls2.size == cap
                    assert ls2.tolist() == (bs + [0x7FFFFFFF] * cap)[:cap]


def test_model_counts_lines_as_wc_does():
    ls, info, starts = lm.index(b"a\nb\n")
    assert starts.tolist() == [0, 2] and info[1] == 2 and info[3] == 1
    ls, info, starts = lm.index(b"a\nb")
    assert starts.tolist() == [0, 2] and info[1] == 1 and info[3] == 0


def test_model_lines_match_split():
    for t, d in TEXTS:
        for prev, begins in prev_cases(d):
            _, info, starts = lm.index(t, 50, d, prev)
            rel, begin, nxt = lm.lines_of(starts, info, 50, 50 + len(t))
            exp = brute_lines(t, d, begins)
            assert [(int(b) - 50, int(e) - 50) for b, e in zip(begin, nxt)] == exp
            assert rel.tolist() == list(range(len(exp)))
            # every line but the last ends with the delimiter and holds no other
            for j, (b, e) in enumerate(exp):
                assert t[b:e].count(bytes([d])) == (1 if t[e - 1] == d else 0)
                assert j + 1 == len(exp) or t[e - 1] == d


def test_model_number_matches_brute_force():
    rng = np.random.default_rng(5)
    for t, d in TEXTS[::3]:
        if not t:
            continue
        for prev, _ in prev_cases(d)[:3]:
            _, info, starts = lm.index(t, 7, d, prev)
            offs = rng.integers(0, len(t), size=12)
            got = lm.number(starts, info, offs + 7)
            assert got.dtype == np.int32
            assert got.tolist() == [t[:int(o)].count(bytes([d])) for o in offs]


def test_model_select_matches_brute_force():
    rng = np.random.default_rng(6)
    for t, d in TEXTS[::3]:
        for prev, begins in prev_cases(d)[:3]:
            _, info, starts = lm.index(t, 7, d, prev)
            offs = np.unique(rng.integers(0, max(len(t), 1), size=5)) if t else np.zeros(0, dtype=np.int64)
            lines = brute_lines(t, d, begins)
            hit = [any(b <= o < e for o in offs) for b, e in lines]
            got = {}
            for inv in (False, True):
                rel, begin, nxt = lm.select(starts, info, 7, 7 + len(t), offs + 7, inv)
                exp = [(j, b + 7, e + 7) for j, ((b, e), h) in enumerate(zip(lines, hit)) if h != inv]
                assert list(zip(rel.tolist(), begin.tolist(), nxt.tolist())) == exp
                got[inv] = set(rel.tolist())
                # rel is what the number pass gives for the line's first byte
                assert lm.number(starts, info, begin).tolist() == rel.tolist()
            assert not (got[False] & got[True]) and len(got[False] | got[True]) == len(lines)


def test_model_chained_pieces_equal_one_call():
    rng = np.random.default_rng(9)
    for d in DELIMS:
        for prev in (-1, d, 0x41 if d != 0x41 else 0x42):
            t = rng.integers(1, 255, size=23).astype(np.uint8)
            t[t == d] = 9
            t[rng.random(23) < 0.35] = d
            t = bytes(t)
            whole_ls, whole_info, whole = lm.index(t, 100, d, prev)
            for a in range(0, len(t) + 1):
                for b in range(a, len(t) + 1):
                    res = lm.chain([t[:a], t[a:b], t[b:]], 100, d, prev)
                    assert np.concatenate([r[2] for r in res]).tolist() == whole.tolist()
                    assert sum(int(r[1][1]) for r in res) == int(whole_info[1])
                    assert int(res[-1][1][3]) == int(whole_info[3])
                    assert lm.stream_delims(res[1][1]) == t[:a].count(bytes([d]))
                    assert lm.stream_delims(res[2][1]) == t[:b].count(bytes([d]))
                    # the line number of every offset: through its own piece, and through the whole
                    o = np.arange(b, len(t)) + 100
                    if o.size:
                        through = lm.stream_delims(res[2][1]) + lm.number(res[2][2], res[2][1], o)
                        assert through.tolist() == lm.number(whole, whole_info, o).tolist()


def test_model_planes():
    p = lm.planes(([1, 2, 3], [10, 20, 30], [20, 30, 40]), 4, -1)
    assert p[0].tolist() == [3, 1, 2, 0] and p[2].tolist() == [3, 20, 30, 0]
    p = lm.planes(([1], [10], [20]), 5, -1)
    assert p[1].tolist() == [1, 10, 0, -1, -1]


def test_symbols_exported(lib):
    for name in ("acm_line_index_workspace_bytes", "acm_line_index_async", "acm_line_number_async",
                 "acm_line_select_workspace_bytes", "acm_line_select_async"):
        assert hasattr(lib, name), name
        assert name in _lib.NATIVE_API


def test_workspace_queries(lib):
    for fn in (lib.acm_line_index_workspace_bytes, lib.acm_line_select_workspace_bytes):
        prev = 0
        for n in (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 20) + 3, 1 << 25, (1 << 31) - 17):
            b = fn(n)
            assert b > 0 and b % 256 == 0 and b >= prev
            prev = b
    assert lib.acm_line_index_workspace_bytes(1 << 25) >= (1 << 25) // 8


def _err(lib, rc):
    assert rc == ACM_ERR_ARG
    assert lib.acm_last_error()


def test_index_argument_errors(lib):
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 15) & ~15     # never dereferenced: every call fails before anything is enqueued
    ws = lib.acm_line_index_workspace_bytes(64)
    ok = dict(text=a, n=64, origin=0, d=10, prev=-1, pinfo=None, out=a + 256, cap=8, info=a + 512, ws=a + 1024, wsb=ws)

    def call(**kw):
        k = dict(ok, **kw)
        return lib.acm_line_index_async(k["text"], k["n"], k["origin"], k["d"], k["prev"], k["pinfo"], k["out"], k["cap"],
                                        k["info"], k["ws"], k["wsb"], None)
    _err(lib, call(out=None))
    _err(lib, call(info=None))
    _err(lib, call(cap=0))
    _err(lib, call(text=a + 4))
    _err(lib, call(n=(1 << 31) - 16))
    _err(lib, call(d=-1))
    _err(lib, call(d=256))
    _err(lib, call(prev=-2))
    _err(lib, call(prev=256))
    _err(lib, call(wsb=ws - 1))
    _err(lib, call(ws=None))
    _err(lib, call(n=1 << 20))            # the workspace is short for this text


def test_number_and_select_argument_errors(lib):
    buf = (C.c_char * 8192)()
    a = (C.addressof(buf) + 15) & ~15
    num = lambda ls=a, cap=8, info=a + 64, offs=a + 128, cnt=None, count=4, out=a + 256: \
        lib.acm_line_number_async(ls, cap, info, offs, cnt, count, out, None)
    _err(lib, num(ls=None))
    _err(lib, num(info=None))
    _err(lib, num(offs=None))
    _err(lib, num(out=None))
    _err(lib, num(cap=0))
    ws = lib.acm_line_select_workspace_bytes(8)
    ok = dict(ls=a, cap=8, info=a + 64, origin=0, end=64, off=a + 128, maxr=4, inv=0, rel=a + 256, beg=a + 512, nxt=a + 768,
              ocap=8, ws=a + 1024, wsb=ws)

    def sel(**kw):
        k = dict(ok, **kw)
        return lib.acm_line_select_async(k["ls"], k["cap"], k["info"], k["origin"], k["end"], k["off"], k["maxr"], k["inv"],
                                         k["rel"], k["beg"], k["nxt"], k["ocap"], k["ws"], k["wsb"], None)
    for name in ("ls", "info", "off", "rel", "beg", "nxt", "ws"):
        _err(lib, sel(**{name: None}))
    _err(lib, sel(cap=0))
    _err(lib, sel(ocap=1))
    _err(lib, sel(wsb=ws - 1))
    _err(lib, sel(end=-1))


def test_usage_names_line_numbers(lib):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "-n " in r.stdout and "line number" in r.stdout
