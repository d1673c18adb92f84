"""Match rewriting in Python (test infrastructure only, not a conftest): the rule of acm_rewrite_async, written from
include/acmatch.h, as one serial splice.

A record (p, o) of pattern p spans [s, e] as in select_model.SelectModel.  It is USED iff p is a pattern index, its
length is >= 1 and text_origin <= s <= e < text_end; every other record is skipped and counted.  The output is the
text with every used span replaced: by the pattern's bytes, by its fill byte once per byte of the span, or (no
replacement) by the span itself.

  RewriteModel   run(): output bytes, info[8], where every used record's replacement begins, where every start lies
  occurrences    every occurrence of every pattern in every text, each text alone (bytes.find)
  selected       the records the select pass leaves for those occurrences (SelectModel)
  re_sub         the same rewrite by re.sub over an alternation sorted by descending length: an independent oracle
                 for sets of distinct literal patterns
"""
import re

import numpy as np

import select_model as sel

INT32_MAX = 0x7FFFFFFF
INT32_MIN = -(2 ** 31)


def sat32(v):
    return max(INT32_MIN, min(int(v), INT32_MAX))


def pair(v):
    """the int64 v as the int32 pair (lo, hi)"""
    lo = v & 0xFFFFFFFF
    return [lo - (1 << 32) if lo >= 1 << 31 else lo, v >> 32]


class RewriteModel:
    """pat_lens: the length of every pattern; repl: per pattern None (copied), (bytes, False) or (one byte, True: a
    fill); pre, post: the wildcard context of every pattern (default: none)"""

    def __init__(self, pat_lens, repl=None, pre=None, post=None):
        self.sel = sel.SelectModel(pat_lens, pre, post)
        self.repl = list(repl) if repl is not None else [None] * len(pat_lens)

    def used(self, cells, offs, n, origin=0):
        """(s, e, used) of every record"""
        s, e, real, _ = self.sel.spans(cells, offs, origin)
        return s, e, real & (s >= origin) & (s <= e) & (e < origin + n)

    def run(self, text, cells, offs, origin=0, seg_start=None, cap=None, have_out=True):
        """(out bytes, info[8], at, seg_out) for spans that are disjoint and ascending.  out is the whole output;
        the call stores its first min(m, cap) bytes and info[6] says whether that cut it."""
        text = bytes(text)
        n = len(text)
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        s, e, used = self.used(cells, offs, n, origin)
        pieces, at, starts, deltas = [], [], [], []
        cursor, m, src = 0, 0, 0                                  # cursor: the first text byte not yet copied
        for a, b, p in zip((s[used] - origin).tolist(), (e[used] - origin + 1).tolist(), cells[used].tolist()):
            assert a >= cursor, "the model takes disjoint ascending spans"
            r = self.repl[p]
            new = text[a:b] if r is None else r[0] * (b - a) if r[1] else r[0]
            pieces += [text[cursor:a], new]
            m += a - cursor
            at.append(sat32(m))
            m += len(new)
            src += b - a
            starts.append(a + origin)
            deltas.append(len(new) - (b - a))
            cursor = b
        pieces.append(text[cursor:])
        m += n - cursor
        out = b"".join(pieces)
        assert len(out) == m
        k = int(used.sum())
        info = [k, int(cells.size) - k] + pair(m) + pair(src) + [int(have_out and cap is not None and m > cap), 0]
        seg_out = None
        if seg_start is not None:
            before = np.concatenate([[0], np.cumsum(np.asarray(deltas, dtype=np.int64))])
            st = np.asarray(starts, dtype=np.int64)
            seg_out = [sat32(min(max(int(x), origin), origin + n) - origin + int(before[np.searchsorted(st, int(x), "left")]))
                       for x in np.asarray(seg_start, dtype=np.int64)]
        return out, info, at, seg_out


def occurrences(pats, texts, nocase=False, windows=None):
    """(cells, offsets) of every occurrence of every pattern in every text, each text alone, in offset order.  pats:
    bytes, or (bytes, nocase) for a mixed set; windows {pattern: (lo, hi or None, from_end)}: position constraints"""
    windows = windows or {}
    out, base = [], 0
    for t in texts:
        t = bytes(t)
        for i, p in enumerate(pats):
            p, nc = p if isinstance(p, tuple) else (p, nocase)
            hay, needle = (t.upper(), p.upper()) if nc else (t, p)
            lo, hi, fe = windows.get(i, (0, None, False))
            k = hay.find(needle) if needle else -1
            while k >= 0:
                v = len(t) - k if fe else k
                if lo <= v and (hi is None or v <= hi):
                    out.append((base + k + len(p) - 1, i))
                k = hay.find(needle, k + 1)
        base += len(t)
    out.sort()
    return np.array([c for _, c in out], dtype=np.int64), np.array([o for o, _ in out], dtype=np.int64)


def selected(pats, texts, nocase=False, min_start=0):
    """(cells, offsets) the select pass leaves for the occurrences of pats in texts"""
    cells, offs = occurrences(pats, texts, nocase)
    ep, eo, _, _ = sel.SelectModel([len(p) for p in pats]).run(cells, offs, min_start)
    return ep.astype(np.int64), eo.astype(np.int64)


def re_sub(pats, repl, text, nocase=False):
    """text rewritten by re.sub: distinct literal patterns of length >= 1, the alternation sorted by descending
    length (the first alternative that matches at a byte is then the longest: leftmost-longest)"""
    key = (lambda b: b.upper()) if nocase else (lambda b: b)
    index = {key(p): i for i, p in enumerate(pats)}
    assert len(index) == len(pats)
    rx = re.compile(b"|".join(re.escape(p) for p in sorted(pats, key=len, reverse=True)), re.I if nocase else 0)

    def one(mt):
        r = repl[index[key(mt.group(0))]]
        return mt.group(0) if r is None else r[0] * len(mt.group(0)) if r[1] else r[0]
    return rx.sub(one, bytes(text))
