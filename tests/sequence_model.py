"""Ordered multi-part signatures in Python (test infrastructure only, not a conftest): the rule of
acm_sequence_matches_async and the signature grammar of acm_automaton_add_signature, written from
include/acmatch.h.

A sequence is parts p_0 .. p_{k-1} (pattern indices) with a gap (lo, hi or None) in front of every part but
the first.  An occurrence of pattern p (length L) that ends at e starts at a = e - L + 1 and lies in the text
that begins at T0.  Level by level: a level-0 record is alive iff a >= T0; a level-j record is alive iff some
alive level-(j-1) record of its sequence ends in [max(a - 1 - hi, T0), a - 1 - lo] (hi None: [T0, a - 1 - lo]).
An alive record of a last part is a match: (sequence index, e).

  SequenceModel   the level rule in numpy over (pattern, offset) entries, whatever the cells hold
  brute_force     bytes.find for every part and a chain search over the occurrences, without an automaton
  regex_force     the same statement as a regular expression, A(?s:.){lo,hi}B...\\Z on every prefix
  parse_body      the signature grammar: hex byte pairs, ??, *, {n}, {n-m}, {-m}, {n-}
"""
import re

import numpy as np

from gpu_pattern_matching_amd import Automaton

import position_model as pm

UNB = 0x7FFFFFFF
MAX_PARTS = 32


def build(pats, seqs, windows=None, compile_first=False):
    """a compiled Automaton of pats (bytes, or (bytes, nocase) pairs) with the sequences seqs: a list of
    (parts, gaps) or (parts, gaps, iid); windows {index: (lo, hi, from_end)}.  compile_first: the sequences
    are added behind compile()"""
    a = Automaton()
    for i, p in enumerate(pats):
        if isinstance(p, tuple):
            a.add(p[0], i, nocase=p[1])
        else:
            a.add(p, i)
    if compile_first:
        a.compile()
    for s in seqs:
        a.add_sequence(s[0], s[1], s[2] if len(s) > 2 else 0)
    if not compile_first:
        a.compile()
    for i, (lo, hi, fe) in (windows or {}).items():
        a.set_position(i, lo, hi, fe)
    return a


class SequenceModel:
    """pat_lens: the length of every pattern; seqs: a list of (parts, gaps[, iid])"""

    def __init__(self, pat_lens, seqs):
        self.len = np.asarray(pat_lens, dtype=np.int64)
        self.seqs = [(list(s[0]), [(lo, UNB if hi is None else hi) for lo, hi in s[1]]) for s in seqs]
        self.seq_of = np.full(self.len.size, -1, dtype=np.int64)
        self.last = np.zeros(self.len.size, dtype=bool)
        for q, (parts, gaps) in enumerate(self.seqs):
            assert len(gaps) == len(parts) - 1
            for p in parts:
                assert self.seq_of[p] < 0 and self.len[p] > 0
                self.seq_of[p] = q
            self.last[parts[-1]] = True

    def run(self, cells, offs, starts=(), lead_begin=0):
        """(sequences int32, offsets int64, info[4]) the pass writes for the cells (pattern form), whatever they hold"""
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        valid = (cells >= 0) & (cells < self.len.size)
        p = np.where(valid, cells, 0)
        part = valid & (self.seq_of[p] >= 0)
        t0 = pm.bounds(offs, starts, lead_begin, 0, None)[0]
        a = offs - self.len[p] + 1
        alive = np.zeros(cells.size, dtype=bool)
        for parts, gaps in self.seqs:
            prev_ends = None
            for j, pj in enumerate(parts):
                idx = np.flatnonzero(part & (p == pj))
                if j == 0:
                    alive[idx] = a[idx] >= t0[idx]
                else:
                    lo, hi = gaps[j - 1]
                    upper = a[idx] - 1 - lo
                    lower = t0[idx] if hi == UNB else np.maximum(a[idx] - 1 - hi, t0[idx])
                    x = np.searchsorted(prev_ends, lower, side="left")
                    y = np.searchsorted(prev_ends, upper, side="right")
                    alive[idx] = y > x
                prev_ends = offs[idx[alive[idx]]]            # in input order: non-decreasing
        out = alive & self.last[p]
        return self.seq_of[p[out]].astype(np.int32), offs[out], [int(part.sum()), int(alive.sum()), 0, 0]


def occurrences(t, pat, nocase=False):
    """start of every occurrence of pat in t (overlapping ones too)"""
    if nocase:
        t, pat = t.upper(), pat.upper()
    out, k = [], t.find(pat)
    while k >= 0:
        out.append(k)
        k = t.find(pat, k + 1)
    return out


def brute_force(pats, seqs, texts, windows=None):
    """every (end offset in the concatenation, sequence index) pair: each part found in each text with bytes.find,
    then a search for a chain of occurrences whose gaps hold.  pats: bytes or (bytes, nocase); windows: {pattern:
    (lo, hi or None, from_end)} tested on every occurrence with the text's own bounds"""
    windows = windows or {}
    out, base = set(), 0
    for t in texts:
        t = bytes(t)
        for q, s in enumerate(seqs):
            parts, gaps = s[0], s[1]
            occ = []
            for pi in parts:
                pat, nc = pats[pi] if isinstance(pats[pi], tuple) else (pats[pi], False)
                lo, hi, fe = windows.get(pi, (0, None, False))
                ks = [k for k in occurrences(t, pat, nc)
                      if lo <= (len(t) - k if fe else k) and (hi is None or (len(t) - k if fe else k) <= hi)]
                occ.append([(k, k + len(pat) - 1) for k in ks])

            memo = {}

            def chain(j, end_before):
                """ends of the last part over the chains of parts j .. behind a part that ended at end_before"""
                if (j, end_before) in memo:
                    return memo[j, end_before]
                found = memo[j, end_before] = set()
                for a, e in occ[j]:
                    if j > 0:
                        lo, hi = gaps[j - 1]
                        gap = a - end_before - 1
                        if gap < lo or (hi is not None and gap > hi):
                            continue
                    if j + 1 == len(parts):
                        found.add(e)
                    else:
                        found |= chain(j + 1, e)
                return found
            out |= {(base + e, q) for e in chain(0, -1)}
        base += len(t)
    return out


def regex_force(pats, seqs, t):
    """every (end offset, sequence index) pair of one text: A(?s:.){lo,hi}B...\\Z searched on every prefix"""
    out = set()
    for q, s in enumerate(seqs):
        parts, gaps = s[0], s[1]
        if any(hi is not None and lo > hi for lo, hi in gaps):
            continue                                         # (never matches; re refuses min > max)
        rx = re.escape(pats[parts[0]])
        for pi, (lo, hi) in zip(parts[1:], gaps):
            rx += b"(?s:.){%d,%s}" % (lo, b"" if hi is None else b"%d" % hi) + re.escape(pats[pi])
        rx = re.compile(rx + b"\\Z")
        for o in range(len(t)):
            if rx.search(t[:o + 1]):
                out.add((o, q))
    return out


_TOKEN = re.compile(rb"([0-9a-fA-F]{2})|(\?\?)|(\*)|\{(\d+)\}|\{(\d+)-(\d+)\}|\{-(\d+)\}|\{(\d+)-\}")


class BodyError(ValueError):
    def __init__(self, column):
        ValueError.__init__(self, "column %d" % column)
        self.column = column


def parse_body(body):
    """(parts: list of bytes, gaps: list of (lo, hi or None)) of a signature body; BodyError names the column
    (from 1) of the first byte that is wrong"""
    body = body.encode() if isinstance(body, str) else bytes(body)
    parts, gaps, cur, gap, pos = [], [], bytearray(), None, 0
    while pos < len(body):
        m = _TOKEN.match(body, pos)
        if not m:
            raise BodyError(pos + 1)
        if m.group(1):
            if gap is not None:
                gaps.append(gap)
                gap = None
            cur.append(int(m.group(1), 16))
        else:
            if m.group(2):
                lo, hi = 1, 1
            elif m.group(3):
                lo, hi = 0, None
            elif m.group(4):
                lo = hi = int(m.group(4))
            elif m.group(5):
                lo, hi = int(m.group(5)), int(m.group(6))
            elif m.group(7):
                lo, hi = 0, int(m.group(7))
            else:
                lo, hi = int(m.group(8)), None
            if gap is None:
                if not cur:
                    raise BodyError(pos + 1)                # a gap in front of the first part
                parts.append(bytes(cur))
                cur = bytearray()
                gap = (0, 0)
            gap = (gap[0] + lo, None if gap[1] is None or hi is None else gap[1] + hi)
            if max(lo, hi or 0, gap[0], gap[1] or 0) >= UNB:
                raise BodyError(pos + 1)
        pos = m.end()
    if gap is not None or not cur:
        raise BodyError(len(body) + 1)                      # a gap behind the last part, or nothing at all
    parts.append(bytes(cur))
    if len(parts) > MAX_PARTS:
        raise BodyError(len(body) + 1)
    return parts, gaps


def planes(seqs, offs, cap, poison, trailer):
    return pm.planes(seqs, offs, cap, poison, trailer)
