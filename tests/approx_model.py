"""Approximate patterns in Python (test infrastructure only, not a conftest): the piece layout of
acm_automaton_add_approx and the rule of acm_approx_matches_async, written from include/acmatch.h.

An approximate pattern is n bytes and a budget k; piece i of its k + 1 pieces covers [b_i, b_{i + 1}),
b_i = i * q + min(i, r), q = n // (k + 1), r = n % (k + 1).  Entry (p, o) -- pattern p of the automaton ends at
o -- in the text [T0, Tend) of its record:
  1. p is no piece: kept, distance 0     2. the span [s, s + n), s = o - L + 1 - b_j, leaves [T0, Tend): dropped
  3. the span leaves the bytes given: undecided (dropped and counted)
  4. kept iff m_j == 0, m_i > 0 for every i < j and the sum of the m_i <= k

  piece_bounds    [b_0, .., b_{k + 1}] of (n, k)
  brute_force     every alignment of every pattern in every text, Hamming distance <= k, without an automaton
  ApproxModel     the rule over (pattern, offset) entries, whatever the cells hold, and the walk
"""
import numpy as np

from gpu_pattern_matching_amd import Automaton

import position_model as pm

STATE, HEAD = 1, 0
DROP, KEEP, UNDECIDED = pm.DROP, pm.KEEP, pm.UNDECIDED
MAX_K, MAX_LEN = 15, 4096

_FOLD = bytes(b - 0x20 if 0x61 <= b <= 0x7A else b for b in range(256))


def fold(x):
    return bytes(x).translate(_FOLD)


def piece_bounds(n, k):
    q, r = divmod(n, k + 1)
    return [i * q + min(i, r) for i in range(k + 2)]


class Approx:
    """pattern: bytes; k: its budget (0: a plain pattern); nocase: the comparison folds ASCII case"""

    def __init__(self, pattern, k=0, nocase=False):
        self.bytes, self.k, self.nocase = bytes(pattern), int(k), bool(nocase)
        self.n = len(self.bytes)
        self.cmp = np.frombuffer(fold(self.bytes) if nocase else self.bytes, dtype=np.uint8)
        self.bounds = piece_bounds(self.n, self.k)

    def mismatches(self, window):
        """per-position mismatch flags against n bytes of text"""
        w = np.frombuffer(fold(window) if self.nocase else bytes(window), dtype=np.uint8)
        return w != self.cmp


def as_approx(pats):
    return [p if isinstance(p, Approx) else Approx(*p) if isinstance(p, tuple) else Approx(p) for p in pats]


def brute_force(pats, texts):
    """every (pattern, start offset in the concatenation, distance) with distance <= k, each text alone"""
    pats = as_approx(pats)
    out, base = set(), 0
    for t in texts:
        t = bytes(t)
        for x, p in enumerate(pats):
            tt = np.frombuffer(fold(t) if p.nocase else t, dtype=np.uint8)
            if p.n == 0 or tt.size < p.n:
                continue
            win = np.lib.stride_tricks.sliding_window_view(tt, p.n)
            for c in range(0, win.shape[0], 1024):           # (in slices: a long pattern's comparison is large)
                d = (win[c:c + 1024] != p.cmp).sum(axis=1)
                for s in np.flatnonzero(d <= p.k).tolist():
                    out.add((x, base + c + s, int(d[s])))
        base += len(t)
    return out


class ApproxModel:
    """pats: bytes, (bytes, k) or (bytes, k, nocase) or Approx, in the order they are added.  Pattern x with budget
    k occupies k + 1 consecutive pattern indices of the automaton, its pieces.  The walk is that of the automaton
    of the pieces, added as plain patterns (not through add_approx)."""

    def __init__(self, pats):
        self.pats = as_approx(pats)
        self.owner, self.piece, self.first = [], [], []
        a = Automaton()
        for x, p in enumerate(self.pats):
            self.first.append(len(self.owner))
            for j in range(p.k + 1):
                self.owner.append(x)
                self.piece.append(j)
                a.add(p.bytes[p.bounds[j]:p.bounds[j + 1]], x, nocase=p.nocase)
        a.compile()
        self.a = a
        self.num_patterns = len(self.owner)
        self.num_states = a.num_states
        self.next = np.abs(a.reference_table()[:, 0, :]).astype(np.int64)
        lists = [a.state_matches(s) for s in range(a.num_states)]
        self.list_len = np.array([len(x) for x in lists], dtype=np.int64)
        self.list = np.full((a.num_states, max(1, int(self.list_len.max()) if lists else 1)), -1, dtype=np.int64)
        for s, x in enumerate(lists):
            self.list[s, :len(x)] = x

    def span(self, p, o):
        """(pattern x, first offset of its span) of entry (p, o)"""
        w, j = self.pats[self.owner[p]], self.piece[p]
        return self.owner[p], o - (w.bounds[j + 1] - w.bounds[j]) + 1 - w.bounds[j]

    def _verdict(self, p, o, t0, tend, known, full, lo):
        """(verdict, distance); full: the bytes given, before ++ text, the first of them at offset lo"""
        if not 0 <= p < self.num_patterns:
            return DROP, 0
        w, j = self.pats[self.owner[p]], self.piece[p]
        if w.n == 0:
            return DROP, 0
        if w.k == 0:
            return KEEP, 0
        _, s = self.span(p, o)
        if s < t0 or (known and s + w.n > tend):
            return DROP, 0
        if s < lo or s + w.n > lo + len(full):
            return UNDECIDED, 0
        mis = w.mismatches(full[s - lo:s - lo + w.n])
        m = [int(mis[w.bounds[i]:w.bounds[i + 1]].sum()) for i in range(w.k + 1)]
        ok = m[j] == 0 and all(x > 0 for x in m[:j]) and sum(m) <= w.k
        return (KEEP, sum(m)) if ok else (DROP, 0)

    def entries(self, p, o, text, origin=0, before=b"", starts=(), lead_begin=0, open_end=None):
        p, o = np.asarray(p, dtype=np.int64), np.asarray(o, dtype=np.int64)
        t0, tend, known = pm.bounds(o, starts, lead_begin, origin + len(text), open_end)
        full, lo = bytes(before) + bytes(pm.as_u8(text)), origin - len(before)
        vd = [self._verdict(int(p[i]), int(o[i]), int(t0[i]), int(tend[i]), bool(known[i]), full, lo) for i in range(p.size)]
        v = np.array([x[0] for x in vd], dtype=np.int64)
        d = np.array([x[1] for x in vd], dtype=np.int64)
        keep = v == KEEP
        return p[keep].astype(np.int32), o[keep], d[keep].astype(np.int32), int((v == UNDECIDED).sum())

    def filter(self, cells, offs, report, text, origin=0, before=b"", starts=(), lead_begin=0, open_end=None):
        """(patterns int32, offsets int64, distances int32, undecided) the pass writes for the cells, whatever they
        hold"""
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        if report != STATE:
            return self.entries(cells, offs, text, origin, before, starts, lead_begin, open_end)
        ok = (cells >= 0) & (cells < self.num_states)
        n = np.where(ok, self.list_len[np.where(ok, cells, 0)], 0)
        rec = np.repeat(np.arange(cells.size), n)
        j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
        return self.entries(self.list[cells[rec], j], offs[rec], text, origin, before, starts, lead_begin, open_end)

    def walk(self, text, init_state=0):
        """(states, offsets, final state): one cell per offset whose state has a match list"""
        s, states, offs = int(init_state), [], []
        for i, c in enumerate(pm.as_u8(text).tolist()):
            s = int(self.next[s, c])
            if self.list_len[s]:
                states.append(s)
                offs.append(i)
        return np.array(states, dtype=np.int64), np.array(offs, dtype=np.int64), s

    def all_entries(self, text, origin=0):
        """(patterns, offsets) of every list entry of the walk over text, in record order"""
        states, offs, _ = self.walk(text)
        n = self.list_len[states]
        rec = np.repeat(np.arange(states.size), n)
        j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
        return self.list[states[rec], j], offs[rec] + origin

    def matches(self, texts):
        """{(pattern x, start in the concatenation, distance)} by the rule, each text alone"""
        out, base = set(), 0
        for t in texts:
            t = bytes(pm.as_u8(t))
            p, o = self.all_entries(t)
            kp, ko, kd, und = self.entries(p, o, t, open_end=len(t))
            assert und == 0
            for pp, oo, dd in zip(kp.tolist(), ko.tolist(), kd.tolist()):
                x, s = self.span(pp, oo)
                key = (x, base + s, dd)
                assert key not in out, "an occurrence is reported once"
                out.add(key)
            base += len(t)
        return out
