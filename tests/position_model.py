"""Position constraints per pattern in Python (test infrastructure only, not a conftest): the rule of
acm_position_matches_async, written from include/acmatch.h.

Pattern p of length L >= 1 that ends at offset o starts at a = o - L + 1; its text occupies [T0, Tend).
With the window (lo, hi, from_end) it is kept iff lo <= a - T0 <= hi, or with from_end iff
lo <= Tend - a <= hi; hi None: no upper bound.  (0, None, False) is no constraint: always kept.  An
end-anchored entry of a text whose end is unknown is undecided: dropped and counted.  Length 0: never kept.

The model works on entries (pattern, offset, group): a group is a record of a STATE plane (its entries the
state's match list, from Automaton.state_matches) or a run of equal offsets of a HEAD plane.  The all form
keeps every kept entry; the first form the first kept entry of each group, and counts only the undecided
entries in front of it.  brute_force restates the rule with bytes.find over each text, without an automaton.
Windows is the rule without an automaton, for entries that come from elsewhere; PositionModel adds the walk.
"""
import numpy as np

from gpu_pattern_matching_amd import Automaton

STATE, HEAD = 1, 0
UNB = 0x7FFFFFFF
DROP, KEEP, UNDECIDED = 0, 1, 2
WORD = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")


def as_u8(text):
    return np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) \
        else np.ascontiguousarray(text, dtype=np.uint8)


def build(pats, windows, **kw):
    """a compiled Automaton of pats (bytes, or (bytes, nocase) pairs) with windows {index: (lo, hi, from_end)}"""
    a = Automaton(**kw)
    for i, p in enumerate(pats):
        if isinstance(p, tuple):
            a.add(p[0], i, nocase=p[1])
        else:
            a.add(p, i)
    a.compile()
    for i, (lo, hi, fe) in windows.items():
        a.set_position(i, lo, hi, fe)
    return a


def bounds(offs, starts, lead_begin, text_end, open_end):
    """(T0, Tend, end known) of the text each offset lies in.  open_end None: unknown."""
    o = np.asarray(offs, dtype=np.int64)
    st = np.asarray(starts, dtype=np.int64)
    S = st.size
    if S == 0:
        ub = np.zeros(o.size, dtype=np.int64)
        t0 = np.full(o.size, lead_begin, dtype=np.int64)
        closed = np.zeros(o.size, dtype=bool)
        nxt = np.zeros(o.size, dtype=np.int64)
    else:
        ub = np.searchsorted(st, o, side="right")
        t0 = np.where(ub > 0, st[np.maximum(ub - 1, 0)], lead_begin)
        nxt = st[np.minimum(ub, S - 1)]
        closed = (ub < S) & (nxt <= text_end)
    tend = np.where(closed, nxt, 0 if open_end is None else open_end)
    known = closed | (open_end is not None)
    return t0.astype(np.int64), tend.astype(np.int64), known


class Windows:
    """the rule alone, for entries that come from elsewhere (an oracle's records): pats: bytes, or (bytes,
    nocase) pairs; windows: {index: (lo, hi or None, from_end)}"""

    def __init__(self, pats, windows):
        self.pats = [bytes(p[0] if isinstance(p, tuple) else p) for p in pats]
        self.nocase = [bool(p[1]) if isinstance(p, tuple) else False for p in pats]
        n = len(self.pats)
        self.lo = np.zeros(n, dtype=np.int64)
        self.hi = np.full(n, UNB, dtype=np.int64)
        self.fe = np.zeros(n, dtype=bool)
        for i, (lo, hi, fe) in windows.items():
            self.lo[i], self.hi[i], self.fe[i] = lo, UNB if hi is None else hi, fe
        self.len = np.array([len(p) for p in self.pats], dtype=np.int64)
        self.free = (self.lo == 0) & (self.hi == UNB) & ~self.fe

    def verdicts(self, p, o, t0, tend, known):
        """DROP / KEEP / UNDECIDED per entry (arrays)"""
        p = np.asarray(p, dtype=np.int64)
        valid = (p >= 0) & (p < len(self.pats))
        q = np.where(valid, p, 0)
        L, lo, hi, fe = self.len[q], self.lo[q], self.hi[q], self.fe[q]
        a = np.asarray(o, dtype=np.int64) - L + 1
        v = np.where(fe, tend - a, a - t0)
        ok = (v >= lo) & ((hi == UNB) | (v <= hi))
        out = np.where(self.free[q], KEEP, np.where(fe & ~known, UNDECIDED, np.where(ok, KEEP, DROP)))
        return np.where(valid & (L > 0), out, DROP)

    @staticmethod
    def select(v, group, all_patterns):
        """(mask of the entries written, undecided count) of verdicts v; group: non-decreasing group ids"""
        if all_patterns or v.size == 0:
            return v == KEEP, int((v == UNDECIDED).sum())
        kept = (v == KEEP).astype(np.int64)
        before = np.cumsum(kept) - kept                      # kept entries in front, all groups
        first = np.flatnonzero(np.r_[True, group[1:] != group[:-1]])
        base = np.repeat(before[first], np.diff(np.r_[first, v.size]))
        ahead = before - base                                # kept entries in front, this group
        return (v == KEEP) & (ahead == 0), int(((v == UNDECIDED) & (ahead == 0)).sum())

    def entries(self, p, o, all_patterns, starts=(), lead_begin=0, text_end=0, open_end=None):
        """(patterns int32, offsets int64, undecided) the pass writes for entries in pattern form: a run of
        equal offsets is a group"""
        p, o = np.asarray(p, dtype=np.int64), np.asarray(o, dtype=np.int64)
        group = np.cumsum(np.r_[0, o[1:] != o[:-1]]) if o.size else o
        t0, tend, known = bounds(o, starts, lead_begin, text_end, open_end)
        keep, und = self.select(self.verdicts(p, o, t0, tend, known), group, all_patterns)
        return p[keep].astype(np.int32), o[keep], und


class PositionModel(Windows):
    """pats: bytes, or (bytes, nocase) pairs (then the walk is the nocase automaton's, as the scan of a mixed
    automaton); windows: {index: (lo, hi or None, from_end)}"""

    def __init__(self, pats, windows):
        Windows.__init__(self, pats, windows)
        a = Automaton(nocase=any(self.nocase))
        for i, p in enumerate(self.pats):
            a.add(p, i)
        a.compile()
        self.a = a
        self.num_states = a.num_states
        self.next = np.abs(a.reference_table()[:, 0, :]).astype(np.int64)   # (final transitions are stored negated)
        lists = [a.state_matches(s) for s in range(a.num_states)]
        self.list_len = np.array([len(x) for x in lists], dtype=np.int64)
        self.list = np.full((a.num_states, max(1, int(self.list_len.max()))), -1, dtype=np.int64)
        for s, x in enumerate(lists):
            self.list[s, :len(x)] = x

    def filter(self, cells, offs, report, all_patterns, starts=(), lead_begin=0, text_end=0, open_end=None):
        """(patterns int32, offsets int64, undecided) the pass writes for the cells, whatever they hold"""
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        if report != STATE:
            return self.entries(cells, offs, all_patterns, starts, lead_begin, text_end, open_end)
        ok = (cells >= 0) & (cells < self.num_states)
        n = np.where(ok, self.list_len[np.where(ok, cells, 0)], 0)
        rec = np.repeat(np.arange(cells.size), n)
        j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
        p, o, group = self.list[cells[rec], j], offs[rec], rec
        t0, tend, known = bounds(o, starts, lead_begin, text_end, open_end)
        keep, und = self.select(self.verdicts(p, o, t0, tend, known), group, all_patterns)
        return p[keep].astype(np.int32), o[keep], und

    # ---- scanned text

    def walk(self, text, init_state=0):
        """(states, offsets, final state): one cell per offset whose state has a match list"""
        s, states, offs = int(init_state), [], []
        for i, c in enumerate(as_u8(text).tolist()):
            s = int(self.next[s, c])
            if self.list_len[s]:
                states.append(s)
                offs.append(i)
        return np.array(states, dtype=np.int64), np.array(offs, dtype=np.int64), s

    def then_keeps(self, then, p, o, t):
        """does entry p ending at offset o of the text t (scanned alone) pass the pass in between?"""
        pat = self.pats[p]
        L = len(pat)
        a = o - L + 1
        if L == 0:
            return False
        if then == "case":
            return self.nocase[p] or t[a:o + 1] == pat
        if then == "words":
            return (a == 0 or t[a - 1] not in WORD) and (o + 1 == len(t) or t[o + 1] not in WORD)
        return True

    def records(self, texts, all_patterns=False, then=None, open_end="end"):
        """(offsets uint32, patterns int32, final state, undecided) of scan_positions(texts=texts): every
        text walked alone from the root, offsets in the coordinates of the concatenation.  then: the
        entries go through that rule first and the pass sees them in HEAD form."""
        ps, os_, gs, starts, base, last = [], [], [], [], 0, 0
        for t in texts:
            t = bytes(as_u8(t))
            starts.append(base)
            states, offs, last = self.walk(t)
            for s, o in zip(states.tolist(), offs.tolist()):
                for p in self.list[s, :self.list_len[s]].tolist():
                    if self.then_keeps(then, p, o, t):
                        ps.append(p)
                        os_.append(o + base)
                        gs.append(o + base)
            base += len(t)
        p, o, g = (np.array(x, dtype=np.int64) for x in (ps, os_, gs))
        end = None if open_end is None else base if open_end == "end" else open_end
        t0, tend, known = bounds(o, starts, 0, base, end)
        keep, und = self.select(self.verdicts(p, o, t0, tend, known), g, all_patterns)
        return o[keep].astype(np.uint32), p[keep].astype(np.int32), last, und


def brute_force(pats, windows, texts):
    """every kept (end offset in the concatenation, pattern index) pair: each pattern found in each text with
    bytes.find and its window tested with the text's own bounds"""
    out, base = set(), 0
    for t in texts:
        t = bytes(t)
        for i, p in enumerate(pats):
            if not p:
                continue
            lo, hi, fe = windows.get(i, (0, None, False))
            k = t.find(p)
            while k >= 0:
                v = len(t) - k if fe else k
                if lo <= v and (hi is None or v <= hi):
                    out.add((base + k + len(p) - 1, i))
                k = t.find(p, k + 1)
        base += len(t)
    return out


def planes(pats, offs, cap, poison, trailer):
    """the two planes of cap cells a call must leave: [0] = count, the records that fit, the trailer at
    min(count + 1, cap - 1), the poison cell value everywhere else"""
    m = len(pats)
    stored = min(m, cap - 2)
    out = []
    for e in (pats, offs):
        p = np.full(cap, poison, dtype=np.int32)
        p[0] = m
        p[1:1 + stored] = np.asarray(e[:stored], dtype=np.int64).astype(np.int32)
        p[min(m + 1, cap - 1)] = trailer
        out.append(p)
    return out
