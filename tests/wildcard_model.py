"""Wildcard patterns in Python (test infrastructure only, not a conftest): the anchor choice of
acm_automaton_add_wildcard, the rule of acm_wildcard_matches_async and the extended signature grammar of
acm_automaton_add_signature_ex, written from include/acmatch.h.

A wildcard pattern is n positions, each a set of byte values.  Its anchor is the longest run of one-byte
positions, the leftmost among equal runs: L bytes, pre positions in front, post behind.  Entry (p, o) -- the
anchor of p ends at o -- has a = o - L + 1 and the span [a - pre, o + post]; in the text [T0, Tend) of its record:
  1. no context: kept            2. the span leaves [T0, Tend): dropped
  3. the span leaves the bytes given: undecided (dropped and counted)
  4. kept iff every context byte is in its set

  brute_force     every position tested at every offset of every text, without an automaton
  regex_force     the same statement for Python's re: one character class per position, a lookahead per offset
  WildcardModel   the rule over (pattern, offset) entries in numpy/Python, whatever the cells hold, and the walk
  parse_body_ex   the extended grammar: HH, H?, ?H, ??, (HH|..), !(HH|..), *, {n}, {n-m}, {-m}, {n-}
  span_sequences  sequences over wildcard parts found by brute force on the parts' full spans
"""
import re

import numpy as np

from gpu_pattern_matching_amd import Automaton

import position_model as pm
from sequence_model import BodyError, MAX_PARTS, UNB

STATE, HEAD = 1, 0
DROP, KEEP, UNDECIDED = pm.DROP, pm.KEEP, pm.UNDECIDED
FULL = frozenset(range(256))
MAX_POSITIONS = 4096
HEX = b"0123456789abcdefABCDEF"


def as_set(position):
    if isinstance(position, int):
        return frozenset((position,))
    return frozenset(int(b) for b in position)


def anchor_of(positions):
    """(at, L): the longest run of one-byte sets, the leftmost among equal runs; L 0: there is none"""
    at = L = run = 0
    for i, s in enumerate(positions):
        run = run + 1 if len(s) == 1 else 0
        if run > L:
            at, L = i + 1 - run, run
    return at, L


def fold(b):
    return b - 0x20 if 0x61 <= b <= 0x7A else b


class Pattern:
    """positions: a list of ints, bytes or iterables of ints; nocase: the anchor ignores ASCII case"""

    def __init__(self, positions, nocase=False):
        self.positions = [as_set(p) for p in positions]
        self.nocase = nocase
        self.at, self.L = anchor_of(self.positions)
        assert self.L > 0
        self.pre, self.post = self.at, len(self.positions) - self.at - self.L
        self.anchor = bytes(min(s) for s in self.positions[self.at:self.at + self.L])

    def holds(self, t, k):
        """does the pattern match with its first position at t[k]?  (t: bytes, the span inside it)"""
        for i, s in enumerate(self.positions):
            b = t[k + i]
            if self.nocase and self.at <= i < self.at + self.L:
                if fold(b) != fold(min(s)):
                    return False
            elif b not in s:
                return False
        return True


def as_patterns(pats):
    return [p if isinstance(p, Pattern) else Pattern(*p) if isinstance(p, tuple) else Pattern(p) for p in pats]


def brute_force(pats, texts):
    """every (offset of the ANCHOR's end in the concatenation, pattern index) pair, each text alone"""
    pats = as_patterns(pats)
    out, base = set(), 0
    for t in texts:
        t = bytes(t)
        for i, p in enumerate(pats):
            n = len(p.positions)
            for k in range(len(t) - n + 1):
                if p.holds(t, k):
                    out.add((base + k + p.at + p.L - 1, i))
        base += len(t)
    return out


def regex_force(positions, t):
    """first offsets at which the positions match in t: a lookahead of one character class per position"""
    rx = b"".join(b"[" + b"".join(b"\\x%02x" % b for b in sorted(as_set(s))) + b"]" for s in positions)
    return [m.start() for m in re.finditer(b"(?s)(?=" + rx + b")", bytes(t))]


class WildcardModel:
    """pats: a list of position lists, (positions, nocase) pairs or Patterns, in the order they are added.  The
    walk is that of the automaton of the anchors, added as plain patterns (not through add_wildcard)."""

    def __init__(self, pats):
        self.pats = as_patterns(pats)
        n = len(self.pats)
        self.len = np.array([p.L for p in self.pats], dtype=np.int64)
        self.pre = np.array([p.pre for p in self.pats], dtype=np.int64)
        self.post = np.array([p.post for p in self.pats], dtype=np.int64)
        a = Automaton()
        for i, p in enumerate(self.pats):
            a.add(p.anchor, i, nocase=p.nocase)
        a.compile()
        self.a = a
        self.num_states = a.num_states
        self.next = np.abs(a.reference_table()[:, 0, :]).astype(np.int64)
        lists = [a.state_matches(s) for s in range(a.num_states)]
        self.list_len = np.array([len(x) for x in lists], dtype=np.int64)
        self.list = np.full((a.num_states, max(1, int(self.list_len.max()) if n else 1)), -1, dtype=np.int64)
        for s, x in enumerate(lists):
            self.list[s, :len(x)] = x

    def verdict(self, p, o, t0, tend, known, text, origin, before):
        return self._verdict(p, o, t0, tend, known, bytes(before) + bytes(pm.as_u8(text)), origin - len(before))

    def _verdict(self, p, o, t0, tend, known, full, lo):
        """full: the bytes given, before ++ text, the first of them at offset lo"""
        if not 0 <= p < len(self.pats):
            return DROP
        w = self.pats[p]
        if w.pre == 0 and w.post == 0:
            return KEEP
        first, last = o - w.L + 1 - w.pre, o + w.post
        if first < t0 or (known and last >= tend):
            return DROP
        if first < lo or last >= lo + len(full):
            return UNDECIDED
        ctx = [(first + i, w.positions[i]) for i in range(w.pre)] + \
              [(o + 1 + i, w.positions[w.at + w.L + i]) for i in range(w.post)]
        return KEEP if all(full[q - lo] in s for q, s in ctx) else DROP

    def entries(self, p, o, group, all_patterns, text, origin=0, before=b"", starts=(), lead_begin=0, open_end=None):
        p, o = np.asarray(p, dtype=np.int64), np.asarray(o, dtype=np.int64)
        t0, tend, known = pm.bounds(o, starts, lead_begin, origin + len(text), open_end)
        full, lo = bytes(before) + bytes(pm.as_u8(text)), origin - len(before)
        v = np.array([self._verdict(int(p[i]), int(o[i]), int(t0[i]), int(tend[i]), bool(known[i]), full, lo)
                      for i in range(p.size)], dtype=np.int64)
        keep, und = pm.Windows.select(v, np.asarray(group), all_patterns)
        return p[keep].astype(np.int32), o[keep], und

    def filter(self, cells, offs, report, all_patterns, text, origin=0, before=b"", starts=(), lead_begin=0, open_end=None):
        """(patterns int32, offsets int64, undecided) the pass writes for the cells, whatever they hold"""
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        if report != STATE:
            assert all_patterns
            return self.entries(cells, offs, np.arange(cells.size), True, text, origin, before, starts, lead_begin, open_end)
        ok = (cells >= 0) & (cells < self.num_states)
        n = np.where(ok, self.list_len[np.where(ok, cells, 0)], 0)
        rec = np.repeat(np.arange(cells.size), n)
        j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
        return self.entries(self.list[cells[rec], j], offs[rec], rec, all_patterns, text, origin, before, starts, lead_begin,
                            open_end)

    def walk(self, text, init_state=0):
        """(states, offsets, final state): one cell per offset whose state has a match list"""
        s, states, offs = int(init_state), [], []
        for i, c in enumerate(pm.as_u8(text).tolist()):
            s = int(self.next[s, c])
            if self.list_len[s]:
                states.append(s)
                offs.append(i)
        return np.array(states, dtype=np.int64), np.array(offs, dtype=np.int64), s

    def records(self, texts, all_patterns=False):
        """(offsets uint32, patterns int32, final state, undecided) of scan_wildcards(texts=texts)"""
        os_, ps, last, base = [], [], 0, 0
        for t in texts:
            t = bytes(pm.as_u8(t))
            states, offs, last = self.walk(t)
            p, o, und = self.filter(states, offs, STATE, all_patterns, t, open_end=len(t))
            assert und == 0
            ps += p.tolist()
            os_ += (o + base).tolist()
            base += len(t)
        return np.array(os_, dtype=np.uint32), np.array(ps, dtype=np.int32), last, 0


# ---- the extended grammar

def _hex2(body, k):
    return int(body[k:k + 2], 16) if k + 1 < len(body) and body[k] in HEX and body[k + 1] in HEX else None


def _number(body, k):
    """(value, index behind the digits) or None"""
    e = k
    while e < len(body) and body[e:e + 1].isdigit():
        e += 1
    if e == k or int(body[k:e]) >= UNB:
        return None
    return int(body[k:e]), e


def _braces(body, k):
    """(lo, hi or None, index behind '}') of the token at body[k] == '{', or None"""
    k += 1
    lo, hi = 0, None
    if body[k:k + 1] == b"-":
        r = _number(body, k + 1)
        if not r:
            return None
        hi, k = r
    else:
        r = _number(body, k)
        if not r:
            return None
        lo, k = r
        if body[k:k + 1] == b"-":
            k += 1
            if body[k:k + 1] != b"}":
                r = _number(body, k)
                if not r:
                    return None
                hi, k = r
        else:
            hi = lo
    return (lo, hi, k + 1) if body[k:k + 1] == b"}" else None


def parse_body_ex(body):
    """(parts: a list of lists of frozensets, gaps: a list of (lo, hi or None)) of an extended body; BodyError
    names the column (from 1) of the first byte that is wrong (a part without an exact byte: where it begins)"""
    body = body.encode() if isinstance(body, str) else bytes(body)
    parts, gaps, cur, cur_at, gap, k = [], [], [], 0, None, 0

    def close_part():
        if not any(len(s) == 1 for s in cur):
            raise BodyError(cur_at + 1)
        parts.append(list(cur))

    while k < len(body):
        at, c = k, body[k:k + 1]
        s = None
        if body[k] in HEX:
            if _hex2(body, k) is not None:
                s = frozenset((_hex2(body, k),))
            elif body[k + 1:k + 2] == b"?":
                s = frozenset(int(c, 16) << 4 | x for x in range(16))
            else:
                raise BodyError(at + 1)
            k += 2
        elif c == b"?":
            n = body[k + 1:k + 2]
            if n == b"?":
                s = FULL
            elif n and n in HEX:
                s = frozenset(x << 4 | int(n, 16) for x in range(16))
            else:
                raise BodyError(at + 1)
            k += 2
        elif c in (b"(", b"!"):
            if c == b"!" and body[k + 1:k + 2] != b"(":
                raise BodyError(at + 1)
            k += 2 if c == b"!" else 1
            listed = set()
            while True:
                b = _hex2(body, k)
                if b is None:
                    raise BodyError(k + 1)
                listed.add(b)
                k += 2
                if body[k:k + 1] == b")":
                    break
                if body[k:k + 1] != b"|":
                    raise BodyError(k + 1)
                k += 1
            k += 1
            s = frozenset(listed) if c == b"(" else FULL - listed
            if not s:
                raise BodyError(at + 1)
        elif c == b"*":
            lo, hi, k = 0, None, k + 1
        elif c == b"{":
            r = _braces(body, k)
            if not r:
                raise BodyError(at + 1)
            lo, hi, k = r
        else:
            raise BodyError(at + 1)
        if s is not None:
            if not parts and not cur and s == FULL:
                raise BodyError(at + 1)
            if len(cur) >= MAX_POSITIONS:
                raise BodyError(at + 1)
            if gap is not None:
                gaps.append(gap)
                gap = None
            if not cur:
                cur_at = at
            cur.append(s)
            continue
        if gap is None:
            if not cur:
                raise BodyError(at + 1)
            close_part()
            cur = []
            gap = (0, 0)
        gap = (gap[0] + lo, None if gap[1] is None or hi is None else gap[1] + hi)
        if max(gap[0], gap[1] or 0) >= UNB:
            raise BodyError(at + 1)
    if gap is not None or not cur or cur[-1] == FULL:
        raise BodyError(len(body) + 1)
    close_part()
    if len(parts) > MAX_PARTS:
        raise BodyError(len(body) + 1)
    return parts, gaps


def span_sequences(pats, seqs, texts, windows=None):
    """every (offset the match ENDS at in the concatenation, sequence index) pair: each part found by brute force
    with its full span, then a chain search with the gaps counted between spans.  pats as WildcardModel takes.
    windows: {pattern: (lo, hi or None, from_end)}, counted from the pattern's first position."""
    pats = as_patterns(pats)
    windows = windows or {}
    out, base = set(), 0
    for t in texts:
        t = bytes(t)
        for q, s in enumerate(seqs):
            parts, gaps = s[0], s[1]
            occ = []
            for pi in parts:
                w = pats[pi]
                n = len(w.positions)
                lo, hi, fe = windows.get(pi, (0, None, False))
                occ.append([(k, k + n - 1) for k in range(len(t) - n + 1) if w.holds(t, k) and
                            lo <= (len(t) - k if fe else k) and (hi is None or (len(t) - k if fe else k) <= hi)])
            alive = {e for _, e in occ[0]}
            for j in range(1, len(parts)):
                glo, ghi = gaps[j - 1]
                alive = {e for a, e in occ[j]
                         if any(glo <= a - pe - 1 and (ghi is None or a - pe - 1 <= ghi) for pe in alive)}
            out |= {(base + e, q) for e in alive}
        base += len(t)
    return out
