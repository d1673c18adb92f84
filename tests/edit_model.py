"""Edit patterns in Python (test infrastructure only, not a conftest): the rule of acm_edit_matches_async, written
from include/acmatch.h, over the pieces' automaton as approx_model.ApproxModel builds it.

  sellers         the whole Sellers matrix of a pattern against a text: row n holds D(e) for every end e
  brute_force     D(e) of every edit pattern at every end of every text, without pieces or an automaton
  EditModel       the rule over (pattern, offset) entries, whatever the cells hold: the unique records in
                  (offset, pattern) order, the undecided entries and the candidates
  check           the three properties of include/acmatch.h -- sound, unique, complete -- of a set of records
                  against brute_force

A pattern of a set is bytes (plain), (bytes, k) or (bytes, k, nocase) (Hamming, as approx_model takes them) or
Edit(bytes, k, nocase)."""
import numpy as np

import approx_model as am
import position_model as pm

STATE, HEAD = am.STATE, am.HEAD
DROP, KEEP, UNDECIDED = am.DROP, am.KEEP, am.UNDECIDED
MAX_K = 4


class Edit(am.Approx):
    """an edit pattern: distance is the unit-cost edit distance"""
    edit = True


def is_edit(p):
    return getattr(p, "edit", False)


def sellers(A, T, nocase=False, anchored=False, limit=None):
    """The (n + 1) x (m + 1) matrix C, C[i][e] = the least edit distance of A[:i] to a span of T that ends at e
    (anchored: to T[:e]).  Row n is D.  limit: None, or stop at the first row that is all > limit and return
    None (the rows behind it are too)."""
    a = np.frombuffer(am.fold(A) if nocase else bytes(A), dtype=np.uint8)
    t = np.frombuffer(am.fold(T) if nocase else bytes(T), dtype=np.uint8)
    n, m = a.size, t.size
    idx = np.arange(m + 1, dtype=np.int64)
    C = np.empty((n + 1, m + 1), dtype=np.int64)
    C[0] = idx if anchored else 0
    for i in range(1, n + 1):
        prev = C[i - 1]
        tmp = np.empty(m + 1, dtype=np.int64)
        tmp[0] = i
        tmp[1:] = np.minimum(prev[:-1] + (t != a[i - 1]), prev[1:] + 1)
        C[i] = np.minimum.accumulate(tmp - idx) + idx        # C[i][e] = min over e' <= e of tmp[e'] + (e - e')
        if limit is not None and C[i].min() > limit:
            return None
    return C


def shortest(A, T, d, nocase=False):
    """the smallest l with ed(A, T[len(T) - l:]) == d, or None"""
    row = sellers(bytes(A)[::-1], bytes(T)[::-1], nocase, anchored=True)[-1]
    hit = np.flatnonzero(row == d)
    return int(hit[0]) if hit.size else None


def brute_force(pats, texts):
    """{x: D} for every edit pattern x of pats: D[e] = D(e) at end e (counted in the concatenation) of the text e
    lies in, each text alone; -1 where e is no end of a text (e == its T0).  And the text bounds [(T0, Tend)]."""
    pats = as_pats(pats)
    total = sum(len(t) for t in texts)
    out = {x: np.full(total + 1, -1, dtype=np.int64) for x, p in enumerate(pats) if is_edit(p)}
    spans, base = [], 0
    for t in texts:
        t = bytes(pm.as_u8(t))
        spans.append((base, base + len(t)))
        for x in out:
            p = pats[x]
            out[x][base + 1:base + len(t) + 1] = sellers(p.bytes, t, p.nocase)[-1][1:]
        base += len(t)
    return out, spans


def as_pats(pats):
    return [p if isinstance(p, am.Approx) else am.Approx(*p) if isinstance(p, tuple) else am.Approx(p) for p in pats]


class EditModel(am.ApproxModel):
    def __init__(self, pats):
        super().__init__(as_pats(pats))

    def _candidate(self, p, o, t0, tend, known, full, lo):
        """(verdict, (pattern, offset, distance, length))"""
        if not 0 <= p < self.num_patterns:
            return DROP, None
        x, j = self.owner[p], self.piece[p]
        w = self.pats[x]
        L = w.bounds[j + 1] - w.bounds[j]
        if L == 0:
            return DROP, None
        hi = lo + len(full)
        if w.k == 0:
            c = (p, o, 0, L)
        elif not is_edit(w):
            v, d = self._verdict(p, o, t0, tend, known, full, lo)
            if v != KEEP:
                return v, None
            c = (self.first[x], o + w.n - w.bounds[j + 1], d, w.n)
        else:
            k, n = w.k, w.n
            a = o - L + 1
            if a < t0 or (known and o + 1 > tend):
                return DROP, None
            s0 = a - w.bounds[j]
            e0 = s0 + n
            if not known and e0 + k > hi:
                return UNDECIDED, None
            wlo, whi = max(t0, s0 - 2 * k), (min(tend, e0 + k) if known else e0 + k)
            if wlo < lo or whi > hi:
                return UNDECIDED, None
            C = sellers(w.bytes, full[wlo - lo:whi - lo], w.nocase, limit=k)
            if C is None:
                return DROP, None
            ends = [(min(int(C[n][e - wlo]), k + 1), abs(e - e0), e) for e in range(e0 - k, e0 + k + 1) if t0 < e <= whi and e >= wlo]
            if not ends or min(ends)[0] > k:
                return DROP, None
            d, _, e = min(ends)
            ln = shortest(w.bytes, full[max(t0, e - n - k) - lo:e - lo], d, w.nocase)
            assert ln is not None
            c = (self.first[x], e - 1, d, ln)
        return (KEEP, c) if lo <= c[1] < hi else (DROP, None)

    def records(self, cells, offs, report, text, origin=0, before=b"", starts=(), lead_begin=0, open_end=None):
        """(patterns, offsets, distances, lengths: int32 arrays in (offset, pattern) order, unique; undecided;
        candidates) the pass writes for the cells, whatever they hold"""
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        if report == STATE:
            ok = (cells >= 0) & (cells < self.num_states)
            n = np.where(ok, self.list_len[np.where(ok, cells, 0)], 0)
            rec = np.repeat(np.arange(cells.size), n)
            j = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
            p, o = self.list[cells[rec], j], offs[rec]
        else:
            p, o = cells, offs
        t0, tend, known = pm.bounds(o, starts, lead_begin, origin + len(text), open_end)
        full, lo = bytes(before) + bytes(pm.as_u8(text)), origin - len(before)
        memo, cands, und = {}, [], 0
        for i in range(p.size):
            key = (int(p[i]), int(o[i]), int(t0[i]), int(tend[i]), bool(known[i]))
            if key not in memo:
                memo[key] = self._candidate(*key, full, lo)
            v, c = memo[key]
            und += v == UNDECIDED
            if v == KEEP:
                cands.append(c)
        uniq = sorted(set(cands), key=lambda c: (c[1], c[0]))
        assert len({(c[0], c[1]) for c in uniq}) == len(uniq), "two candidates of one (pattern, end) differ"
        cols = [np.array([c[i] for c in uniq], dtype=np.int64).astype(np.int32) for i in (0, 1, 2, 3)]
        return cols[0], cols[1], cols[2], cols[3], int(und), len(cands)

    def scan(self, texts):
        """the records of whole texts, each matched alone, offsets in the concatenation: as Matcher.scan_edit"""
        cells, offs, starts, base = [], [], [], 0
        for t in texts:
            t = pm.as_u8(t)
            p, o = self.all_entries(t, base)
            cells.append(p)
            offs.append(o)
            starts.append(base)
            base += t.size
        text = b"".join(bytes(pm.as_u8(t)) for t in texts)
        cat = (lambda x: np.concatenate(x) if x else np.zeros(0, dtype=np.int64))
        return self.records(cat(cells), cat(offs), HEAD, text, starts=starts, open_end=len(text))


def check(pats, texts, records):
    """the three properties of the records (pattern x, end offset, distance, length) of the edit patterns of pats
    over texts (each alone, offsets in the concatenation) against brute_force; x indexes pats.  Returns the number
    of ends with D(e) <= k."""
    pats = as_pats(pats)
    D, spans = brute_force(pats, texts)
    text = b"".join(bytes(pm.as_u8(t)) for t in texts)
    recs = [r for r in records if r[0] in D]
    assert len({(x, o) for x, o, _, _ in recs}) == len(recs), "unique: a (pattern, offset) appears twice"
    starts = np.array([s for s, _ in spans], dtype=np.int64)
    by = {x: {} for x in D}
    for x, o, d, ln in recs:                                     # sound
        p, e = pats[x], o + 1
        assert 0 < e <= len(text) and d == D[x][e] <= p.k, (x, o, d, int(D[x][e]))
        t0 = int(starts[np.searchsorted(starts, o, side="right") - 1])
        assert e - ln >= t0 and shortest(p.bytes, text[max(t0, e - p.n - p.k):e], d, p.nocase) == ln, (x, o, d, ln)
        by[x][e] = (d, ln)
    near = 0
    for x, row in D.items():                                     # complete
        p = pats[x]
        for e in np.flatnonzero((row >= 0) & (row <= p.k)).tolist():
            near += 1
            if row[e] == 0:
                assert by[x].get(e) == (0, p.n), "complete: the exact occurrence of %d at %d is %s" % (x, e, by[x].get(e))
            assert any(by[x].get(f, (p.k + 1,))[0] <= row[e] for f in range(e - 2 * p.k, e + 2 * p.k + 1)), \
                "complete: nothing near end %d of pattern %d, distance %d" % (e, x, row[e])
    return near


# ---- planted occurrences ----

def variants(A, k):
    """near-copies of the edit pattern A: [(name, bytes)]; '#' is a byte no pattern holds"""
    A = bytes(A)
    b = am.piece_bounds(len(A), k)
    X = b"#"
    out = [("exact", A), ("front deleted", A[k:]), ("front inserted", A[:1] + X * k + A[1:]), ("end deleted", A[:-k]),
           ("end inserted", A[:-1] + X * k + A[-1:])]
    for j in sorted({0, k // 2, k}):
        # piece j is the only exact one: a deletion in every piece in front of it, an insertion in every one behind
        v = bytearray()
        for i in range(k + 1):
            piece = A[b[i]:b[i + 1]]
            v += piece[1:] if i < j else piece if i == j else piece[:1] + X + piece[1:]
        out.append(("only piece %d" % j, bytes(v)))
        v = bytearray(A)                         # an error on each side of the piece's borders
        if b[j] > 0:
            v[b[j] - 1] = X[0]
        if b[j + 1] < len(A) and (k >= 2 or b[j] == 0):
            v[b[j + 1]] = X[0]
        out.append(("borders of %d" % j, bytes(v)))
    v = bytearray(A)                             # k + 1 errors: no piece is exact
    for i in range(k + 1):
        v[b[i]] = X[0]
    out.append(("over budget", bytes(v)))
    return out


def planted(pats, seed=3, letters=b"abc", gap=(3, 9), lead=5):
    """random letters with every variant of every edit pattern of pats planted; returns (text, [(x, name, at, bytes)])"""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(letters, dtype=np.uint8)
    parts, where, at = [bytes(rng.choice(al, size=lead))], [], lead
    for x, p in enumerate(as_pats(pats)):
        if not is_edit(p):
            continue
        for name, v in variants(p.bytes, p.k):
            where.append((x, name, at, v))
            noise = bytes(rng.choice(al, size=int(rng.integers(*gap))))
            parts += [v, noise]
            at += len(v) + len(noise)
    return b"".join(parts), where
