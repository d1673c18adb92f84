"""Logical signatures on bytes (test infrastructure only, not a conftest): what a database of
"expr;body0;body1;..." lines matches in a list of texts, computed with numpy from the text of the lines and
include/acmatch.h alone.  Nothing here knows of states, records, slots, planes or passes, and nothing is shared
with the C side; the body grammar is wildcard_model.parse_body_ex (group_model.parse_body_groups for a database with
groups) and the expression grammar rule_model.parse.

  part        a list of 256-entry truth tables, one per position.  It occurs at k iff table[i][T[k + i]] for every
              i, and k .. k + n - 1 lie in one text.  Candidates come from the first position and are thinned by
              the others (the AND over positions of a lookup on the shifted text).
  group       (at, strings, negated) on a part (acmatch.h, "Groups: alternatives of more than one byte"): after the
              truth tables have thinned the candidates k, the group holds iff the w bytes T[k + at : k + at + w]
              equal one of its strings (negated: none).  Raw bytes, whatever the case flag says.  The positions it
              covers carry the full set and a full set is no one-byte set: they are never part of the anchor, so
              the anchor, post, nocase and the windows are what they are without the group.
  nocase      acmatch.h: "ACM_PATTERN_NOCASE applies to the anchor only", the anchor being the longest run of
              one-byte positions, the leftmost among equal runs.  Those positions compare through fold(), every
              other position with the raw byte.  (wildcard_model.Pattern.holds folds the same positions.)
  window      (lo, hi or None, from_end) on a part: lo <= k - T0 <= hi, or lo <= Tend - k <= hi, k the part's FIRST
              position (acmatch.h: "count from the pattern's FIRST POSITION ... for both window kinds")
  join        sequence.hip's rule on full spans: level 0 is alive iff the part lies in its text; level j iff some
              alive level j - 1 occurrence ends in [max(a - 1 - hi, T0), a - 1 - lo].  One cumulative sum over the
              concatenation per level; T0 keeps every chain inside its text.
  rule        per (rule, text) from the counts; the trigger is the first hit in that text of the lowest-numbered
              operand that occurs there, and its offset the end of the last part's ANCHOR (Matcher.scan_rules)

Offsets are those of the concatenation of the texts, as Matcher.pack_segments lays them out.
"""
import numpy as np

import group_model as gm
import rule_model as rm
import wildcard_model as wm

FULL = np.ones(256, dtype=bool)
FOLD = np.arange(256)
FOLD[0x61:0x7B] -= 0x20


def split_line(line):
    """(expression, bodies) of "expr;body0;body1;..." """
    f = (line.decode() if isinstance(line, bytes) else line).strip().split(";")
    assert len(f) >= 2 and all(f)
    return f[0], f[1:]


def longest_exact_run(sets):
    """(at, n) of the longest run of one-byte sets, the leftmost among equal runs"""
    at = n = run = 0
    for i, s in enumerate(sets):
        run = run + 1 if len(s) == 1 else 0
        if run > n:
            at, n = i + 1 - run, run
    return at, n


class Part:
    """sets: one per position; groups: (at, strings, negated) tuples, at counted from the part's first position"""

    def __init__(self, sets, nocase, groups=()):
        self.sets = sets
        self.groups = [(int(at), [bytes(x) for x in strings], bool(neg)) for at, strings, neg in groups]
        self.n = len(sets)
        self.at, self.L = longest_exact_run(sets)
        self.post = self.n - self.at - self.L              # positions behind the anchor
        self.nocase = nocase

    def tables(self, nocase=True, contexts=True):
        out = []
        for i, s in enumerate(self.sets):
            anchor = self.at <= i < self.at + self.L
            t = np.zeros(256, dtype=bool)
            t[list(s)] = True
            if anchor and self.nocase and nocase:
                t = FOLD == FOLD[min(s)]
            elif not anchor and not contexts:
                t = FULL
            out.append(t)
        return out


class Database:
    """lines: logical signatures; nocase: one flag per SIGNATURE (body), in the order of the file; windows:
    {(signature, part): (lo, hi or None, from_end)}; groups: the bodies are in the grammar with multi-byte alternatives,
    (aabb|ccdd) and !(aabb|ccdd)"""

    def __init__(self, lines, nocase=None, windows=None, groups=False):
        self.sigs, self.rules = [], []                     # (parts, gaps); (operand signatures, tree)
        self.windows = dict(windows or {})
        for line in lines:
            expr, bodies = split_line(line)
            ops = []
            for b in bodies:
                q = len(self.sigs)
                parts, gaps, grps = gm.parse_body_groups(b) if groups else wm.parse_body_ex(b) + (None,)
                nc = bool(nocase[q]) if nocase is not None else False
                self.sigs.append(([Part(p, nc, grps[j] if grps else ()) for j, p in enumerate(parts)], gaps))
                ops.append(q)
            self.rules.append((ops, rm.parse(expr, len(ops))))


class Corpus:
    def __init__(self, texts):
        self.texts = [bytes(t) for t in texts]
        self.T = np.frombuffer(b"".join(self.texts), dtype=np.uint8)
        lens = np.array([len(t) for t in self.texts], dtype=np.int64)
        self.starts = np.cumsum(lens) - lens
        self.N = int(lens.sum())
        self.text_of = np.repeat(np.arange(len(self.texts)), lens)          # per byte
        self.t0 = np.repeat(self.starts, lens)
        self.tend = np.repeat(self.starts + lens, lens)


def group_holds(c, k, group):
    """per candidate k (the part's first position, its span inside the text): does the group hold there?"""
    at, strings, negated = group
    w = len(strings[0])
    under = c.T[(k + at)[:, None] + np.arange(w)[None, :]]                   # [candidate, byte of the group]
    one = np.zeros(k.size, dtype=bool)
    for s in strings:
        one |= (under == np.frombuffer(s, dtype=np.uint8)[None, :]).all(axis=1)
    return ~one if negated else one


def occurrences(c, tables, groups=()):
    """first positions k at which the tables hold, whose span lies in one text, and at which every group holds"""
    n = len(tables)
    if c.N < n:
        return np.zeros(0, dtype=np.int64)
    k = np.flatnonzero(tables[0][c.T[:c.N - n + 1]])
    for i in range(1, n):
        k = k[tables[i][c.T[k + i]]]
    k = k[k + n <= c.tend[k]]
    for g in groups:
        k = k[group_holds(c, k, g)]
    return k


def in_window(c, k, w):
    lo, hi, from_end = w
    rel = c.tend[k] - k if from_end else k - c.t0[k]
    return (rel >= lo) & (rel <= hi if hi is not None else True)


def sequences(db, texts, nocase=True, windows=True, contexts=True, counts=None, anchors_from=0, groups=True):
    """(ends, anchor_ends, signatures): every match of every signature, sorted by (anchor end, signature).  ends:
    where the match ends; anchor_ends: where its last part's anchor ends.  nocase / windows / contexts / groups
    False: the database as if it had none (a group then is as many ?? as it is wide).  counts: a dict that
    receives what each stage of a record chain sees:
    "anchors" (anchor occurrences inside a text), "parts" (with their contexts and groups), "windowed" (inside their
    windows), "matches".  anchors_from: only parts whose anchor begins at or behind this offset take part (a scan
    that begins there, with the bytes in front given as context, finds no other)."""
    c = texts if isinstance(texts, Corpus) else Corpus(texts)
    ends, aends, sigs = [], [], []
    tally = dict(anchors=0, parts=0, windowed=0, matches=0)
    for q, (parts, gaps) in enumerate(db.sigs):
        alive_ends = None
        for j, p in enumerate(parts):
            tabs = p.tables(nocase, contexts)
            if counts is not None:
                tally["anchors"] += occurrences(c, tabs[p.at:p.at + p.L]).size
            k = occurrences(c, tabs, p.groups if groups and contexts else ())
            k = k[k + p.at >= anchors_from]
            tally["parts"] += k.size
            if windows and (q, j) in db.windows:
                k = k[in_window(c, k, db.windows[q, j])]
            tally["windowed"] += k.size
            if j > 0:
                lo, hi = gaps[j - 1]
                cum = np.zeros(c.N + 1, dtype=np.int64)
                cum[alive_ends + 1] = 1
                cum = np.cumsum(cum)                                        # cum[x]: alive ends < x
                y = k - 1 - lo
                x = c.t0[k] if hi is None else np.maximum(k - 1 - hi, c.t0[k])
                ok = y >= x
                k = k[ok][cum[y[ok] + 1] - cum[x[ok]] > 0]
            alive_ends = k + p.n - 1
        if alive_ends.size:
            ends.append(alive_ends)
            aends.append(alive_ends - parts[-1].post)
            sigs.append(np.full(alive_ends.size, q, dtype=np.int64))
    ends, aends, sigs = (np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in (ends, aends, sigs))
    order = np.lexsort((sigs, aends))
    tally["matches"] = int(ends.size)
    if counts is not None:
        counts.update(tally)
    return ends[order], aends[order], sigs[order]


def group_decisions(db, texts, nocase=True):
    """(held, kept): the occurrences of the parts that have a group with their groups taken as ??, and how many
    of those the groups keep"""
    c = texts if isinstance(texts, Corpus) else Corpus(texts)
    held = kept = 0
    for parts, _ in db.sigs:
        for p in parts:
            if p.groups:
                tabs = p.tables(nocase)
                held += occurrences(c, tabs).size
                kept += occurrences(c, tabs, p.groups).size
    return held, kept


def count_matrix(db, c, aends, sigs):
    """[signature, text] occurrences"""
    m = np.zeros((len(db.sigs), len(c.texts)), dtype=np.int64)
    np.add.at(m, (sigs, c.text_of[aends]), 1)
    return m


def rules(db, texts, matches):
    """sorted (rule, text, offset) of every rule that holds in a text; matches: what sequences() returned"""
    c = texts if isinstance(texts, Corpus) else Corpus(texts)
    _, aends, sigs = matches
    m = count_matrix(db, c, aends, sigs)
    txt = c.text_of[aends]
    out = []
    for r, (ops, tree) in enumerate(db.rules):
        sub = m[ops]
        for t in np.flatnonzero(sub.sum(axis=0)).tolist():
            if rm.evaluate(tree, sub[:, t])[1]:
                q = ops[int(np.flatnonzero(sub[:, t])[0])]
                out.append((r, t, int(aends[(sigs == q) & (txt == t)].min())))
    return sorted(out)


def evaluated_pairs(db, texts, matches):
    """(rule, text) pairs with a hit: the programs the rule pass runs"""
    c = texts if isinstance(texts, Corpus) else Corpus(texts)
    m = count_matrix(db, c, matches[1], matches[2])
    return sum(int((m[ops].sum(axis=0) > 0).sum()) for ops, _ in db.rules)


# ---- seeded generators: bodies, expressions, databases and texts

LETTERS = b"aAbB1"          # both cases of two letters, so that nocase matters; nibbles 4?, 6?, ?1, ?2 split them


def _position(rng, alphabet, kinds):
    """(token, set) of one context position"""
    kind = kinds[int(rng.integers(len(kinds)))]
    a, b = (int(x) for x in rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=2, replace=False))
    if kind == "hi":
        return "%x?" % (a >> 4), frozenset((a & 0xF0) | x for x in range(16))
    if kind == "lo":
        return "?%x" % (a & 15), frozenset(x << 4 | (a & 15) for x in range(16))
    if kind == "alt":
        return "(%02x|%02x)" % (a, b), frozenset((a, b))
    if kind == "not":
        return "!(%02x)" % a, wm.FULL - {a}
    if kind == "not2":
        return "!(%02x|%02x)" % (a, b), wm.FULL - {a, b}
    return "??", wm.FULL


EDGE_KINDS = ("hi", "lo", "alt", "not", "not2")
INNER_KINDS = EDGE_KINDS + ("any", "any")


GROUP_WIDTHS = (2, 3, 4, 5, 8)
GROUP_PLACES = ("first", "last", "front", "behind", "adjacent", "exact")


def random_group(rng, alphabet, kind=None):
    """(token, strings, negated) of one group.  Widths 2, 3, 4, 5, 8 and one time in ten 31 or 32; 1 to 8 strings
    and one time in twelve 255 or 256 (of a width up to 5); a group of one string is negated, but for kind "exact":
    a non-negated group of one string, which the grammar turns into exact bytes.  The first strings are letters
    of the alphabet (so that text hits them by chance and nocase would matter), the others any bytes."""
    wide, many = rng.random() < 0.1, rng.random() < 1 / 12
    w = int(rng.integers(31, 33)) if wide else int(GROUP_WIDTHS[int(rng.integers(len(GROUP_WIDTHS)))])
    n = int(rng.integers(1, 9))
    if many and not wide:
        w, n = min(w, 5), int(rng.integers(255, 257))
    negated = bool(rng.random() < 0.4)
    if kind == "exact":
        n, negated, w = 1, False, min(w, 8)
    elif n == 1:
        negated = True
    pool = np.frombuffer(alphabet, dtype=np.uint8)
    strings = []
    while len(strings) < n:
        s = bytes(rng.choice(pool, size=w)) if len(strings) < 6 else bytes(rng.integers(0, 256, size=w, dtype=np.uint8))
        if s not in strings:
            strings.append(s)
    return ("!(" if negated else "(") + "|".join(s.hex() for s in strings) + ")", strings, negated


def random_part(rng, alphabet=LETTERS, anchor=(2, 4), context=2, group_share=0.0, groups_out=None):
    """(body text, sets) of one part: up to `context` positions in front of and behind an anchor of exact bytes,
    sometimes a ?? and one more exact byte inside; ?? never at an edge.  group_share: the share of parts that get
    a group token (two for "adjacent") at one of GROUP_PLACES: as the part's first or last positions, directly in
    front of or behind the anchor; its positions are full sets, and groups_out receives the (at, strings, negated)
    of the part.  With a share of 0 no random number is drawn for it."""
    def exact(n):
        bs = [int(x) for x in rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n)]
        return [("%02x" % c, frozenset((c,))) for c in bs]
    pre, post = int(rng.integers(0, context + 1)), int(rng.integers(0, context + 1))
    pos = [_position(rng, alphabet, EDGE_KINDS if i == 0 else INNER_KINDS) for i in range(pre)]
    pos += exact(int(rng.integers(anchor[0], anchor[1] + 1)))
    behind = len(pos)
    if rng.random() < 0.25:
        pos += [("??", wm.FULL)] + exact(1)
    pos += [_position(rng, alphabet, EDGE_KINDS if i == post - 1 else INNER_KINDS) for i in range(post)]
    if not group_share or rng.random() >= group_share:
        return "".join(t for t, _ in pos), [s for _, s in pos]
    # tokens of one position so far; a group token stands for several
    place = GROUP_PLACES[int(rng.integers(len(GROUP_PLACES)))]
    at = {"first": 0, "last": len(pos), "front": pre, "behind": behind}.get(place, (pre, behind, 0, len(pos))[int(rng.integers(4))])
    new = [random_group(rng, alphabet, place) for _ in range(2 if place == "adjacent" else 1)]
    toks = [(t, [s], None) for t, s in pos]
    toks[at:at] = [(t, [frozenset((b,)) for b in strings[0]], None) if place == "exact" else (t, [wm.FULL] * len(strings[0]), (strings, neg))
                   for t, strings, neg in new]
    sets = []
    for _, ss, grp in toks:
        if grp is not None and groups_out is not None:
            groups_out.append((len(sets), grp[0], grp[1]))
        sets += ss
    return "".join(t for t, _, _ in toks), sets


def random_gap(rng, longest=6):
    """(token, lo, hi or None)"""
    n = int(rng.integers(0, longest))
    m = n + int(rng.integers(0, longest))
    return [("{%d}" % n, n, n), ("{%d-%d}" % (n, m), n, m), ("{-%d}" % m, 0, m), ("{%d-}" % n, n, None),
            ("*", 0, None)][int(rng.integers(5))]


def random_body(rng, parts=(1, 4), groups_out=None, **kw):
    """(body, [sets of each part], [(lo, hi)]); groups_out: a list that receives the groups of each part (with
    group_share=..., see random_part)"""
    k = int(rng.integers(parts[0], parts[1] + 1))
    body, sets, gaps = "", [], []
    for j in range(k):
        if j:
            tok, lo, hi = random_gap(rng)
            body += tok
            gaps.append((lo, hi))
        if groups_out is not None:
            groups_out.append([])
            kw["groups_out"] = groups_out[-1]
        t, s = random_part(rng, **kw)
        body += t
        sets.append(s)
    return body, sets, gaps


def other_than(rng, strings, s, alphabet):
    """s with one byte changed, its last or for widths above 4 its first, and none of the strings: the bytes a
    word-wise compare sees last, or that a compare of the first word alone does not see"""
    i = 0 if len(s) > 4 else len(s) - 1
    while True:
        c = int(alphabet[int(rng.integers(len(alphabet)))]) if rng.random() < 0.7 else int(rng.integers(0, 256))
        t = s[:i] + bytes([c]) + s[i + 1:]
        if t not in strings:
            return t


def group_bytes(rng, group, alphabet, miss):
    """the bytes to lay under a group.  It holds: one of the strings of a positive group; for a negated one
    letters that are none of them, or every other time a string with one byte changed (other_than).  miss, a
    near miss, it fails: a string of a positive group with one byte changed, a string of a negated one as it is."""
    _, strings, negated = group
    s = strings[int(rng.integers(len(strings)))]
    if negated != miss:                                   # bytes that are none of the strings
        if negated and rng.random() < 0.5:
            while True:
                t = bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=len(s)))
                if t not in strings:
                    return t
        return other_than(rng, strings, s, alphabet)
    return s


NEAR_MISS = 0.5     # materialise(near_miss=True): the share of groups under which it lays bytes that fail


def materialise(rng, sets, gaps, alphabet=LETTERS, nocase=False, groups=None, near_miss=False):
    """bytes that the signature matches from their first to their last byte.  groups: per part its (at, strings,
    negated); near_miss: every position holds a byte of its set, but each group fails with probability NEAR_MISS
    (and the last one if none did): only the groups decide that this is no match."""
    pool = np.frombuffer(alphabet, dtype=np.uint8)
    out = bytearray()
    todo = sum(len(g) for g in groups) if groups else 0
    missed = False
    for j, part in enumerate(sets):
        if j:
            lo, hi = gaps[j - 1]
            n = lo + int(rng.integers(0, 3 if hi is None else min(hi - lo, 2) + 1))
            out += bytes(rng.choice(pool, size=n))
        at, L = longest_exact_run(part)
        base = len(out)
        for i, s in enumerate(part):
            good = [c for c in alphabet if c in s] or sorted(s)
            c = good[int(rng.integers(len(good)))]
            if nocase and at <= i < at + L and rng.random() < 0.5:
                c = c ^ 0x20 if 0x41 <= (c & 0xDF) <= 0x5A else c
            out.append(c)
        for g in groups[j] if groups else ():
            todo -= 1
            miss = near_miss and (rng.random() < NEAR_MISS or (todo == 0 and not missed))
            missed |= miss
            out[base + g[0]:base + g[0] + len(g[1][0])] = group_bytes(rng, g, alphabet, miss)
    return bytes(out)


def random_expr(rng, nops):
    """an expression over operands 0 .. nops - 1 that acm_automaton_add_rule accepts, each operand named once"""
    def cmp_(text):
        r = rng.random()
        if r < 0.55:
            return text
        return text + ["=%d" % rng.integers(0, 3), ">%d" % rng.integers(0, 3), "<%d" % rng.integers(1, 4)][int(rng.integers(3))]

    def tree(ops):
        if len(ops) == 1:
            return cmp_("%d" % ops[0])
        cuts = sorted(set(int(x) for x in rng.integers(1, len(ops), size=int(rng.integers(1, 3)))))
        groups = [ops[a:b] for a, b in zip([0] + cuts, cuts + [len(ops)])]
        op = "&|"[int(rng.integers(2))]
        kids = [tree(g) if len(g) == 1 else cmp_("(" + tree(g) + ")") for g in groups]
        return op.join(kids)
    for _ in range(200):
        e = tree(list(range(nops)))
        try:
            rm.parse(e, nops)
            return e
        except rm.RuleError:
            continue
    return "|".join("%d" % j for j in range(nops))


class Generated:
    """A seeded database and corpus (make): lines, rule_nocase (one flag per LINE: every body of a line shares it,
    as acm_automaton_add_logical_signature takes it), nocase (the same per signature), windows {(signature, 0):
    window}, texts, and db: the Database of them"""


ALPHABET = LETTERS + b"2"


def _random_text(rng, n, alphabet=ALPHABET):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n))


def make(seed, rules=64, texts=3000, total=204 * 1024, empties=2200, long_text=17000, max_ops=8, window_share=0.2,
         anchor=(5, 6), group_share=0.0):
    """about 4.5 * rules signatures of 1 - 4 parts with anchors of 5 or 6 bytes (every pattern has its three bytes:
    the sparse pipeline applies; and a text has fewer anchor records than bytes, which is what acm_grep -Q takes
    per buffer) and a corpus in which every signature is planted: texts that are one match, texts
    that hold all or some operands of a rule, one long text, a run of empty texts, texts of one byte and of exactly
    one part.  group_share: that share of the parts carries a group (random_part); the database is then in the
    grammar with groups, every planted match lays bytes under its groups that hold, and every signature with a
    group has a text of its own that is a near miss (materialise).  The expressions are drawn last, so that every
    rule holds in some text and fails in another that has a hit (the draw looks at sequences() of the corpus,
    never at a device)."""
    rng = np.random.default_rng(seed)
    g = Generated()
    sigs, bodies, ops_of, g.rule_nocase, g.nocase, g.windows = [], [], [], [], [], {}
    with_groups = group_share > 0
    g.groups = []                                        # per signature, per part: (at, strings, negated)
    for r in range(rules):
        nc = bool(rng.random() < 0.34)
        g.rule_nocase.append(nc)
        ops = []
        for _ in range(int(rng.integers(1, max_ops + 1))):
            if with_groups:
                g.groups.append([])
                body, sets, gaps = random_body(rng, parts=(1, 4), alphabet=ALPHABET, anchor=anchor, group_share=group_share,
                                               groups_out=g.groups[-1])
            else:
                body, sets, gaps = random_body(rng, parts=(1, 4), alphabet=ALPHABET, anchor=anchor)
            q = len(sigs)
            sigs.append((sets, gaps))
            bodies.append(body)
            g.nocase.append(nc)
            ops.append(q)
            if rng.random() < window_share:
                n0 = len(sets[0])
                lo = int(rng.integers(0, 6))
                choice = [(0, 0, False), (lo, lo + int(rng.integers(0, 40)), False), (lo, None, False), (0, 90, True),
                          (lo, 120, True)] + ([(n0, n0, True)] if len(sets) == 1 else [])
                g.windows[q, 0] = choice[int(rng.integers(len(choice)))]
        ops_of.append(ops)

    def planted(q, room=12):
        """a text in which signature q matches inside its window"""
        inst = materialise(rng, sigs[q][0], sigs[q][1], ALPHABET, g.nocase[q], g.groups[q] if with_groups else None)
        lo, hi, from_end = g.windows.get((q, 0), (0, None, False))
        if from_end:
            after = max(lo - len(inst), 0) if hi == lo else int(rng.integers(max(lo - len(inst), 0), max(lo - len(inst), 0) + 3))
            return _random_text(rng, int(rng.integers(0, room))) + inst + _random_text(rng, after)
        front = lo + int(rng.integers(0, (min(hi - lo, room) if hi is not None else room) + 1))
        return _random_text(rng, front) + inst + _random_text(rng, int(rng.integers(0, room)))

    out = [b"", _random_text(rng, 1), b"a"]
    for q in range(len(sigs)):
        out.append(planted(q))
        if q % 5 == 0:
            out.append(materialise(rng, sigs[q][0][:1], [], ALPHABET, g.nocase[q], g.groups[q][:1] if with_groups else None))   # exactly one part
        if with_groups and any(g.groups[q]):
            miss = materialise(rng, sigs[q][0], sigs[q][1], ALPHABET, g.nocase[q], g.groups[q], near_miss=True)
            out.append(_random_text(rng, int(rng.integers(0, 6))) + miss + _random_text(rng, int(rng.integers(0, 6))))
    for ops in ops_of:
        for share in (1.0, 0.6, 0.3):
            t = b""
            for q in ops:
                if rng.random() < share:
                    t += b"".join(planted(q, 4) for _ in range(int(rng.integers(1, 4))))
            out.append(t)
    long_one = bytearray(_random_text(rng, long_text))
    at = 50
    while at + 200 < long_text:
        inst = planted(int(rng.integers(len(sigs))), 3)
        long_one[at:at + len(inst)] = inst
        at += len(inst) + int(rng.integers(0, 120))
    filler = max(texts - empties - len(out) - 1, 0)
    room = max(total - long_text - sum(len(t) for t in out), 0)
    for _ in range(filler):
        out.append(_random_text(rng, int(rng.integers(1, 2 * room // max(filler, 1) + 2))))
    order = rng.permutation(len(out))
    out = [out[i] for i in order]
    cut = len(out) // 3
    g.texts = out[:cut] + [b""] * empties + [bytes(long_one)] + out[cut:]
    # the expressions
    g.db = Database(["%s;%s" % ("|".join("%d" % j for j in range(len(ops))), ";".join(bodies[q] for q in ops)) for ops in ops_of],
                    g.nocase, g.windows, with_groups)
    c = Corpus(g.texts)
    found = sequences(g.db, c)
    counts = count_matrix(g.db, c, found[1], found[2])
    g.lines = []
    for r, ops in enumerate(ops_of):
        sub = counts[ops]
        hit = np.flatnonzero(sub.sum(axis=0))
        expr = None
        for _ in range(300):
            e = random_expr(rng, len(ops))
            truth = [rm.evaluate(rm.parse(e, len(ops)), sub[:, t])[1] for t in hit[:400].tolist()]
            if any(truth) and not all(truth):
                expr = e
                break
        g.lines.append("%s;%s" % (expr or "|".join("%d" % j for j in range(len(ops))), ";".join(bodies[q] for q in ops)))
    g.db = Database(g.lines, g.nocase, g.windows, with_groups)
    return g


def small_slice(texts, count=300, chunk=64, longest=900, empties=4):
    """count of the texts, in their order: those of at most `longest` bytes and only the first few empty ones.
    Returns (texts, chunks): the chunks of `chunk` bytes they take when every text begins a chunk of its own."""
    out, seen_empty = [], 0
    for t in texts:
        if len(t) > longest or (not t and seen_empty >= empties):
            continue
        seen_empty += not t
        out.append(t)
        if len(out) == count:
            break
    return out, sum(max(1, -(-len(t) // chunk)) for t in out)
