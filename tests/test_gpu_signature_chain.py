"""The signature chain at the sizes and in the combinations a real database produces.

1. Slot counts at the radix borders.  Sets whose sequence-slot count, and sets whose rule-slot count, is exactly
   255, 256, 257, 65 535 and 65 536: one, two, two, two and three 8-bit radix passes.  acm_sequence_matches_async
   and acm_rule_matches_async run over synthetic planes of 1, 1025 and 2049 records (and once 1024 * 1024 + 1025)
   whose cells hit the slots next to every digit border, the all-ones key between them, long runs of one slot across
   tile and block cuts and multi-part chains that a text start does or does not cut; cell for cell against
   sequence_model.SequenceModel and rule_model.RuleModel, from poisoned outputs and workspaces (the run_pass
   helpers of test_gpu_sequences.py and test_gpu_rules.py).
   A sequence slot is a part and a set with multi-part sequences has more slots than sequences, while a rule slot
   is an operand and needs a sequence of its own: one set cannot sit at the same border for both passes, so every
   border has a set for either pass (each set carries sequences AND rules; the other pass's count lies beside it).
2. The whole chain on real scan output: a seeded database of about 300 extended signatures under 70 rules and a
   corpus of 3000 texts (signature_oracle.make), through Matcher.scan_sequences / scan_rules under both scan
   pipelines and through every pass enqueued on one created stream the way acm_grep enqueues them, against
   tests/signature_oracle.py: exact equality of the records, and of the record counts the case, wildcard,
   position, sequence and rule passes write (the oracle has no count for the scan and the segment pass: theirs
   are printed, and bounded below by the offsets that have a match).
"""
import time

import numpy as np
import pytest

import poison
import position_model as pm
import rule_model as rm
import sequence_model as sm
import signature_oracle as so
import streams
import test_gpu_rules as trul
import test_gpu_sequences as tseq
import wildcard_model as wm
from gpu_pattern_matching_amd import Automaton, Matcher, _lib

pytestmark = pytest.mark.gpu

NO_CELL = tseq.NO_CELL
BIG = tseq.BIG
COUNTS = [1, 1025, 2049]
BORDERS = [255, 256, 257, 65535, 65536]
PASSES = {255: 1, 256: 2, 257: 2, 65535: 2, 65536: 3}
EDGE_SLOTS = [0, 254, 255, 256, 0xFF00, 0xFFFE, 0xFFFF, 0x10000]
MULTI_GAPS = {2: [(1, 3)], 3: [(0, None), (2, 2)], 4: [(0, 4), (1, 1), (0, 300)]}
MULTI_STEPS = {2: [7], 3: [6, 7], 4: [6, 6, 10]}          # end-to-end distances that satisfy the gaps (parts of 5 bytes)
PAT_LEN = 5


def passes_for(slots):
    """8-bit passes that tell the keys 0 .. slots - 1 and the all-ones key apart: slots <= 256 ** p - 1"""
    p = 1
    while slots > 256 ** p - 1:
        p += 1
    return p


def rule_expr(r, n):
    alls = "|".join("%d" % j for j in range(n))
    if n == 1:
        return "0"
    return [alls, "(%s)>1&%d=0" % ("|".join("%d" % j for j in range(n - 1)), n - 1),
            "0&(%s)" % "|".join("%d" % j for j in range(1, n)), "(%s)>2" % alls][r % 4]


class BorderSet:
    """kind "seq": exactly `slots` sequence slots; kind "rule": exactly `slots` rule slots.  Patterns are five hex
    digits (a small automaton); all sequences have one part but three, of 2, 3 and 4 parts, whose higher levels
    take the highest slots; the rules take 64 consecutive sequences each, the last one what is left"""

    def __init__(self, kind, slots):
        t0 = time.perf_counter()
        S = slots - 6 if kind == "seq" else slots + 2
        self.kind, self.slots, self.S = kind, slots, S
        multi_at = {5: 2, S // 2: 3, S - 1: 4}
        self.npat = S - 3 + 9 + 1                              # the last pattern is in no sequence
        a = Automaton()
        for i in range(self.npat):
            a.add(b"%05x" % i, i)
        self.seqs, nxt = [], 0
        for q in range(S):
            k = multi_at.get(q, 1)
            self.seqs.append((list(range(nxt, nxt + k)), MULTI_GAPS.get(k, [])))
            a.add_sequence(self.seqs[-1][0], self.seqs[-1][1], iid=q)
            nxt += k
        a.compile()
        self.R = slots if kind == "rule" else S - 2           # the last two sequences are operands of nothing
        self.rules = []
        for r, at in enumerate(range(0, self.R, 64)):
            n = min(64, self.R - at)
            self.rules.append((list(range(at, at + n)), rule_expr(r, n)))
            assert a.add_rule(self.rules[-1][0], self.rules[-1][1], iid=r) == r
        self.host_seconds = time.perf_counter() - t0
        self.a = a
        # slots as device_dfa.hip numbers them: parts level-major, operands rule-major
        self.seq_slot = np.full(self.npat, -1, dtype=np.int64)
        n = 0
        for j in range(4):
            for parts, _ in self.seqs:
                if len(parts) > j:
                    self.seq_slot[parts[j]] = n
                    n += 1
        self.seq_slots = n
        self.pat_of_slot = np.argsort(np.where(self.seq_slot < 0, 1 << 40, self.seq_slot))[:n]
        self.rule_slots = sum(len(ops) for ops, _ in self.rules)
        assert (self.seq_slots if kind == "seq" else self.rule_slots) == slots
        self.multi = [self.seqs[q] for q in sorted(multi_at)]
        self.m = None

    def matcher(self):
        if self.m is None:
            t0 = time.perf_counter()
            self.m = Matcher(self.a, 0, max_text=4096)
            print("set %s/%d: upload %.2f s" % (self.kind, self.slots, time.perf_counter() - t0))
        return self.m

    def close(self):
        if self.m is not None:
            self.m.close()
        self.a.close()


_SETS = {}


@pytest.fixture(scope="module")
def border_sets(gpu):
    """every set is built once, when its first test asks for it"""
    def get(kind, slots):
        if (kind, slots) not in _SETS:
            _SETS[kind, slots] = BorderSet(kind, slots)
            b = _SETS[kind, slots]
            print("set %s/%d: %d sequence slots, %d rule slots, host build %.2f s" % (kind, slots, b.seq_slots, b.rule_slots,
                                                                                       b.host_seconds))
        return _SETS[kind, slots]
    yield get
    for b in _SETS.values():
        b.close()
    _SETS.clear()


class SubModel:
    """sm.SequenceModel of the sequences the cells can name (the model loops over sequences, and a set has
    65 536 of them); the sequence indices it reports are mapped back"""

    def __init__(self, bs, pool):
        seq_of = {}
        for q, (parts, _) in enumerate(bs.seqs):
            for p in parts:
                seq_of[p] = q
        self.ids = np.array(sorted({seq_of[p] for p in pool if p in seq_of}), dtype=np.int64)
        self.pool = set(pool)
        self.inner = sm.SequenceModel([PAT_LEN] * bs.npat, [bs.seqs[q] for q in self.ids])

    def run(self, cells, offs, starts=(), lead_begin=0):
        assert set(np.asarray(cells).tolist()) <= self.pool | {NO_CELL, -1}
        q, o, info = self.inner.run(cells, offs, starts, lead_begin)
        return self.ids[q].astype(np.int32), o, info


def edge_slots(n):
    return sorted({s for s in EDGE_SLOTS + [n - 1] if s < n})


def lay_out(pool, edges, runs, chains, m, seed):
    """(cells, offsets) of m records.  A quarter of the cells names nothing (no index, -1, or an index that is in
    no sequence / no rule: the all-ones key); offsets in runs of equal values as tseq.syn_planes; edges: cells
    that must occur, laid down with a no-key cell between two of them; runs: (begin, end, cell) stretches of one
    cell; chains: (cells, steps) planted twelve times, one record after the other at those offset steps"""
    rng = np.random.default_rng(seed)
    nothing = np.array([NO_CELL, -1, pool[-1]], dtype=np.int64)
    cells = np.where(rng.random(m) < 0.25, nothing[rng.integers(0, 3, m)], np.array(pool[:-1], dtype=np.int64)[rng.integers(0, len(pool) - 1, m)])
    d = (rng.random(m) < 0.7) * rng.integers(1, 3, m)
    if m > 1024:
        for i, e in enumerate(edges):
            cells[10 + 2 * i], cells[11 + 2 * i] = e, NO_CELL
        for b, e, c in runs:
            cells[b:e] = c
        at = 100
        for k in range(12 * len(chains)):
            parts, steps = chains[k % len(chains)]
            if at + len(parts) >= min(m, 1000):
                break
            cells[at:at + len(parts)] = parts
            d[at + 1:at + len(parts)] = steps
            at += len(parts) + int(rng.integers(3, 30))
    else:
        cells[0] = edges[0]
    return cells, (np.cumsum(d) + 3).astype(np.int64)


def run_cuts(m):
    """where the long runs lie: across the tile cut at 1024 and behind it; for the big count across three block
    cuts (a block owns 2048 consecutive records there)"""
    if m >= BIG:
        return [(2048 * 100 - 300, 2048 * 100 + 300), (2048 * 300 + 1024 - 150, 2048 * 300 + 1024 + 150),
                (2048 * 512 - 700, 2048 * 512 + 700)]
    return [(1010, 1040), (1100, 1400), (2040, 2049)] if m > 2048 else [(1010, 1025)]


def seq_case(bs, m):
    """(cells, offsets, pool) for the sequence pass over set bs"""
    rng = np.random.default_rng(bs.slots)
    edges = [int(bs.pat_of_slot[s]) for s in edge_slots(bs.seq_slots)]
    multi = [p for parts, _ in bs.multi for p in parts]
    pool = edges + multi + [int(x) for x in rng.integers(0, bs.npat - 1, 24)] + [bs.npat - 1]
    hot = [edges[-1], edges[min(2, len(edges) - 1)], edges[0]]
    runs = [(b, e, hot[i % 3]) for i, (b, e) in enumerate(run_cuts(m))]
    chains = [(parts, MULTI_STEPS[len(parts)]) for parts, _ in bs.multi]
    cells, offs = lay_out(pool, edges, runs, chains, m, 5000 + m)
    return cells, offs, pool


def rule_case(bs, m):
    """(cells, offsets) for the rule pass over set bs: the cells are sequence indices; sequence q is operand q % 64
    of rule q // 64"""
    rng = np.random.default_rng(bs.slots + 1)
    edges = edge_slots(bs.rule_slots)
    mates = sorted({q - q % 64 for q in edges} | {min(q - q % 64 + 1, bs.R - 1) for q in edges})    # operands 0 and 1 of their rules
    pool = edges + mates + [int(x) for x in rng.integers(0, bs.R, 24)] + [bs.S - 1]
    hot = [edges[-1], edges[min(2, len(edges) - 1)], edges[0]]
    runs = [(b, e, hot[i % 3]) for i, (b, e) in enumerate(run_cuts(m))]
    return lay_out(pool, edges, runs, [], m, 6000 + m)


def check_sequence_pass(bs, m):
    cells, offs, pool = seq_case(bs, m)
    model = SubModel(bs, pool)
    slot = np.where((cells >= 0) & (cells < bs.npat), bs.seq_slot[np.clip(cells, 0, bs.npat - 1)], -1)
    if m > 1024:
        assert set(edge_slots(bs.seq_slots)) <= set(slot.tolist()) and (slot < 0).sum() > m // 8
        b, e = run_cuts(m)[0]                                              # a run of one slot across a tile (big: block) cut
        assert (slot[b:e] == slot[b]).all() and slot[b] >= 0 and e - b >= 15
    text_end = tseq.end_of(offs)
    starts = tseq.syn_starts(text_end)
    planes = tseq.upload(cells, offs)
    what = "%s/%d" % (bs.kind, bs.slots)
    eq, eo, info = tseq.run_pass(bs.matcher(), model, planes, cells, offs, starts=starts, lead_begin=-20, text_end=text_end, what=what)
    if 1024 < m < BIG:
        one = tseq.run_pass(bs.matcher(), model, planes, cells, offs, lead_begin=-20, text_end=text_end, what=what + " one text")
        # every multi-part sequence matches, and less often when text starts cut the chains: a predecessor counts
        # only in the same text
        multi_ids = [bs.seqs.index(s) for s in bs.multi]
        for q in multi_ids:
            assert 0 < (eq == q).sum() < (one[0] == q).sum(), (q, (eq == q).sum(), (one[0] == q).sum())
        assert info[0] > info[1] > eq.size > 0
    for x in planes:
        x.free()
    return info


def check_rule_pass(bs, m):
    cells, offs = rule_case(bs, m)
    model = bs.rule_model
    slot = np.where((cells >= 0) & (cells < bs.R), cells, -1)
    if m > 1024:
        assert set(edge_slots(bs.rule_slots)) <= set(slot.tolist()) and (slot < 0).sum() > m // 8
    starts = trul.syn_starts(trul.end_of(offs))
    planes = trul.upload(cells, offs)
    what = "%s/%d" % (bs.kind, bs.slots)
    er, et, eo, info = trul.run_pass(bs.matcher(), model, planes, cells, offs, starts=starts, what=what)
    if m < BIG:
        trul.run_pass(bs.matcher(), model, planes, cells, offs, what=what + " one text")
    if m > 1024:
        assert info[0] > info[1] > info[2] > er.size > 0 and len(set(er.tolist())) >= 3
    for x in planes:
        x.free()
    return info


def rule_model_of(bs):
    if not hasattr(bs, "rule_model"):
        bs.rule_model = rm.RuleModel(bs.S, bs.rules)
    return bs.rule_model


@pytest.mark.parametrize("slots", BORDERS)
def test_sequence_slots_at_the_radix_borders(border_sets, slots):
    assert passes_for(slots) == PASSES[slots]
    bs = border_sets("seq", slots)
    assert bs.seq_slots == slots
    for m in COUNTS:
        check_sequence_pass(bs, m)


@pytest.mark.parametrize("slots", BORDERS)
def test_rule_slots_at_the_radix_borders(border_sets, slots):
    assert passes_for(slots) == PASSES[slots]
    bs = border_sets("rule", slots)
    assert bs.rule_slots == slots and bs.seq_slots == slots + 8
    rule_model_of(bs)
    for m in COUNTS:
        check_rule_pass(bs, m)
    if slots == 65536:
        # this set has 65 544 sequence slots: slot 0x10000, the first key above the 16-bit border, and 0x10007
        assert 0x10000 in edge_slots(bs.seq_slots)
        check_sequence_pass(bs, 2049)


def test_three_passes_over_every_block(border_sets):
    """1024 * 1024 + 1025 records (a block owns two tiles) in 65 536 slots: three radix passes whose scatter spans
    every block, the slot borders found in keys that three passes ordered"""
    check_sequence_pass(border_sets("seq", 65536), BIG)
    bs = border_sets("rule", 65536)
    rule_model_of(bs)
    check_rule_pass(bs, BIG)


# ------------------------------------------------------------------ 2. the whole chain

SEED = 1
SLACK = 256                     # guard bytes behind every plane and workspace of a device chain
GUARD = 0x3C


class Case:
    """the generated database and corpus, what the oracle says of them, and the models' view of the patterns.
    made: another so.make() result than the one of this file (test_gpu_signature_chain_groups.py); groups: its
    lines are in the grammar with groups"""

    def __init__(self, made=None, groups=False):
        t0 = time.perf_counter()
        self.g = g = so.make(SEED, rules=70) if made is None else made()
        self.groups = groups
        self.corpus = so.Corpus(g.texts)
        self.counts = {}
        self.found = so.sequences(g.db, self.corpus, counts=self.counts)
        self.fired = so.rules(g.db, self.corpus, self.found)
        self.pairs = so.evaluated_pairs(g.db, self.corpus, self.found)
        self.small_texts = so.small_slice(g.texts)[0]        # 300 short texts, a second corpus
        self.runs = {}
        self.seconds = time.perf_counter() - t0

    def automaton(self, lines=None, rule_nocase=None, windows=None, extra=None):
        """the database line by line through add_logical_signature(extended=True): a file has one case flag for
        all its lines (load_logical_file; test_gpu_signature_chain_cli.py loads the database that way), a line its
        own.  extra: one more pattern, in no sequence"""
        g = self.g
        a = Automaton()
        lines = g.lines if lines is None else lines
        rule_nocase = g.rule_nocase if rule_nocase is None else rule_nocase
        for r, line in enumerate(lines):
            assert a.add_logical_signature(line, iid=r, nocase=rule_nocase[r], extended=True, groups=self.groups) == r
        if extra is not None:
            a.add(extra, 0)
        a.compile()
        for (q, j), w in (g.windows if windows is None else windows).items():
            a.set_position(a.sequence(q)[0][j], *w)
        return a


@pytest.fixture(scope="module")
def case(gpu):
    return Case()


def expected_of(db, texts, **kw):
    c = so.Corpus(texts)
    counts = {}
    found = so.sequences(db, c, counts=counts, **kw)
    return c, counts, found, so.rules(db, c, found)


def seq_tuples(found):
    return sorted(zip(found[0].tolist(), found[2].tolist()))


def test_the_input_is_worth_running(case):
    """from the oracle alone"""
    g, c, counts = case.g, case.corpus, case.counts
    print("oracle and generator: %.1f s; stage counts %s, rule records %d, (rule, text) pairs %d" % (
        case.seconds, counts, len(case.fired), case.pairs))
    nsig, nrule = len(g.db.sigs), len(g.db.rules)
    parts = sum(len(p) for p, _ in g.db.sigs)
    assert 250 <= nsig <= 350 and parts > 255 and sum(len(ops) for ops, _ in g.db.rules) > 255 and 55 <= nrule <= 75
    assert 0.25 < sum(g.nocase) / nsig < 0.45 and 0.12 < len(g.windows) / nsig < 0.3
    assert any(w == (0, 0, False) for w in g.windows.values()) and any(w[2] and w[0] == 0 for w in g.windows.values())
    body = "".join(g.lines)
    for token in ("?", "(", "!(", "??", "{", "-}", "{-", "*", "&", "|", "=", ">", "<", "(("):
        assert token in body, token
    lens = np.array([len(t) for t in g.texts])
    assert 2900 <= lens.size <= 3100 and 180 * 1024 <= lens.sum() <= 210 * 1024 and lens.max() > 16 * 1024
    empty_run = max(len(r) for r in "".join("e" if n == 0 else "." for n in lens).split("."))
    assert empty_run > 2100 and (lens == 1).any()
    first_parts = {len(p[0].sets) for p, _ in g.db.sigs}
    assert first_parts & set(lens.tolist())
    # the case pass sees the scan's records (at least one per anchor end that stays), the wildcard pass every anchor,
    # the position pass every part, the sequence pass those inside their windows, the rule pass the matches
    assert min(counts["anchors"], counts["parts"], counts["windowed"], counts["matches"]) >= 2049
    assert np.unique(case.found[1]).size >= 2049                      # offsets with a record: what the case pass gets, at least
    assert set(case.found[2].tolist()) == set(range(nsig))            # every signature holds somewhere
    m = so.count_matrix(g.db, c, case.found[1], case.found[2])
    assert ((m == 0).any(axis=1)).all()                               # ... and fails somewhere
    holds = {}
    for r, t, o in case.fired:
        holds.setdefault(r, set()).add(t)
    fails_on_a_hit = 0
    for r, (ops, _) in enumerate(g.db.rules):
        hit = set(np.flatnonzero(m[ops].sum(axis=0)).tolist())
        assert holds.get(r) and len(holds[r]) < lens.size, r          # every rule holds in a text and fails in another
        fails_on_a_hit += bool(hit - holds[r])
    assert fails_on_a_hit >= 0.9 * nrule                              # ... nearly all of them in a text where an operand occurs
    first = {}
    for o in case.found[1].tolist():
        first.setdefault(int(c.text_of[o]), o)
    assert sum(o != first[t] for _, t, o in case.fired) > 100         # triggers that are not their text's first record
    # more than 2048 starts under one tile of records: the records around the run of empty texts
    at = int(c.starts[int(np.flatnonzero(lens == 0)[5])])
    assert (case.found[1] < at).sum() > 1024 and (case.found[1] >= at).sum() > 1024
    base = seq_tuples(case.found)
    for drop in ("nocase", "windows", "contexts"):
        assert seq_tuples(so.sequences(g.db, c, **{drop: False})) != base, drop


def matcher_for(a, name, max_text):
    """a Matcher that scans under the pipeline `name` (the chain set has a one-byte pattern: not sparse-eligible)"""
    m = Matcher(a, 0, max_text=max_text)
    assert m.sparse_eligible() == (name == "sparse")
    if name == "sparse":
        assert m.set_mode("sparse") == "sparse"
    return m


def pipeline_run(case, name):
    """scan_sequences and scan_rules of the corpus under one pipeline, once per session"""
    if name not in case.runs:
        a = case.automaton(extra=None if name == "sparse" else b"a")
        assert a.has_wildcards and a.mixed_case and a.positioned
        m = matcher_for(a, name, case.corpus.N)
        go, gq, _, info = m.scan_sequences(texts=case.g.texts)
        path = m.path_taken(case.corpus.N)
        r, t, o, rinfo = m.scan_rules(texts=case.g.texts)
        long_one = max(case.g.texts, key=len)
        lo, lq, _, _ = m.scan_sequences(long_one)
        lr, lt, lx, _ = m.scan_rules(long_one)
        case.runs[name] = dict(records=(go, gq, r, t, o), info=info.tolist(), rinfo=rinfo.tolist(), path=path,
                               long=(lo, lq, lr, lt, lx))
        m.close()
        a.close()
    return case.runs[name]


@pytest.mark.parametrize("name", ["sparse", "chain"])
def test_scan_sequences_and_rules(case, name):
    g = case.g
    run = pipeline_run(case, name)
    assert run["path"] == name
    go, gq, r, t, o = run["records"]
    got = sorted(zip(go.tolist(), gq.tolist()))
    want = seq_tuples(case.found)
    assert got == want, (len(got), len(want), sorted(set(got) ^ set(want))[:6])
    assert run["info"][0] == case.counts["windowed"]
    assert sorted(zip(r.tolist(), t.tolist(), o.tolist())) == case.fired
    assert run["rinfo"][2] == case.pairs and run["rinfo"][0] <= case.counts["matches"]
    # one text alone: the long one
    _, counts, found, fired = expected_of(g.db, [max(g.texts, key=len)])
    lo, lq, lr, lt, lx = run["long"]
    assert sorted(zip(lo.tolist(), lq.tolist())) == seq_tuples(found) and counts["matches"] > 100
    assert sorted(zip(lr.tolist(), (lt + 1).tolist(), lx.tolist())) == fired and (lt == -1).all() and len(fired) > 10


def test_the_pipelines_agree_bit_for_bit(case):
    x, y = pipeline_run(case, "sparse"), pipeline_run(case, "chain")
    for u, v in zip(x["records"] + x["long"], y["records"] + y["long"]):
        assert np.array_equal(u, v)
    assert x["info"] == y["info"] and x["rinfo"] == y["rinfo"]


@pytest.mark.parametrize("name", ["sparse", "chain"])
def test_a_piece_with_the_bytes_in_front(case, name):
    """the window-free lines of the database over the long text cut in two: the second piece through scan_sequences
    and scan_rules with the first as `before` and lead_begin in front of it.  Contexts and gaps reach into the bytes
    in front; a part whose anchor begins there is no record of this scan, so it counts for no rule either."""
    g = case.g
    keep, nocase, q = [], [], 0
    for r, line in enumerate(g.lines):
        n = len(so.split_line(line)[1])
        if not any((q + j, 0) in g.windows for j in range(n)):
            keep.append(r)
            nocase += [g.rule_nocase[r]] * n
        q += n
    lines = [g.lines[r] for r in keep]
    assert len(lines) > 10
    db = so.Database(lines, nocase)
    a = case.automaton(lines, [g.rule_nocase[r] for r in keep], {}, extra=None if name == "sparse" else b"a")
    assert not a.positioned
    long_one = max(g.texts, key=len)
    cut = 5014                                   # a part's context lies in front of it, its anchor behind
    piece = long_one[cut:]
    m = matcher_for(a, name, len(long_one))
    go, gq, _, _ = m.scan_sequences(piece, before=long_one[:cut], lead_begin=-cut)
    assert m.path_taken(len(piece)) == name
    found = so.sequences(db, [long_one], anchors_from=cut)
    assert sorted(zip((go.astype(np.int64) + cut).tolist(), gq.tolist())) == seq_tuples(found) and found[0].size > 50
    # ... and some of them need the bytes in front: a context or a first part's span that begins there
    alone = so.sequences(db, [piece])
    assert set(seq_tuples(found)) - {(e + cut, s) for e, s in seq_tuples(alone)}
    r, t, o, rinfo = m.scan_rules(piece, before=long_one[:cut], lead_begin=-cut)
    assert m.path_taken(len(piece)) == name
    fired = so.rules(db, [long_one], found)
    assert sorted(zip(r.tolist(), (t + 1).tolist(), (o.astype(np.int64) + cut).tolist())) == fired and (t == -1).all()
    assert len(fired) > 3 and rinfo.tolist()[0] == found[0].size and fired != so.rules(db, [long_one], so.sequences(db, [long_one]))
    m.close()
    a.close()


class Guarded:
    """a device block with guard bytes behind it"""

    def __init__(self, rig, nbytes):
        self.n = int(nbytes)
        self.buf = rig.buf(self.n + SLACK)
        self.ptr = self.buf.ptr
        self.lib = rig.lib

    def poison(self, fill):
        _lib.check(self.lib.acm_rt_memset(self.ptr, fill, self.n, None), "acm_rt_memset")
        _lib.check(self.lib.acm_rt_memset(self.ptr + self.n, GUARD, SLACK, None), "acm_rt_memset")

    def intact(self, stream):
        return bool((self.buf.to_numpy(np.uint8, SLACK, offset_bytes=self.n, stream=stream) == GUARD).all())

    def cells(self, count, stream):
        return self.buf.to_numpy(np.int32, count, stream=stream)


class DeviceChain:
    """every pass from the scan to the rule pass on one stream, as acm_grep.cpp's finish() enqueues them: each
    pass takes max_records = capacity - 2 of the planes in front of it and a workspace sized by that; nothing is
    read back in between.  starve: the capacity of the case pass's output planes (and of every plane behind)."""

    def __init__(self, rig, m, texts, starve=None):
        self.rig, self.m, self.s = rig, m, rig.stream()
        t, starts = Matcher.pack_segments(texts)
        self.n, self.nseg = int(t.size), int(starts.size)
        host = np.zeros(poison.round16(self.n) + 16, dtype=np.uint8)
        host[:self.n] = t
        self.text = rig.upload(host)
        self.starts = rig.upload(starts, pad_to=0)
        lib, dfa = m.lib, m.dfa
        self.cap = cap = self.n + 2
        self.icap = icap = starve if starve is not None else 8 * cap
        mk = lambda cells: Guarded(rig, cells * 4)
        self.scan, self.seg = (mk(cap), mk(cap)), (mk(cap), mk(cap))
        self.all, self.wild, self.pos, self.seq = ((mk(icap), mk(icap)) for _ in range(4))
        self.rule = (mk(icap), mk(icap), mk(icap))
        self.info = [mk(4) for _ in range(4)]
        self.ws = dict(scan=Guarded(rig, lib.acm_scan_workspace_bytes(dfa, self.n)),
                       seg=Guarded(rig, lib.acm_segment_workspace_bytes(cap - 2)),
                       case=Guarded(rig, lib.acm_case_workspace_bytes(cap - 2)),
                       wild=Guarded(rig, lib.acm_wildcard_workspace_bytes(icap - 2)),
                       pos=Guarded(rig, lib.acm_position_workspace_bytes(icap - 2)),
                       seq=Guarded(rig, lib.acm_sequence_workspace_bytes(dfa, icap - 2)),
                       rule=Guarded(rig, lib.acm_rule_workspace_bytes(dfa, icap - 2)))
        self.blocks = [x for pair in (self.scan, self.seg, self.all, self.wild, self.pos, self.seq, self.rule) for x in pair] + \
            self.info + list(self.ws.values())

    def poison(self, fill):
        for b in self.blocks:
            b.poison(fill)

    def enqueue(self):
        m, s, n, cap, icap = self.m, self.s, self.n, self.cap, self.icap
        w = lambda k: (self.ws[k].ptr, self.ws[k].n)
        where = dict(seg_start=self.starts, segments=self.nseg, lead_begin=0)
        m.scan_async(self.text, n, 0, stream=s, pat_plane=self.scan[0].ptr, off_plane=self.scan[1].ptr, plane_capacity=cap,
                     workspace=w("scan"), report=_lib.REPORT_STATE)
        m.segment_async(self.scan[0].ptr, self.scan[1].ptr, cap - 2, self.starts, self.nseg, n, self.seg[0].ptr, self.seg[1].ptr,
                        cap, report=_lib.REPORT_STATE, workspace=w("seg"), stream=s)
        m.case_async(self.seg[0].ptr, self.seg[1].ptr, cap - 2, self.text, 0, n, self.all[0].ptr, self.all[1].ptr, icap,
                     all_patterns=True, workspace=w("case"), stream=s)
        m.wildcard_async(self.all[0].ptr, self.all[1].ptr, icap - 2, self.text, 0, n, self.wild[0].ptr, self.wild[1].ptr, icap,
                         self.info[0].ptr, report=_lib.REPORT_HEAD, open_end=n, all_patterns=True, workspace=w("wild"),
                         stream=s, **where)
        m.position_async(self.wild[0].ptr, self.wild[1].ptr, icap - 2, self.pos[0].ptr, self.pos[1].ptr, icap, self.info[1].ptr,
                         report=_lib.REPORT_HEAD, text_end=n, open_end=n, all_patterns=True, workspace=w("pos"), stream=s, **where)
        m.sequence_async(self.pos[0].ptr, self.pos[1].ptr, icap - 2, self.seq[0].ptr, self.seq[1].ptr, icap, self.info[2].ptr,
                         text_end=n, workspace=w("seq"), stream=s, **where)
        m.rule_async(self.seq[0].ptr, self.seq[1].ptr, icap - 2, self.rule[0].ptr, self.rule[1].ptr, self.rule[2].ptr, icap,
                     self.info[3].ptr, seg_start=self.starts, segments=self.nseg, workspace=w("rule"), stream=s)

    def counts(self):
        """the count cell of every pass's output"""
        return {k: int(p[0].cells(1, self.s)[0]) for k, p in
                (("scan", self.scan), ("seg", self.seg), ("all", self.all), ("wild", self.wild), ("pos", self.pos),
                 ("seq", self.seq), ("rule", self.rule))}

    def records(self, planes):
        k = min(int(planes[0].cells(1, self.s)[0]), self.icap - 2)
        return [p.cells(k + 1, self.s)[1:] for p in planes]

    def check_guards(self, what):
        self.rig.sync(self.s)
        bad = [i for i, b in enumerate(self.blocks) if not b.intact(self.s)]
        assert not bad, "%s: written behind block(s) %s" % (what, bad)


def check_chain(ch, counts, found, fired, what):
    ch.check_guards(what)
    got = ch.counts()
    assert (got["all"], got["wild"], got["pos"], got["seq"], got["rule"]) == \
        (counts["anchors"], counts["parts"], counts["windowed"], counts["matches"], len(fired)), (what, got, counts)
    assert got["scan"] >= got["seg"] >= np.unique(found[1]).size
    q, o = ch.records(ch.seq)
    assert sorted(zip(o.tolist(), q.tolist())) == sorted(zip(found[1].tolist(), found[2].tolist())), what
    r, t, x = ch.records(ch.rule)
    assert sorted(zip(r.tolist(), t.tolist(), x.tolist())) == fired, what
    return got, (q, o, r, t, x)


def test_device_chains_on_two_streams(case):
    """two chains at once on two created streams, the whole corpus and its 300-text slice, each with buffers of its
    own; from buffers full of 0xA5, 0x00 and 0xFF, and once more over what the last run left"""
    g = case.g
    a = case.automaton()
    m = Matcher(a, 0, max_text=case.corpus.N)
    assert m.set_mode("sparse") == "sparse"
    rig = streams.Rig()
    small = expected_of(g.db, case.small_texts)
    assert small[1]["windowed"] >= 2049 and small[1]["matches"] > 500
    try:
        big, lil = DeviceChain(rig, m, g.texts), DeviceChain(rig, m, case.small_texts)
        runs = []
        for fill in (0xA5, 0x00, 0xFF, None):
            if fill is not None:
                big.poison(fill)
                lil.poison(fill)
                rig.sync(None)
            big.enqueue()
            lil.enqueue()
            got, recs = check_chain(big, case.counts, case.found, case.fired, "corpus, fill %s" % fill)
            check_chain(lil, small[1], small[2], small[3], "slice, fill %s" % fill)
            runs.append(recs)
        print("record counts along the chain (the count cell of every pass's output):", got)
        for r in runs[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))
        # ... and bit for bit what Matcher.scan_sequences and scan_rules return, in their order (the pipelines
        # agree: test_the_pipelines_agree_bit_for_bit); scan_sequences adds the last part's post context
        q, o, r, t, x = runs[0]
        post = np.array([parts[-1].post for parts, _ in g.db.sigs], dtype=np.int64)
        go, gq, gr, gt, gx = pipeline_run(case, "sparse")["records"]
        assert np.array_equal(gq, q) and np.array_equal(go.astype(np.int64), o + post[q])
        assert np.array_equal(gr, r) and np.array_equal(gt, t) and np.array_equal(gx.astype(np.int64), x)
    finally:
        rig.close()
        m.close()
        a.close()


def folded_models(a, g):
    """the models' view of the automaton the upload makes: a window counts from a pattern's first position and a
    gap between full spans, so a pattern is pre + anchor bytes long and every gap grows by the post context of the
    part in front (include/acmatch.h, "How the other per-pattern rules see a wildcard pattern")"""
    pats, seqs, windows = [], [], {}
    for q, (parts, gaps) in enumerate(g.db.sigs):
        seqs.append((list(range(len(pats), len(pats) + len(parts))),
                     [(lo + parts[j].post, None if hi is None else hi + parts[j].post) for j, (lo, hi) in enumerate(gaps)]))
        for j, p in enumerate(parts):
            if (q, j) in g.windows:
                windows[len(pats)] = g.windows[q, j]
            pats.append(wm.Pattern(p.sets, p.nocase))
    for i, p in enumerate(pats):
        assert a.pattern(i)[0].upper() == p.anchor.upper() and a.wildcard_lengths(i) == (p.pre, p.post)
    return (wm.WildcardModel(pats), pm.Windows([b"." * (p.pre + p.L) for p in pats], windows),
            sm.SequenceModel([p.pre + p.L for p in pats], seqs),
            rm.RuleModel(len(seqs), [(ops, g.lines[r].split(";")[0]) for r, (ops, _) in enumerate(g.db.rules)]))


def test_a_starved_middle_plane(case):
    """the case pass's output planes hold fewer cells than it has records: their count cell says how many there
    were, every pass behind works on the records that fit, and nothing is written behind any plane"""
    g = case.g
    a = case.automaton()
    m = Matcher(a, 0, max_text=case.corpus.N)
    rig = streams.Rig()
    try:
        K = 4099
        ch = DeviceChain(rig, m, case.small_texts, starve=K)
        ch.poison(0xA5)
        rig.sync(None)
        ch.enqueue()
        ch.check_guards("starved")
        _, counts, _, _ = expected_of(g.db, case.small_texts)
        assert int(ch.all[0].cells(1, ch.s)[0]) == counts["anchors"] > K - 2
        cells, offs = (p.cells(K, ch.s) for p in ch.all)
        assert cells[K - 1] == offs[K - 1]                               # the trailer: the scan's final state
        cells, offs = cells[1:K - 1].astype(np.int64), offs[1:K - 1].astype(np.int64)
        wmodel, windows, smodel, rmodel = folded_models(a, g)
        t, starts = Matcher.pack_segments(case.small_texts)
        starts = starts.tolist()
        wp, wo, und = wmodel.filter(cells, offs, wm.HEAD, True, t, starts=starts, lead_begin=0, open_end=int(t.size))
        pp, po, _ = windows.entries(wp, wo, True, starts, 0, int(t.size), int(t.size))
        sq, sof, sinfo = smodel.run(pp, po, starts, 0)
        rr, rt, ro, rinfo = rmodel.run(sq, sof, starts)
        got = ch.counts()
        assert (got["wild"], got["pos"], got["seq"], got["rule"]) == (len(wp), len(pp), len(sq), len(rr)), got
        assert und == 0 and len(wp) > len(pp) > len(sq) > len(rr) > 0
        q, o = ch.records(ch.seq)
        assert np.array_equal(q, sq) and np.array_equal(o, sof)
        r, x, o = ch.records(ch.rule)
        assert np.array_equal(r, rr) and np.array_equal(x, rt) and np.array_equal(o, ro)
        assert ch.info[2].cells(4, ch.s).tolist() == sinfo and ch.info[3].cells(4, ch.s).tolist() == rinfo
    finally:
        rig.close()
        m.close()
        a.close()
