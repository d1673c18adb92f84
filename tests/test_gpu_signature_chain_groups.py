"""Groups, (aabb|ccdd) and !(aabb|ccdd), through the signature chain and at table scale.

1. The whole chain on a second generated database, smaller than that of test_gpu_signature_chain.py, in which
   nearly half the parts carry a group (signature_oracle.make(group_share=...)): positive and negated, of every
   width and count the word-wise compare distinguishes, at a part's first and last positions, next to the anchor
   on either side, two adjacent ones, beside nocase anchors, windows and every gap form; a corpus in which every
   signature is planted and every signature with a group has a near miss that only its groups refuse.  Through
   Matcher.scan_sequences / scan_rules under both scan pipelines, on a piece whose seam with the bytes in front
   cuts a group, and through every pass enqueued on a created stream the way acm_grep enqueues them; against
   tests/signature_oracle.py, which states groups on bytes: exact equality of the records and of the per-pass
   record counts, with the groups on and (the oracle alone) off.
2. Group tables past 16 bits: a set of 4 097 * 16 groups, whose last pattern's groups are numbered from 0x10000,
   and a set whose string pool is longer than 0x10000 words; both built by per-call adds, run through
   acm_wildcard_matches_async in its three forms from poisoned buffers (run_pass of test_gpu_wildcards.py) and
   through Matcher.scan_wildcards, against wildcard_model.brute_force.
"""
import re
import time

import numpy as np
import pytest

import group_model as gm
import signature_oracle as so
import streams
import wildcard_model as wm
from gpu_pattern_matching_amd import Automaton, Matcher, _lib
from test_gpu_groups import all_forms, both_pipelines
from test_gpu_signature_chain import SEED, Case, DeviceChain, check_chain, expected_of, matcher_for, pipeline_run, seq_tuples

pytestmark = pytest.mark.gpu

GROUP_MAKE = dict(rules=40, texts=1800, total=110 * 1024, empties=1200, long_text=9000, group_share=0.45)


class GroupCase(Case):
    """the generated database with groups, what the oracle says of it, and what it says with the groups as ??"""

    def __init__(self):
        super().__init__(lambda: so.make(SEED, **GROUP_MAKE), groups=True)
        t0 = time.perf_counter()
        self.loose_counts = {}
        self.loose = so.sequences(self.g.db, self.corpus, counts=self.loose_counts, groups=False)
        self.loose_fired = so.rules(self.g.db, self.corpus, self.loose)
        self.loose_seconds = time.perf_counter() - t0


@pytest.fixture(scope="module")
def case(gpu):
    return GroupCase()


def group_parts(db):
    """(signature, part index, part) of every part with a group"""
    return [(q, j, p) for q, (parts, _) in enumerate(db.sigs) for j, p in enumerate(parts) if p.groups]


def test_the_input_is_worth_running(case):
    """from the oracle alone"""
    g, c, counts, loose = case.g, case.corpus, case.counts, case.loose_counts
    print("generator and oracle: %.1f s, the oracle once more without groups: %.1f s; stage counts %s, without groups %s, "
          "rule records %d (without groups %d), (rule, text) pairs %d" % (case.seconds, case.loose_seconds, counts, loose,
                                                                         len(case.fired), len(case.loose_fired), case.pairs))
    nsig = len(g.db.sigs)
    parts = sum(len(p) for p, _ in g.db.sigs)
    lens = np.array([len(t) for t in g.texts])
    print("%d rules, %d signatures, %d parts, %d of them with %d groups; %d texts, %d bytes" % (
        len(g.db.rules), nsig, parts, len(group_parts(g.db)), sum(len(p.groups) for _, _, p in group_parts(g.db)), lens.size, lens.sum()))
    assert lens.sum() <= 204 * 1024 and lens.size <= 3000                 # no larger than the corpus without groups
    # every kind of group
    kinds = set()
    for q, j, p in group_parts(g.db):
        for i, (at, strings, neg) in enumerate(p.groups):
            w = len(strings[0])
            kinds |= {"negated" if neg else "positive", "width %d" % w, "strings %d" % len(strings)}
            kinds |= {"first"} if at == 0 else set()
            kinds |= {"last"} if at + w == p.n else set()
            kinds |= {"in front of the anchor"} if at + w == p.at else set()
            kinds |= {"behind the anchor"} if at == p.at + p.L else set()
            kinds |= {"adjacent"} if i and p.groups[i - 1][0] + len(p.groups[i - 1][1][0]) == at else set()
            kinds |= {"negated, one string"} if neg and len(strings) == 1 else set()
    want = {"negated", "positive", "first", "last", "in front of the anchor", "behind the anchor", "adjacent", "negated, one string",
            "strings 255", "strings 256", "width 31", "width 32"} | {"width %d" % w for w in so.GROUP_WIDTHS} | \
        {"strings %d" % n for n in range(2, 9)}
    assert want <= kinds, sorted(want - kinds)
    assert re.search(r"(?<!!)\((?:[0-9a-f]{2}){2,}\)", "".join(g.lines))  # a non-negated group of one string: exact bytes
    # where the sets of a part with a group hold, the groups keep at least a fifth and drop at least a fifth
    held, kept = so.group_decisions(g.db, c)
    print("occurrences of the parts with a group: %d by their sets, %d kept by the groups" % (held, kept))
    assert kept >= held / 5 and held - kept >= held / 5 and held > 2049
    assert loose["parts"] - counts["parts"] == held - kept and loose["anchors"] == counts["anchors"]
    assert min(counts["parts"], counts["windowed"]) >= 2049 and counts["matches"] > 500
    # the groups decide matches and rules
    on, off = set(seq_tuples(case.found)), set(seq_tuples(case.loose))
    assert on < off
    assert set(case.found[2].tolist()) == set(range(nsig))                # every signature holds somewhere
    fired, loose_fired = {(r, t) for r, t, _ in case.fired}, {(r, t) for r, t, _ in case.loose_fired}
    print("(rule, text) verdicts the groups turn: %d to false, %d to true" % (len(loose_fired - fired), len(fired - loose_fired)))
    assert fired != loose_fired and len(fired ^ loose_fired) >= 10
    # a nocase signature with a group whose planted occurrence has its anchor in the other case
    with_group = {q for q, _, _ in group_parts(g.db)}
    cased = so.sequences(g.db, c, nocase=False)
    n_on, n_off = np.bincount(case.found[2], minlength=nsig), np.bincount(cased[2], minlength=nsig)
    assert any(g.nocase[q] and n_on[q] > n_off[q] for q in with_group)
    # a window on a part whose first position lies in a group, and it decides
    on_group = [(q, j) for (q, j) in g.windows if g.db.sigs[q][0][j].groups and g.db.sigs[q][0][j].groups[0][0] == 0]
    assert on_group
    free = np.bincount(so.sequences(g.db, c, windows=False)[2], minlength=nsig)
    assert any(free[q] > n_on[q] for q, _ in on_group)
    # gaps counted from and to a span's edge that is a group
    assert any(j > 0 and p.groups[0][0] == 0 for _, j, p in group_parts(g.db))
    assert any(j + 1 < len(g.db.sigs[q][0]) and p.groups[-1][0] + len(p.groups[-1][1][0]) == p.n for q, j, p in group_parts(g.db))


@pytest.mark.parametrize("name", ["sparse", "chain"])
def test_scan_sequences_and_rules(case, name):
    g = case.g
    run = pipeline_run(case, name)
    assert run["path"] == name
    go, gq, r, t, o = run["records"]
    got = sorted(zip(go.tolist(), gq.tolist()))
    want = seq_tuples(case.found)
    assert got == want, (len(got), len(want), sorted(set(got) ^ set(want))[:6])
    assert run["info"][0] == case.counts["windowed"] < case.loose_counts["windowed"]
    assert sorted(zip(r.tolist(), t.tolist(), o.tolist())) == case.fired
    assert run["rinfo"][2] == case.pairs and run["rinfo"][0] <= case.counts["matches"]
    # one text alone: the long one
    _, counts, found, fired = expected_of(g.db, [max(g.texts, key=len)])
    lo, lq, lr, lt, lx = run["long"]
    assert sorted(zip(lo.tolist(), lq.tolist())) == seq_tuples(found) and counts["matches"] > 50
    assert sorted(zip(lr.tolist(), (lt + 1).tolist(), lx.tolist())) == fired and (lt == -1).all() and len(fired) > 5


def test_the_pipelines_agree_bit_for_bit(case):
    x, y = pipeline_run(case, "sparse"), pipeline_run(case, "chain")
    for u, v in zip(x["records"] + x["long"], y["records"] + y["long"]):
        assert np.array_equal(u, v)
    assert x["info"] == y["info"] and x["rinfo"] == y["rinfo"]


def seam_in_a_group(db, text):
    """(cut, matches): a cut of the text inside a group, one byte behind the group's first, such that this byte,
    the last in front of the seam, decides a match of a scan that begins at the cut, and decides it through a
    group: with another byte there the oracle finds other matches, and with the groups off the same.  The group
    is one in front of the anchor of a first part, so the anchor begins behind the cut and the part is a record
    of that scan.  From the oracle's occurrences alone."""
    c = so.Corpus([text])
    for q, (parts, _) in enumerate(db.sigs):
        p = parts[0]
        for at, strings, _ in p.groups:
            if at + len(strings[0]) > p.at:
                continue
            for k in so.occurrences(c, p.tables(), p.groups).tolist()[:4]:
                cut = k + at + 1
                other = text[:cut - 1] + bytes([text[cut - 1] ^ 0x40]) + text[cut:]
                on = [seq_tuples(so.sequences(db, [t], anchors_from=cut)) for t in (text, other)]
                off = [seq_tuples(so.sequences(db, [t], anchors_from=cut, groups=False)) for t in (text, other)]
                if on[0] != on[1] and off[0] == off[1] and 1000 < cut < len(text) - 1000:
                    return cut, sorted(set(on[0]) - set(on[1]))
    return None


@pytest.mark.parametrize("name", ["sparse", "chain"])
def test_a_piece_with_the_bytes_in_front(case, name):
    """the database without its windows over the first 16 KiB of the corpus as one text, cut in two inside a group that decides
    a match: the second piece through scan_sequences and scan_rules with the first as `before`.  The group's first
    byte is the last byte of `before`, its others the first of the text."""
    g = case.g
    db = so.Database(g.lines, g.nocase, groups=True)
    long_one = b"".join(g.texts)[:16384]
    seam = seam_in_a_group(db, long_one)
    assert seam is not None
    cut, decided = seam
    a = case.automaton(windows={}, extra=None if name == "sparse" else b"a")
    assert not a.positioned and a.has_groups
    piece = long_one[cut:]
    m = matcher_for(a, name, len(long_one))
    go, gq, _, _ = m.scan_sequences(piece, before=long_one[:cut], lead_begin=-cut)
    assert m.path_taken(len(piece)) == name
    found = so.sequences(db, [long_one], anchors_from=cut)
    got = sorted(zip((go.astype(np.int64) + cut).tolist(), gq.tolist()))
    assert got == seq_tuples(found) and found[0].size > 30
    assert decided and set(decided) <= set(got)                          # the matches whose group the seam cuts
    assert set(got) < set(seq_tuples(so.sequences(db, [long_one], anchors_from=cut, groups=False)))
    alone = so.sequences(db, [piece])
    assert set(seq_tuples(found)) - {(e + cut, s) for e, s in seq_tuples(alone)}
    r, t, o, rinfo = m.scan_rules(piece, before=long_one[:cut], lead_begin=-cut)
    fired = so.rules(db, [long_one], found)
    assert sorted(zip(r.tolist(), (t + 1).tolist(), (o.astype(np.int64) + cut).tolist())) == fired and (t == -1).all()
    assert len(fired) > 3 and rinfo.tolist()[0] == found[0].size
    m.close()
    a.close()


def test_device_chains_on_two_streams(case):
    """two chains at once on two created streams, the whole corpus and its 300-text slice, each with buffers of its
    own; from buffers full of 0xA5, 0x00 and 0xFF, and once more over what the last run left.  The wildcard pass
    keeps what the oracle's parts are with the groups on: fewer than with the groups as ??."""
    g = case.g
    a = case.automaton()
    assert a.has_groups
    m = Matcher(a, 0, max_text=case.corpus.N)
    assert m.set_mode("sparse") == "sparse"
    rig = streams.Rig()
    small = expected_of(g.db, case.small_texts)
    small_loose = {}
    so.sequences(g.db, small[0], counts=small_loose, groups=False)
    assert small[1]["parts"] >= 1025 and small[1]["matches"] > 100 and small_loose["parts"] > small[1]["parts"]
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
            lil_got, _ = check_chain(lil, small[1], small[2], small[3], "slice, fill %s" % fill)
            assert got["wild"] == case.counts["parts"] < case.loose_counts["parts"]
            assert lil_got["wild"] == small[1]["parts"] < small_loose["parts"]
            runs.append(recs)
        print("record counts along the chain (the count cell of every pass's output):", got)
        for r in runs[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))
        q, o, r, t, x = runs[0]
        post = np.array([parts[-1].post for parts, _ in g.db.sigs], dtype=np.int64)
        go, gq, gr, gt, gx = pipeline_run(case, "sparse")["records"]
        assert np.array_equal(gq, q) and np.array_equal(go.astype(np.int64), o + post[q])
        assert np.array_equal(gr, r) and np.array_equal(gt, t) and np.array_equal(gx.astype(np.int64), x)
    finally:
        rig.close()
        m.close()
        a.close()


# ------------------------------------------------------------------ 2. group tables past 65 535

ANY = wm.FULL
MANY, PER = 4097, 16                     # patterns, groups of each: the last pattern's groups are 0x10000 .. 0x1000F
PLANTED = [0, 1, 4095, 4096]             # (4095: groups 0xFFF0 .. 0xFFFF; 4096, the last: from 0x10000)


def many_strings(i, k):
    """the two strings of group k of pattern i: no other pattern has either at that k, whatever of i is cut off"""
    return [bytes([(7 * i + k) & 0xFF, 0x80 | i >> 8]), bytes([0xFF - k, 0x40 | (i ^ i >> 8) & 0x3F])]


class Laid(gm.Pattern):
    """gm.Pattern for an anchor with nothing but full sets behind it, its fields written down (thousands are built,
    and the constructor walks 256 values per full set); the planted ones are compared with the constructor's"""

    def __init__(self, anchor, tail, groups):
        self.positions = [frozenset((b,)) for b in anchor] + [ANY] * tail
        self.nocase, self.at, self.L, self.pre, self.post, self.anchor = False, 0, len(anchor), 0, tail, bytes(anchor)
        self.groups = [(at, [bytes(x) for x in strings], bool(neg)) for at, strings, neg in groups]

    def same_as_built(self):
        b = gm.Pattern(self.positions, self.groups)
        return all(getattr(b, k) == getattr(self, k) for k in ("positions", "nocase", "at", "L", "pre", "post", "anchor", "groups"))


def many_pattern(i):
    return Laid(b"%04x" % i, 2 * PER, [(4 + 2 * k, many_strings(i, k), False) for k in range(PER)])


def many_text():
    """for each planted pattern: its anchor with all sixteen groups holding (their strings in turn), with only the
    sixteenth failing (in its last byte), with only the first failing; and for pattern 4096 the bytes that would
    hold for pattern 0, whose groups are numbered 4096's modulo 0x10000"""
    out = bytearray(b"....")
    for i in PLANTED:
        good = [many_strings(i, k)[k & 1] for k in range(PER)]
        last_wrong = good[:-1] + [good[-1][:1] + bytes([good[-1][1] ^ 1])]
        first_wrong = [bytes([good[0][0] ^ 1]) + good[0][1:]] + good[1:]
        for strings in (good, last_wrong, first_wrong):
            out += b"%04x" % i + b"".join(strings) + b".."
    out += b"%04x" % 4096 + b"".join(many_strings(0, k)[k & 1] for k in range(PER)) + b".."
    # under one group the first string of the group behind it in the table (a group has two strings, and the
    # compare takes four a step): group 4's under group 3 of pattern 0, and under the last group of pattern 4095,
    # number 0xFFFF, that of group 0x10000
    for i, k, nxt in ((0, 3, many_strings(0, 4)[0]), (4095, PER - 1, many_strings(4096, 0)[0])):
        assert nxt not in many_strings(i, k)
        out += b"%04x" % i + b"".join(nxt if j == k else many_strings(i, j)[j & 1] for j in range(PER)) + b".."
    return bytes(out)


FULL_SET = Automaton.byte_set(ANY)


def add_all(pats):
    """acm_automaton_add_wildcard_groups pattern by pattern, as Automaton.add_wildcard calls it"""
    a = Automaton()
    for i, p in enumerate(pats):
        sets = b"".join(Automaton.byte_set(min(s)) for s in p.positions[:p.L]) + FULL_SET * p.post
        raw = [b"".join(strings) for _, strings, _ in p.groups]
        arr = (_lib.WildGroup * len(raw))(*[_lib.WildGroup(at, len(strings[0]), len(strings), int(neg), raw[k])
                                            for k, (at, strings, neg) in enumerate(p.groups)])
        assert a.lib.acm_automaton_add_wildcard_groups(a.h, sets, len(p.positions), arr, len(raw), i, 0) == i
    a.compile()
    assert a.has_groups
    return a


def check_set(pats, planted, text, expect):
    """the set through the pass in its three forms and through scan_wildcards under both pipelines, against brute
    force over the planted patterns (no other pattern's anchor is in the text)"""
    assert all(bytes(p.anchor) not in text for i, p in enumerate(pats) if i not in planted)
    want = {(o, planted[k]) for o, k in wm.brute_force([pats[i] for i in planted], [text])}
    assert sorted(p for _, p in want) == expect, sorted(want)
    a = add_all(pats)
    for i in planted:
        assert a.wildcard_groups(i) == pats[i].groups and a.wildcard_lengths(i) == (0, pats[i].post) and pats[i].same_as_built()
    model = gm.GroupModel(pats)
    m = Matcher(a, 0, max_text=4096)
    try:
        kept, und = all_forms(m, model, text, aligns=(0, 3), open_end=len(text))
        assert und == 0 and kept == want
        for mode in both_pipelines(m):
            go, gp, _, info = m.scan_wildcards(text, all_patterns=True)
            assert set(zip(go.tolist(), gp.tolist())) == want and go.size == len(want) and info[0] == 0, mode
    finally:
        m.close()
        a.close()


def test_more_than_65535_groups(gpu):
    t0 = time.perf_counter()
    pats = [many_pattern(i) for i in range(MANY)]
    assert (MANY - 1) * PER == 0x10000 and 4095 * PER + PER - 1 == 0xFFFF
    text = many_text()
    print("%d groups, a text of %d bytes; patterns built in %.2f s" % (MANY * PER, len(text), time.perf_counter() - t0))
    check_set(pats, PLANTED, text, PLANTED)                              # one occurrence of each holds, the others do not


POOL_W, POOL_N = 32, 256                 # a group of 256 strings of 32 bytes: 2048 words of the pool
POOL_GROUPS = 34                         # the last one's strings begin at word 33 * 2048 = 0x10800


def pool_strings(g):
    rng = np.random.default_rng(900 + g)
    out = []
    while len(out) < POOL_N:
        s = bytes(rng.integers(1, 256, size=POOL_W, dtype=np.uint8))
        if s not in out:
            out.append(s)
    return out


def test_a_pool_past_65535_words(gpu):
    """one group per pattern; the strings of group g begin at word 2048 * g"""
    words = POOL_N * (POOL_W // 4)
    assert (POOL_GROUPS - 1) * words > 0x10000 > (POOL_GROUPS - 3) * words
    strings = [pool_strings(g) for g in range(POOL_GROUPS)]
    pats = [Laid(b"p%03d" % g, POOL_W, [(4, strings[g], bool(g % 3 == 1))]) for g in range(POOL_GROUPS)]
    last = POOL_GROUPS - 1
    assert not pats[0].groups[0][2] and not pats[last].groups[0][2] and pats[1].groups[0][2]
    planted = [0, 1, last - 1, last]
    flip = lambda s, at: s[:at] + bytes([s[at] ^ 0x10]) + s[at + 1:]
    text = b"...." + b"..".join([
        b"p000" + strings[0][-1],                                         # the last string of the first group
        b"p%03d" % last + strings[last][0], b"p%03d" % last + strings[last][-1],     # the first and the last of the last group
        b"p%03d" % last + flip(strings[last][-1], POOL_W - 1),            # near misses: the last word only,
        b"p%03d" % last + flip(strings[last][0], POOL_W - 4), b"p000" + flip(strings[0][-1], POOL_W - 2),
        b"p%03d" % last + flip(strings[last][100], 0),                    # ... the first word only,
        b"p%03d" % last + strings[(last * words & 0xFFFF) // words][0],   # the group at the word index modulo 0x10000,
        b"p%03d" % last + strings[last - 1][-1], b"p%03d" % (last - 1) + strings[last - 1][-1],   # the group in front: its own pattern
        b"p001" + strings[1][7], b"p001" + flip(strings[1][7], POOL_W - 1), b"p001" + strings[0][-1]]) + b"...."   # negated
    assert (last * words & 0xFFFF) // words == 1
    check_set(pats, planted, text, [0, 1, 1, last - 1, last, last])
