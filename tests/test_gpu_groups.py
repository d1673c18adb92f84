"""Groups of wildcard patterns on the device (acm_wildcard_matches_async over an automaton with groups,
Matcher.scan_wildcards, scan_sequences and scan_rules over bodies with multi-byte alternatives), cell for cell
against the model of tests/group_model.py: every width at which the word-wise compare changes shape with one to
256 strings, negated and not, zero and non-zero bytes behind a group; groups in front of, behind and next to the
anchor, sixteen of them, adjacent ones; spans at the borders of a text, of the bytes given and across the seam of
`before` and text; state cells, pattern cells and cells that are neither; sequences, windows and rules over such
bodies; a seeded database.  Every call of the pass starts from poisoned outputs, workspace and text surroundings
and checks the guard cells (run_pass of tests/test_gpu_wildcards.py)."""
import numpy as np
import pytest

import group_model as gm
import wildcard_model as wm
from gpu_pattern_matching_amd import Automaton, Matcher
from test_gpu_wildcards import FORMS, INT32_MAX, NO_CELL, entries_of, random_texts, run_pass, upload
from test_host_groups import random_body

pytestmark = pytest.mark.gpu

ANY = wm.FULL
a_, b_, c_ = 0x61, 0x62, 0x63
A, B = 0x41, 0x42
WIDTHS = [2, 3, 4, 5, 8, 31, 32]
COUNTS = [1, 2, 255, 256]
X = 0x78


def build(pats, max_text=8192):
    """(automaton, model, matcher) of gm.Patterns added with their groups"""
    a = Automaton()
    for i, p in enumerate(pats):
        assert a.add_wildcard(p.positions, i, nocase=p.nocase, groups=p.groups) == i
        assert a.wildcard_groups(i) == p.groups and a.wildcard_lengths(i) == (p.pre, p.post)
    a.compile()
    assert a.has_groups and a.has_wildcards
    return a, gm.GroupModel(pats), Matcher(a, 0, max_text=max_text)


def cells_of(model, text, report, origin=0):
    if report == wm.STATE:
        states, offs, _ = model.walk(text)
        return states, offs + origin
    return entries_of(model, text, origin)


def all_forms(m, model, text, aligns=(0,), **kw):
    """the pass in its three forms; returns (model's kept entries, entries the groups alone dropped) of the all form"""
    out = None
    for report, all_patterns in FORMS:
        cells, offs = cells_of(model, text, report, kw.get("origin", 0))
        planes = upload(cells, offs)
        for align in aligns:
            ep, eo, und, _ = run_pass(m, model, planes, cells, offs, report, all_patterns, text, align=align, **kw)
        if report == wm.HEAD:
            out = set(zip(eo.tolist(), ep.tolist())), und
        for x in planes:
            x.free()
    return out


def both_pipelines(m):
    yield m.set_mode("chain")
    if m.sparse_eligible():
        assert m.set_mode("sparse") == "sparse"
        yield "sparse"
    m.set_mode("auto")


# ------------------------------------------------------------------ 1. widths and counts

def strings_of(w, count):
    """count distinct strings of w bytes: the first half differ from xx..x in the last byte only, the second in the
    first byte only"""
    base = bytes([X]) * w
    return [base[:-1] + bytes([i]) if i < 128 else bytes([i]) + base[1:] for i in range(count)]


def width_set():
    """every (width, count, negated) as a group behind the one anchor AB: a state with 56 entries"""
    return [gm.Pattern([A, B] + [ANY] * w, [(2, strings_of(w, n), neg)]) for w in WIDTHS for n in COUNTS for neg in (False, True)]


def width_text():
    """AB, w bytes, one byte behind them: strings of the groups and near misses, the byte behind once 0 and once not"""
    out = bytearray(b"..")
    for w in WIDTHS:
        base = bytes([X]) * w
        cands = [strings_of(w, 256)[k] for k in (0, 1, 2, 127, 128, 254, 255)]
        cands += [base[:-1] + b"\xf0", b"\xf0" + base[1:], base, bytes([0]) + base[1:-1] + bytes([1]) if w > 2 else b"\x00\x01",
                  base[:w // 2] + b"\x00" + base[w // 2 + 1:], bytes(w)]
        for cand in cands:
            assert len(cand) == w
            for tail in (b"\x00", b"\xff", bytes([X])):
                out += b"AB" + cand + tail + b"."
    return bytes(out) + b"AB"                                        # (and an anchor whose group leaves the text)


def test_widths_and_counts(gpu):
    pats = width_set()
    a, model, m = build(pats, max_text=16384)
    text = width_text()
    states, offs, _ = model.walk(text)
    assert int(model.list_len[states].max()) == len(pats) >= 40      # verdict bits beyond the 32 a row carries
    kept, und = all_forms(m, model, text, aligns=(0, 1), open_end=len(text))
    assert und == 0
    by_pattern = {i: sum(1 for _, p in kept if p == i) for i in range(len(pats))}
    n_occ = text.count(b"AB") - 1
    assert all(0 < by_pattern[i] < n_occ for i in range(len(pats))), by_pattern      # every group keeps and drops
    assert kept == wm.brute_force(pats, [text])
    # the end withheld: the last anchor's group is not in the bytes given
    _, und = all_forms(m, model, text, open_end=None)
    assert und == len(pats)
    for mode in both_pipelines(m):
        go, gp, _, info = m.scan_wildcards(text, all_patterns=True)
        assert set(zip(go.tolist(), gp.tolist())) == kept and go.size == len(kept) and info[0] == 0, mode
    m.close()


# ------------------------------------------------------------------ 2. placement

AB_, BC_, CA_ = b"ab", b"bc", b"ca"
PLACED = [gm.Pattern([ANY, ANY, a_, b_], [(0, [AB_, BC_], False)]),                        # 0: in the pre context, first positions
          gm.Pattern([a_, b_, ANY, ANY], [(2, [AB_, BC_], True)]),                         # 1: in the post context, last positions
          gm.Pattern([ANY, ANY, ANY, c_, a_, ANY, ANY], [(0, [b"abc", b"bca", b"cab"], False), (5, [CA_], True)]),   # 2: both, touching
          gm.Pattern([ANY, ANY, {a_, b_}, b_, c_, {b_, c_}, ANY, ANY, ANY],
                     [(0, [AB_, CA_], True), (6, [b"aaa", b"abc", b"ccc", b"cab"], False)]),                     # 3: both, apart
          gm.Pattern([b_, a_, ANY, ANY, ANY, ANY], [(2, [AB_, BC_, CA_], False), (4, [b"aa", b"bb", b"cc"], True)]),   # 4: adjacent
          gm.Pattern([c_, c_] + [ANY] * 32, [(2 + 2 * k, [b"aa", b"ab", b"ba", b"bb", b"ac", b"ca", b"cb", b"bc"], False)
                                              for k in range(16)]),                        # 5: sixteen groups
          gm.Pattern([ANY, ANY, ANY, ANY, ANY, a_, c_], [(1, [b"abca", b"bcab", b"aaaa", b"cccc", b"acac"], True)]),   # 6: a ?? in front
          gm.Pattern([a_, a_, ANY], []),                                                   # 7: no group, a context
          gm.Pattern([b_, b_], [])]                                                        # 8: plain


def test_placement(gpu):
    a, model, m = build(PLACED)
    rng = np.random.default_rng(12)
    text = bytes(rng.choice(np.array([a_, b_, c_], dtype=np.uint8), size=2600))
    # (pattern 5 wants sixteen pairs without "cc": plant some that hold and some with one pair wrong)
    good = b"cc" + b"abbaacca" * 4
    text = text[:500] + good + text[500:900] + good[:20] + b"cc" + good[22:] + text[900:1500] + good[:-1] + b"c" + text[1500:]
    cells, offs = entries_of(model, text)
    full = bytes(text)
    ctx = [model.context_verdict(int(p), int(o), 0, len(full), True, full, 0) == wm.KEEP for p, o in zip(cells, offs)]
    kept, und = all_forms(m, model, text, aligns=range(4), open_end=len(text))
    assert und == 0 and kept == wm.brute_force(PLACED, [text])
    decided = {i: [0, 0] for i in range(7)}
    for p, o, c in zip(cells.tolist(), offs.tolist(), ctx):
        if c and p < 7:
            decided[p][(o, p) in kept] += 1
    assert all(min(v) >= 1 for v in decided.values()) and sum(v[0] for v in decided.values()) >= 50 \
        and sum(v[1] for v in decided.values()) >= 50, decided
    for mode in both_pipelines(m):
        go, gp, _, info = m.scan_wildcards(text, all_patterns=True)
        assert set(zip(go.tolist(), gp.tolist())) == kept and info[0] == 0, mode
        fo, fp, _, _ = m.scan_wildcards(text)
        assert np.array_equal(fo, np.unique(go)), mode
    m.close()


# ------------------------------------------------------------------ 3. spans at the borders

EDGE = [gm.Pattern([ANY, ANY, b_, b_], [(0, [b"cx", b"xc"], False)]),      # 0: the group reaches in front
        gm.Pattern([b_, b_, ANY, ANY], [(2, [b"cb", b"bb"], False)]),      # 1: ... behind
        gm.Pattern([ANY, ANY, ANY, b_, b_], [(0, [b"cxc"], True)])]        # 2: three in front, negated


def test_span_rules_by_hand(gpu):
    a, model, m = build(EDGE)
    text = b"cxbbcbbbb"                                                   # bb ends at 3, 6, 7, 8
    cells, offs = entries_of(model, text)
    planes = upload(cells, offs)

    def got(t=text, c=cells, o=offs, pl=planes, **kw):
        ep, eo, und, _ = run_pass(m, model, pl, c, o, wm.HEAD, True, t, **kw)
        return sorted(zip(eo.tolist(), ep.tolist())), und
    recs, und = got(open_end=9)
    # 0: "cx" in front of bb at 2; 1: "cb" behind bb at 2..3, "bb" behind bb at 5..6; 2: bbc, bcb, cbb in front are not
    # "cxc", and in front of bb at 2 there are only two bytes
    assert und == 0 and recs == [(3, 0), (3, 1), (6, 1), (6, 2), (7, 2), (8, 2)]
    # Tend: the group of 1 behind bb at 6..7 would need the byte at 9
    assert (7, 1) not in recs
    # the end withheld: it is undecided, and so is the one behind bb at 7..8
    recs, und = got(open_end=None)
    assert und == 2 and (6, 1) in recs
    # a text that starts at 1: the groups that reach in front of it drop, whatever lies there
    recs, und = got(open_end=9, starts=[0, 1])
    assert und == 0 and (3, 0) not in recs and (3, 1) in recs
    # texts [0, 5) and [5, 9): behind bb at 2..3 only "c" is left of its text
    recs, und = got(open_end=9, starts=[0, 5])
    assert und == 0 and (3, 1) not in recs and (3, 0) in recs and (6, 2) not in recs and (8, 2) not in recs
    # the piece [1, 9) alone: the group's first byte is not given -- undecided; with it as `before`, across the seam, decided
    c2, o2 = entries_of(model, text[1:], 1)
    p2 = upload(c2, o2)
    recs, und = got(text[1:], c2, o2, p2, origin=1, open_end=9)
    assert und == 1 and (3, 0) not in recs and (3, 1) in recs
    for before, want in ((b"c", True), (b"b", False), (b"qc", True)):
        recs, und = got(text[1:], c2, o2, p2, origin=1, open_end=9, before=before)
        assert und == 0 and ((3, 0) in recs) == want, before
    # the seam inside a group, byte by byte: "cxcbb", bb ends at 4; 2 is dropped iff the three bytes in front are
    # "cxc", 0 is kept iff the two in front are "xc"
    t2 = b"cxcbb"
    for cut, before, want in ((1, b"c", [(4, 0)]), (1, b"q", [(4, 0), (4, 2)]), (1, b"\x00", [(4, 0), (4, 2)]),
                              (2, b"cx", [(4, 0)]), (2, b"qx", [(4, 0), (4, 2)]), (2, b"cq", [(4, 2)]), (2, b"c\x00", [(4, 2)]),
                              (2, b"zzcx", [(4, 0)])):
        c3, o3 = entries_of(model, t2[cut:], cut)
        p3 = upload(c3, o3)
        for align in range(4):
            recs, und = got(t2[cut:], c3, o3, p3, origin=cut, open_end=5, before=before, align=align)
            assert und == 0 and recs == want, (cut, before, align)
        for x in p3:
            x.free()
    for x in planes + p2:
        x.free()
    m.close()


def test_borders_swept_and_hostile_cells(gpu):
    a, model, m = build(PLACED)
    rng = np.random.default_rng(31)
    text = rng.choice(np.array([a_, b_, c_], dtype=np.uint8), size=400)
    T = text.size
    unds = set()
    for kw in (dict(open_end=T), dict(open_end=None), dict(open_end=T + 5), dict(open_end=T, lead_begin=3),
               dict(open_end=None, starts=[0, 50, 50, 120, T - 2]),
               dict(open_end=T, starts=[30, 31, 33, T, T + 7, INT32_MAX], lead_begin=-3)):
        _, und = all_forms(m, model, text, **kw)
        unds.add(und > 0)
    assert unds == {False, True}
    piece = text[100:]
    prev = None
    for nb in (0, 1, 2, 3, 5, 8, 40):
        _, und = all_forms(m, model, piece, origin=100, before=bytes(text[100 - nb:100]), open_end=T, aligns=(nb % 4,))
        assert prev is None or und <= prev
        prev = und
    assert prev == 0
    # cells that are no state and no pattern, offsets outside the text
    n = 900
    edge = np.array([-(2 ** 31), -5, -1, 0, 1, 2, 33, T - 3, T - 2, T - 1, T, T + 1, 5000, INT32_MAX - 1, INT32_MAX], dtype=np.int64)
    states, _, _ = model.walk(text)
    for report, all_patterns in FORMS:
        good = np.unique(states) if report == wm.STATE else np.arange(len(PLACED))
        bad = np.array([-1, -(2 ** 31), INT32_MAX, NO_CELL, len(PLACED), model.num_states], dtype=np.int64)
        cells = np.concatenate([good, bad])[rng.integers(0, good.size + bad.size, n)]
        offs = np.sort(np.concatenate([edge[rng.integers(0, edge.size, n // 2)], rng.integers(0, T, n - n // 2)]))
        for count in (n, -1):
            planes = upload(cells, offs, count=count)
            for kw in (dict(open_end=None, lead_begin=-(2 ** 40)), dict(open_end=T, starts=[0, 200, T - 1, T, INT32_MAX]),
                       dict(open_end=2 ** 40, lead_begin=-(2 ** 31) - 50, before=b"abcabcabcabc")):
                ep, eo, und, _ = run_pass(m, model, planes, cells, offs, report, all_patterns, text, what="hostile", **kw)
            for x in planes:
                x.free()
        assert ep.size > 10 and und > 0
    m.close()


# ------------------------------------------------------------------ 4. no groups: the tables of a set without them

def test_a_set_without_groups_uploads_no_group_table(gpu):
    pos = [[ANY, a_, b_, {a_, c_}], [a_, ANY, ANY, c_], [b_, b_]]
    x, y, z = Automaton(), Automaton(), Automaton()
    for i, p in enumerate(pos):
        x.add_wildcard(p, i)
        sets = b"".join(Automaton.byte_set(s) for s in p)
        assert y.lib.acm_automaton_add_wildcard_groups(y.h, sets, len(p), None, 0, i, 0) == i
        z.add_wildcard(p, i, groups=[(1, [b"ab", b"bc"], False)] if i == 1 else ())
    ms = [Matcher(q.compile(), 0, max_text=4096) for q in (x, y, z)]
    assert ms[0].device_bytes == ms[1].device_bytes < ms[2].device_bytes
    text = b"".join(random_texts(5, count=6, longest=300))
    outs = [m.scan_wildcards(text, all_patterns=True) for m in ms]
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][0].size > 30
    with_group = set(zip(outs[2][0].tolist(), outs[2][1].tolist()))
    assert with_group < set(zip(outs[0][0].tolist(), outs[0][1].tolist()))
    assert with_group == wm.brute_force([gm.Pattern(pos[0]), gm.Pattern(pos[1], [(1, [b"ab", b"bc"], False)]), gm.Pattern(pos[2])], [text])
    for m in ms:
        m.close()


# ------------------------------------------------------------------ 5. composition

BODIES = ["(6162|6263)61*62!(6161|6363)",                  # 0: begins and ends with a group; a * between the parts
          "61(626361|636162)62{1-3}(6161|6262|6363)63",    # 1: {1-3} counted between the full spans
          "!(6162)63",                                     # 2: the first position lies in a group (a window, below)
          "63(6161)62",                                    # 3: one string: exact bytes
          "6263"]                                          # 4: plain


def body_automaton(bodies, windows=None):
    a, pats, seqs = Automaton(), [], []
    for q, body in enumerate(bodies):
        ps, gaps = gm.body_patterns(body)
        assert a.add_signature(body, iid=q, groups=True) == q
        seqs.append((list(range(len(pats), len(pats) + len(ps))), gaps))
        pats += ps
    a.compile()
    for i, (lo, hi, fe) in (windows or {}).items():
        a.set_position(i, lo, hi, fe)
    return a, pats, seqs


@pytest.mark.parametrize("kind", ["plain", "window"])
def test_scan_sequences_over_groups(gpu, kind):
    # pattern 4 is "!(6162)63": its window counts from the group's first byte, 2 .. 20 bytes into its text
    windows = {4: (2, 20, False), 0: (0, 40, True)} if kind == "window" else None
    a, pats, seqs = body_automaton(BODIES, windows)
    assert a.has_groups and pats[4].groups and pats[4].pre == 2 and pats[0].groups[0][0] == 0
    m = Matcher(a, 0, max_text=4096)
    texts = random_texts(19, count=40, longest=120)
    want = wm.span_sequences(pats, seqs, texts, windows)
    loose = wm.span_sequences([wm.Pattern(p.positions) for p in pats], seqs, texts, windows)
    assert want < loose and {q for _, q in want} == set(range(len(BODIES)))
    if kind == "plain":                                    # and re says the same of every body, text by text
        base = 0
        for t in texts:
            for q, body in enumerate(BODIES):
                assert {o for o in gm.regex_ends(body, t)} == {o - base for o, s in want if s == q and base <= o < base + len(t)}
            base += len(t)
    for mode in both_pipelines(m):
        go, gq, _, _ = m.scan_sequences(texts=texts)
        got = set(zip(go.tolist(), gq.tolist()))
        assert got == want, (mode, sorted(got - want)[:5], sorted(want - got)[:5])
    m.close()


def test_the_issue_body(gpu):
    body = "aa(bbcc|ddee)ff*!(0102|0304)11"
    a, pats, seqs = body_automaton([body])
    m = Matcher(a, 0, max_text=4096)
    rng = np.random.default_rng(2)
    menu = [bytes.fromhex(x) for x in ("aabbccff", "aaddeeff", "aabbeeff", "010211", "030411", "010411", "ff11", "00", "aa")]
    texts = [b"".join(menu[int(k)] for k in rng.integers(0, len(menu), size=int(rng.integers(0, 14)))) for _ in range(30)]
    want, base = set(), 0
    for t in texts:
        want |= {(base + o, 0) for o in gm.regex_ends(body, t)}
        base += len(t)
    assert len(want) > 20 and want == wm.span_sequences(pats, seqs, texts)
    for mode in both_pipelines(m):
        go, gq, _, _ = m.scan_sequences(texts=texts)
        assert set(zip(go.tolist(), gq.tolist())) == want, mode
    m.close()


def test_scan_rules_over_groups(gpu):
    lines = [("0&1", ["(6162|6263)61", "63!(6161|6363)"]),       # both
             ("0=0&1", ["61(6262|6363)", "6263"]),               # bc without a(bb|cc)
             ("0>1", ["!(6162)63"])]                             # more than once
    a = Automaton()
    for k, (expr, bodies) in enumerate(lines):
        assert a.add_logical_signature(";".join([expr] + bodies), iid=k, groups=True) == k
    a.compile()
    m = Matcher(a, 0, max_text=4096)
    texts = random_texts(23, count=30, longest=40)
    truth = [lambda c: c[0] > 0 and c[1] > 0, lambda c: c[0] == 0 and c[1] > 0, lambda c: c[0] > 1]
    want = set()
    for ti, t in enumerate(texts):
        for k, (expr, bodies) in enumerate(lines):
            counts = [len(gm.regex_ends(b, t)) for b in bodies]
            if truth[k](counts):
                want.add((k, ti))
    assert {k for k, _ in want} == {0, 1, 2} and 10 < len(want) < 3 * len(texts)
    for mode in both_pipelines(m):
        r, t, o, info = m.scan_rules(texts=texts)
        assert set(zip(r.tolist(), t.tolist())) == want and r.size == len(want), mode
    m.close()


# ------------------------------------------------------------------ 6. a seeded database

def test_random_database(gpu):
    rng = np.random.default_rng(101)
    letters = [a_, b_, c_]
    bodies, pats = [], []
    a = Automaton()
    while len(bodies) < 60:
        body = random_body(rng, letters)
        (w,), _ = gm.body_patterns(body)
        assert a.add_signature(body, iid=len(bodies), groups=True) == len(bodies)
        bodies.append(body)
        pats.append(w)
    a.compile()
    model = gm.GroupModel(pats)
    m = Matcher(a, 0, max_text=8192)
    texts = random_texts(7, count=25, longest=100)
    want = wm.brute_force(pats, texts)
    kept = dropped = 0
    for t in texts:
        for w in pats:
            for k in range(len(t) - len(w.positions) + 1):
                if w.context_holds(t, k):
                    kept += w.holds(t, k)
                    dropped += not w.holds(t, k)
    assert kept == len(want) and kept >= 50 and dropped >= 50, (kept, dropped)
    base = 0
    for t in texts[:10]:                                   # re agrees with the model
        for q, body in enumerate(bodies):
            w = pats[q]
            ends = {base + k + w.at + w.L - 1 for k in gm.regex_starts(body, t)}
            assert ends == {o for o, p in want if p == q and base <= o < base + len(t)}
        base += len(t)
    one = b"".join(texts)
    kept_one, und = all_forms(m, model, one, aligns=(1,), open_end=len(one), starts=np.cumsum([0] + [len(t) for t in texts])[:-1].tolist())
    assert und == 0 and kept_one == want
    for mode in both_pipelines(m):
        go, gp, _, info = m.scan_wildcards(texts=texts, all_patterns=True)
        assert set(zip(go.tolist(), gp.tolist())) == want and go.size == len(want) and info[0] == 0, mode
        go, gq, _, _ = m.scan_sequences(texts=texts)
        assert set(zip(go.tolist(), gq.tolist())) == {(o + pats[p].post, p) for o, p in want}, mode
    m.close()
