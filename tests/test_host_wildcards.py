"""Wildcard patterns on the host: acm_automaton_add_wildcard and its getters, the anchor choice, interning, the
extended signature syntax and its file loader, that an automaton without contexts is what it was, and the model
of tests/wildcard_model.py against Python's re.  No device needed.

Of the BAD table of tests/test_host_sequences.py every entry without a new token is tried under the extended
syntax but one: "aa{2147483646}??bb".  In the extended syntax ?? is a position, not a gap of one, so that
body's gap no longer overflows and it is legal (a part ??bb behind a gap of 2147483646)."""
import ctypes as C
import os

import numpy as np
import pytest

import sequence_model as sm
import wildcard_model as wm
from gpu_pattern_matching_amd import AcmError, Automaton
from test_host_sequences import BAD as BAD0, GOOD as GOOD0

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_ARG, ERR_LIMIT, ERR_IO, ERR_PARSE = -1, -5, -6, -7
NIB_HI = lambda h: frozenset(h << 4 | x for x in range(16))      # noqa: E731
NIB_LO = lambda l: frozenset(x << 4 | l for x in range(16))      # noqa: E731
ANY = wm.FULL


def one(b):
    return frozenset((b,))


def snapshot(a):
    return (a.num_patterns, a.num_sequences, a.has_wildcards, a.wildcard_reach,
            [a.wildcard(p) for p in range(a.num_patterns)])


# ------------------------------------------------------------------ the model

@pytest.mark.parametrize("alphabet", [b"ab", b"abc"])
def test_model_against_re(lib, alphabet):
    rng = np.random.default_rng(10 + len(alphabet))
    letters = list(alphabet)
    hits = 0
    for _ in range(60):
        n = int(rng.integers(1, 6))
        positions = []
        for _ in range(n):
            k = int(rng.integers(1, len(letters) + 1))
            positions.append(frozenset(int(x) for x in rng.choice(letters, size=k, replace=False)))
        positions[int(rng.integers(n))] = one(int(rng.choice(letters)))          # an exact byte somewhere
        w = wm.Pattern(positions)
        t = bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=int(rng.integers(0, 40))))
        want = {(k + w.at + w.L - 1, 0) for k in wm.regex_force(positions, t)}
        assert wm.brute_force([w], [t]) == want, (positions, t)
        # the rule over the anchor's records says the same
        model = wm.WildcardModel([w])
        states, offs, _ = model.walk(t)
        p, o, und = model.filter(states, offs, wm.STATE, True, t, open_end=len(t))
        assert und == 0 and set(zip(o.tolist(), p.tolist())) == want, (positions, t)
        hits += len(want)
    assert hits > 50


def test_model_rule_order(lib):
    """no context: kept whatever its text; span outside its text: dropped, not undecided; outside the bytes:
    undecided whatever they hold"""
    m = wm.WildcardModel([[0x61], [ANY, 0x62, 0x62, {0x63, 0x64}]])
    text = b"xbbc"
    assert m.verdict(0, -50, 0, 4, True, text, 0, b"") == wm.KEEP
    assert m.verdict(1, 2, 0, 4, True, text, 0, b"") == wm.KEEP
    assert m.verdict(1, 2, 1, 4, True, text, 0, b"") == wm.DROP              # the pre byte lies in front of T0
    assert m.verdict(1, 2, 0, 3, True, text, 0, b"") == wm.DROP              # the post byte at Tend
    assert m.verdict(1, 2, 0, 0, False, text[:3], 0, b"") == wm.UNDECIDED    # the post byte is not given
    assert m.verdict(1, 2, -5, 9, True, text[1:], 1, b"") == wm.UNDECIDED    # the pre byte is not given
    assert m.verdict(1, 2, -5, 9, True, text[1:], 1, b"x") == wm.KEEP        # ... but for `before`
    assert m.verdict(1, 2, 0, 4, True, b"xbbe", 0, b"") == wm.DROP
    assert m.verdict(7, 2, 0, 4, True, text, 0, b"") == wm.DROP


# ------------------------------------------------------------------ add_wildcard

def test_anchor_choice_and_getters(lib):
    a = Automaton()
    A, B, Cc = 0x41, 0x42, 0x43
    cases = [([A], 0, b"A", 0),                                               # a single exact byte
             ([A, B, {A, B}, Cc], 0, b"AB", 2),                               # an anchor at the front
             ([{A, B}, ANY, A, B, Cc], 2, b"ABC", 0),                         # ... at the back
             ([A, B, ANY, Cc, A], 0, b"AB", 3),                               # a tie: the leftmost
             ([A, ANY, B, Cc, ANY, A, B], 2, b"BC", 3),                       # the leftmost of the longest
             ([ANY, A, ANY], 1, b"A", 1),
             ([{A}, bytes([B]), [Cc]], 0, b"ABC", 0)]                         # all exact: a plain pattern
    for k, (positions, pre, anchor, post) in enumerate(cases):
        assert wm.anchor_of([wm.as_set(p) for p in positions]) == (pre, len(anchor))
        assert a.add_wildcard(positions, iid=100 + k) == k
        assert a.pattern(k)[:2] == (anchor, 100 + k) and a.pattern_flags(k) == 0
        sets = [wm.as_set(p) for p in positions]
        assert a.wildcard(k) == (sets[:pre], sets[pre + len(anchor):]) and a.wildcard_lengths(k) == (pre, post)
        assert lib.acm_automaton_pattern_wildcard(a.h, k, None, None, None, None) == (1 if pre or post else 0)
    assert a.has_wildcards and a.wildcard_reach == (5, 3)
    assert a.add_wildcard([A, ANY], nocase=True) == len(cases) and a.pattern_flags(len(cases)) == 1
    a.add(b"plain")
    assert a.wildcard(len(cases) + 1) == ([], [])
    assert lib.acm_automaton_pattern_wildcard(a.h, 99, None, None, None, None) == ERR_ARG
    assert lib.acm_automaton_wildcards(None) == 0 and lib.acm_automaton_wildcard_reach(None, None, None) == ERR_ARG
    a.compile()                                                               # contexts do not enter compile
    assert a.wildcard(1) == ([], [wm.as_set({A, B}), one(Cc)])
    b = Automaton()
    b.add(b"xy")
    assert not b.has_wildcards and b.wildcard_reach == (0, 0)


def test_errors_apply_nothing(lib):
    a = Automaton()
    a.add(b"first")
    a.add_wildcard([0x41, {1, 2}])
    before = snapshot(a)
    bad = [([], ERR_ARG), ([{1, 2}, wm.FULL], ERR_ARG), ([0x41, []], ERR_ARG),
           ([0x41] * 4097, ERR_LIMIT), ([{1, 2}] + [0x41] * 4096, ERR_LIMIT)]
    for positions, code in bad:
        with pytest.raises(AcmError) as e:
            a.add_wildcard(positions)
        assert e.value.code == code and snapshot(a) == before, (len(positions), str(e.value))
    sets = Automaton.byte_set(0x41)
    assert lib.acm_automaton_add_wildcard(a.h, sets, 1, 0, 2) == ERR_ARG       # unknown flags
    assert lib.acm_automaton_add_wildcard(a.h, None, 1, 0, 0) == ERR_ARG
    assert lib.acm_automaton_add_wildcard(None, sets, 1, 0, 0) == ERR_ARG
    assert lib.acm_automaton_add_wildcard(a.h, sets, 0, 0, 0) == ERR_ARG
    assert lib.acm_automaton_add_wildcard(a.h, sets, -3, 0, 0) == ERR_ARG
    assert snapshot(a) == before
    assert a.add_wildcard([0x41] + [{1, 2}] * 4095) == 2                       # the limit itself
    a.compile()
    with pytest.raises(AcmError) as e:
        a.add_wildcard([0x41, {1, 2}])                                         # it adds a pattern: only before compile
    assert e.value.code == ERR_ARG and a.num_patterns == 3


def test_interning_limit(lib):
    a = Automaton()
    distinct = [frozenset((k, (k + 1 + j) % 256)) for j in range(2) for k in range(128)]    # 256 two-byte sets
    assert len(set(distinct)) == 256
    for k in range(0, 255, 5):
        a.add_wildcard([0x41] + distinct[k:k + 5])
    a.add_wildcard([distinct[3], 0x42, distinct[255], 7, 9])    # the 256th distinct set; repeats and one-byte sets are free
    before = snapshot(a)
    extra = frozenset((1, 2, 3))
    assert extra not in distinct
    with pytest.raises(AcmError) as e:
        a.add_wildcard([0x43, distinct[0], extra])                            # the 257th
    assert e.value.code == ERR_LIMIT and snapshot(a) == before
    assert a.add_wildcard([0x43, distinct[0], distinct[200], 5]) == a.num_patterns - 1
    for syntax_body in ("41(01|02|03)", "41*42{3}(01|02|03)43"):
        with pytest.raises(AcmError) as e:
            a.add_signature(syntax_body, extended=True)                       # asked before any part is added
        assert e.value.code == ERR_LIMIT and a.num_patterns == before[0] + 1 and a.num_sequences == 0
    a.compile()


def test_all_exact_is_the_plain_automaton(lib):
    rng = np.random.default_rng(5)
    pats = [bytes(rng.integers(97, 101, size=int(rng.integers(3, 9)), dtype=np.uint8)) for _ in range(40)]
    plain, wild = Automaton(), Automaton()
    for i, p in enumerate(pats):
        plain.add(p, i)
        assert wild.add_wildcard(list(p), i) == i
    plain.compile()
    wild.compile()
    assert not wild.has_wildcards and wild.num_states == plain.num_states
    assert np.array_equal(wild.reference_table(), plain.reference_table())
    assert wild.byte_classes()[0] == plain.byte_classes()[0]
    assert np.array_equal(wild.byte_classes()[1], plain.byte_classes()[1])
    st = [(C.c_uint32 * 21)(), (C.c_uint32 * 21)()]
    assert lib.acm_sieve_selftest(plain.h, st[0]) == lib.acm_sieve_selftest(wild.h, st[1]) == 1
    assert list(st[0]) == list(st[1])
    # and with contexts compile still sees the anchors alone
    ctx = Automaton()
    for i, p in enumerate(pats):
        ctx.add_wildcard([wm.FULL] + list(p) + [{1, 2}], i)
    ctx.compile()
    assert ctx.has_wildcards and np.array_equal(ctx.reference_table(), plain.reference_table())
    assert lib.acm_sieve_selftest(ctx.h, st[1]) == 1 and list(st[0]) == list(st[1])


# ------------------------------------------------------------------ the extended syntax

GOOD = [("aabb", [[one(0xAA), one(0xBB)]], []),
        ("aa?b", [[one(0xAA), NIB_LO(0xB)]], []),
        ("a?bb", [[NIB_HI(0xA), one(0xBB)]], []),
        ("aA??bB", [[one(0xAA), ANY, one(0xBB)]], []),                          # ?? is a position
        ("aa????bb", [[one(0xAA), ANY, ANY, one(0xBB)]], []),
        ("(aa|bb)cc", [[frozenset((0xAA, 0xBB)), one(0xCC)]], []),
        ("(aa)", [[one(0xAA)]], []),                                            # one entry: an exact byte
        ("(aa|aa|AA)", [[one(0xAA)]], []),
        ("!(aa|bb)cc", [[ANY - {0xAA, 0xBB}, one(0xCC)]], []),
        ("!(00)11", [[ANY - {0}, one(0x11)]], []),
        ("aa{2-10}?bcc*dd??(01|02)", [[one(0xAA)], [NIB_LO(0xB), one(0xCC)], [one(0xDD), ANY, frozenset((1, 2))]],
         [(2, 10), (0, None)]),
        ("aa??*bb", [[one(0xAA), ANY], [one(0xBB)]], [(0, None)]),              # ?? next to a gap stays a position
        ("aa{3}??bb", [[one(0xAA)], [ANY, one(0xBB)]], [(3, 3)]),
        ("aa{2147483646}??bb", [[one(0xAA)], [ANY, one(0xBB)]], [(2147483646, 2147483646)]),
        ("00{5}{-3}*11", [[one(0)], [one(0x11)]], [(5, None)])]
BAD = [("", 1), ("a", 1), ("aab", 3), ("a?", 1), ("?a", 1), ("a?*b?", 1), ("aa*?b", 4), ("aa?", 3), ("?", 1), ("?g", 1),
       ("??aa", 1), ("aa??", 5), ("aa*??", 6), ("(aabb|ccdd)", 4), ("(aa|bbcc)", 7), ("aa(bb|cc", 9), ("aa(bb|)", 7),
       ("aa()", 4), ("aa(b)", 4), ("aa(bb", 6), ("aa|bb", 3), ("aa)bb", 3), ("!aa", 1), ("aa!bb", 3), ("aa!", 3), ("aa!!(bb)", 3),
       ("aa!(bb", 7), ("aa bb", 3), ("aag0", 3), ("*aa", 1), ("{3}aa", 1), ("aa*", 4), ("aa{3}", 6), ("aa{}bb", 3),
       ("aa{x}bb", 3), ("aa{2147483647}bb", 3), ("aa{1-2147483646}{1}bb", 17), ("aa}bb", 3),
       ("aa*(bb|cc)??*dd", 4),                                                  # a part without an exact byte: where it begins
       ("!(" + "|".join("%02x" % b for b in range(256)) + ")aa", 1),            # no byte left
       ("00" + "*11" * 32, 99)]


def test_parser_token_forms(lib):
    for k, (body, parts, gaps) in enumerate(GOOD):
        assert wm.parse_body_ex(body) == (parts, gaps), body
        a = Automaton()
        a.add(b"first")
        assert a.add_signature(body, iid=40 + k, extended=True) == 0
        assert a.num_patterns == 1 + len(parts) and a.num_sequences == 1
        ps, gs, iid = a.sequence(0)
        assert ps == list(range(1, 1 + len(parts))) and gs == gaps and iid == 40 + k, body
        for j, p in enumerate(ps):
            w = wm.Pattern(parts[j])
            assert a.pattern(p)[:2] == (w.anchor, 40 + k) and a.pattern_flags(p) == 0
            assert a.wildcard(p) == (parts[j][:w.pre], parts[j][w.at + w.L:]), body
        a.compile()
    a = Automaton()
    assert a.add_signature("61?263{1-2}4445", iid=3, nocase=True, extended=True) == 0
    assert [a.pattern_flags(p) for p in range(2)] == [1, 1] and a.wildcard_lengths(0) == (0, 2)
    with pytest.raises(sm.BodyError):
        wm.parse_body_ex("aa" + "??" * 4096 + "bb")                            # a part of 4098 positions
    with pytest.raises(AcmError) as e:
        a.add_signature("aa" + "??" * 4096 + "bb", extended=True)
    assert e.value.code == ERR_PARSE and a.num_patterns == 2


def test_parser_rejects_with_the_column(lib):
    carried = [(b, c) for b, c in BAD0 if not set(b) & set("?(|)!")]
    assert len(carried) >= 15
    for body, col in BAD + carried:
        with pytest.raises(sm.BodyError) as me:
            wm.parse_body_ex(body)
        assert me.value.column == col, body
        a = Automaton()
        a.add(b"first")
        with pytest.raises(AcmError) as e:
            a.add_signature(body, extended=True)
        assert e.value.code == ERR_PARSE and "column %d:" % col in str(e.value), (body, str(e.value))
        assert a.num_patterns == 1 and a.num_sequences == 0, body
    # syntax 0 keeps rejecting every new token, through the new entry point as well
    for body in ("a?", "?a", "(aa|bb)", "!(aa)bb"):
        assert lib.acm_automaton_add_signature_ex(Automaton().h, body.encode(), 0, 0, 0) == ERR_PARSE
    assert lib.acm_automaton_add_signature_ex(Automaton().h, b"aa", 0, 0, 2) == ERR_ARG     # unknown syntax bits
    assert lib.acm_automaton_add_signature_ex(Automaton().h, b"aa", 0, 2, 1) == ERR_ARG     # unknown flags
    assert lib.acm_automaton_add_signature_ex(Automaton().h, None, 0, 0, 1) == ERR_ARG
    assert lib.acm_automaton_load_signature_file_ex(Automaton().h, b"x", 0, 4) == ERR_ARG
    c = Automaton().compile()
    with pytest.raises(AcmError) as e:
        c.add_signature("aa?b", extended=True)
    assert e.value.code == ERR_ARG and c.num_patterns == 0


def test_syntaxes_agree_without_new_tokens(lib):
    bodies = [g[0] for g in GOOD0 if "?" not in g[0]] + ["aabbcc", "00*11{2-3}2233"]
    assert len(bodies) >= 9
    for body in bodies:
        a, b = Automaton(), Automaton()
        assert a.add_signature(body, iid=7) == b.add_signature(body, iid=7, extended=True) == 0
        assert a.num_patterns == b.num_patterns and a.sequence(0) == b.sequence(0)
        assert [a.pattern(p) for p in range(a.num_patterns)] == [b.pattern(p) for p in range(b.num_patterns)]
        assert not b.has_wildcards


def test_signature_file(lib, tmp_path):
    good = tmp_path / "good.sig"
    good.write_bytes(b"# signatures\n\naabb\n  77:cc?d{2-4}ee  \n00*11??22\r\n12:(34|35)36\n")
    a = Automaton()
    a.add(b"first")
    assert a.load_signature_file(good, extended=True) == 4
    assert a.num_sequences == 4 and a.num_patterns == 1 + 1 + 2 + 2 + 1
    assert a.sequence(1) == ([2, 3], [(2, 4)], 77) and a.wildcard(2) == ([], [NIB_LO(0xD)])
    assert a.sequence(2) == ([4, 5], [(0, None)], 2) and a.pattern(5)[0] == b"\x11" and a.wildcard_lengths(5) == (0, 2)
    assert a.sequence(3) == ([6], [], 12) and a.pattern(6)[:2] == (b"\x36", 12)
    for k, (line, col) in enumerate([(b"aab", 3), (b"5:aa??", 7), (b"aa(bbcc)", 6), (b"9:", 3)]):
        b = Automaton()
        b.add(b"first")
        f = tmp_path / ("bad%d.sig" % k)
        f.write_bytes(b"# c\naa?b\n" + line + b"\nccdd\n")
        with pytest.raises(AcmError) as e:
            b.load_signature_file(f, extended=True)
        assert e.value.code == ERR_PARSE and "bad%d.sig:3:" % k in str(e.value), (line, str(e.value))
        assert "column %d:" % col in str(e.value), (line, str(e.value))
        assert b.num_patterns == 1 and b.num_sequences == 0 and not b.has_wildcards, line
    with pytest.raises(AcmError) as e:
        a.load_signature_file(tmp_path / "missing.sig", extended=True)
    assert e.value.code == ERR_IO


def test_clamav_fixture_loads_identically(lib, tmp_path):
    with open(os.path.join(HERE, "data", "clamav", "15000.txt"), "rb") as f:
        lines = f.read().split(b"\n")[:2000]
    part = tmp_path / "2000.txt"
    part.write_bytes(b"\n".join(lines) + b"\n")
    a, b = Automaton(), Automaton()
    assert a.load_signature_file(part) == b.load_signature_file(part, extended=True) == 2000
    assert b.num_sequences == 2000 and b.num_patterns == 2000 and not b.has_wildcards
    for i in range(2000):
        assert a.pattern(i) == b.pattern(i)
    assert all(a.sequence(i) == b.sequence(i) for i in (0, 1, 999, 1999))
    a.compile()
    b.compile()
    assert np.array_equal(a.reference_table(), b.reference_table())


# ------------------------------------------------------------------ the two folds, on the model

def test_folds_on_the_model(lib):
    """A sequence over wildcard parts, found by brute force on the parts' full spans, equals the sequence model
    run on the anchors' records that the wildcard rule keeps, with the folded lengths L + pre + post of the part
    in front; the reported end is the last anchor's, post of the last part in front of the match's end."""
    rng = np.random.default_rng(21)
    a_, b_ = 0x61, 0x62
    AB = frozenset((a_, b_))
    found = 0
    for trial in range(40):
        pats = []
        for _ in range(5):
            n = int(rng.integers(1, 5))
            pos = [AB if rng.random() < 0.4 else one(int(rng.choice([a_, b_]))) for _ in range(n)]
            pos[int(rng.integers(n))] = one(int(rng.choice([a_, b_])))
            pats.append(wm.Pattern(pos))
        seqs = [([0, 1], [(int(rng.integers(0, 3)), int(rng.integers(0, 4)))]), ([2, 3, 4], [(0, None), (1, 2)])]
        texts = [bytes(rng.choice(np.array([a_, b_, 0x63], dtype=np.uint8), size=int(rng.integers(0, 18)))) for _ in range(3)]
        want = wm.span_sequences(pats, seqs, texts)
        model = wm.WildcardModel(pats)
        whole = b"".join(texts)
        starts = np.cumsum([0] + [len(t) for t in texts])[:-1]
        recs = sorted((o, i) for o, i in wm.brute_force([wm.Pattern([one(x) for x in p.anchor]) for p in pats], texts))
        # (the anchors' records per text; the rule then sees them with the texts' starts)
        p = np.array([i for _, i in recs], dtype=np.int64)
        o = np.array([x for x, _ in recs], dtype=np.int64)
        kp, ko, und = model.filter(p, o, wm.HEAD, True, whole, starts=starts, open_end=len(whole))
        assert und == 0
        folded = []
        for i, w in enumerate(pats):
            prev = next((s[0][s[0].index(i) - 1] for s in seqs if i in s[0] and s[0].index(i) > 0), None)
            folded.append(w.L + w.pre + (pats[prev].post if prev is not None else 0))
        q, e, _ = sm.SequenceModel(folded, seqs).run(kp, ko, starts=starts)
        got = {(int(end) + pats[seqs[int(s)][0][-1]].post, int(s)) for s, end in zip(q.tolist(), e.tolist())}
        assert got == want, (trial, texts)
        found += len(want)
    assert found > 20
