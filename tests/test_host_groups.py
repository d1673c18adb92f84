"""Groups of wildcard patterns on the host: acm_automaton_add_wildcard_groups and its getters, the syntax bit
ACM_SIG_GROUPS and the loaders that take it, that nothing is applied on an error, that a pattern without groups
is what acm_automaton_add_wildcard adds, and the model of tests/group_model.py against Python's re.  No device
needed."""
import ctypes as C

import numpy as np
import pytest

import group_model as gm
import sequence_model as sm
import wildcard_model as wm
from gpu_pattern_matching_amd import AcmError, Automaton, _lib

ERR_ARG, ERR_LIMIT, ERR_IO, ERR_PARSE = -1, -5, -6, -7
ANY = wm.FULL
EXT, GROUPS = 1, 2


def one(b):
    return frozenset((b,))


def snapshot(a):
    return (a.num_patterns, a.num_sequences, a.num_rules, a.has_wildcards, a.has_groups, a.wildcard_reach,
            [(a.wildcard(p), a.wildcard_groups(p)) for p in range(a.num_patterns)])


def alts(n, width=2):
    """n distinct strings of `width` bytes as hex alternatives"""
    return ["%0*x" % (2 * width, 0x0100 + k) for k in range(n)]


# ------------------------------------------------------------------ the syntax

G = lambda at, strings, neg=False: (at, [bytes.fromhex(s) for s in strings], neg)    # noqa: E731

# body, parts, gaps, groups per part
GOOD = [("aa(bbcc|ddee)ff", [[one(0xAA), ANY, ANY, one(0xFF)]], [], [[G(1, ["bbcc", "ddee"])]]),
        ("aa!(0102|0304)11", [[one(0xAA), ANY, ANY, one(0x11)]], [], [[G(1, ["0102", "0304"], True)]]),
        ("(aabb|ccdd)ee", [[ANY, ANY, one(0xEE)]], [], [[G(0, ["aabb", "ccdd"])]]),            # a group begins the body
        ("ee(aabb|ccdd)", [[one(0xEE), ANY, ANY]], [], [[G(1, ["aabb", "ccdd"])]]),            # ... and ends it
        ("(aabb)", [[one(0xAA), one(0xBB)]], [], [[]]),                                       # one string: exact bytes
        ("(aabb|AABB|aabb)cc", [[one(0xAA), one(0xBB), one(0xCC)]], [], [[]]),                # ... after deduplication
        ("11!(aabb)", [[one(0x11), ANY, ANY]], [], [[G(1, ["aabb"], True)]]),                 # negated: a group all the same
        ("11(aabb|ccdd|aabb|CCDD|eeff)", [[one(0x11), ANY, ANY]], [], [[G(1, ["aabb", "ccdd", "eeff"])]]),
        ("(aa|bb)cc", [[frozenset((0xAA, 0xBB)), one(0xCC)]], [], [[]]),                      # one byte: a set, as without the bit
        ("!(aa|bb)cc(0102|0304)", [[ANY - {0xAA, 0xBB}, one(0xCC), ANY, ANY]], [], [[G(2, ["0102", "0304"])]]),
        ("11(aabb|ccdd)(0102|0304)22", [[one(0x11)] + [ANY] * 4 + [one(0x22)]], [],
         [[G(1, ["aabb", "ccdd"]), G(3, ["0102", "0304"])]]),                                 # adjacent groups
        ("aa(bbcc|ddee)ff*!(0102|0304)11", [[one(0xAA), ANY, ANY, one(0xFF)], [ANY, ANY, one(0x11)]], [(0, None)],
         [[G(1, ["bbcc", "ddee"])], [G(0, ["0102", "0304"], True)]]),
        ("11(" + "|".join(alts(256)) + ")", [[one(0x11), ANY, ANY]], [], [[G(1, alts(256))]]),  # the limits themselves
        ("11(" + "|".join(alts(2, 32)) + ")", [[one(0x11)] + [ANY] * 32], [], [[G(1, alts(2, 32))]]),
        ("11" + "(0102|0304)" * 16, [[one(0x11)] + [ANY] * 32], [], [[G(1 + 2 * k, ["0102", "0304"]) for k in range(16)]]),
        ("11" + "(0102|0304)" * 16 + "(0506)", [[one(0x11)] + [ANY] * 32 + [one(5), one(6)]], [],
         [[G(1 + 2 * k, ["0102", "0304"]) for k in range(16)]]),                              # an exact run is no group
        ("aa??(0102|0304)?b", [[one(0xAA), ANY, ANY, ANY, frozenset(x << 4 | 0xB for x in range(16))]], [],
         [[G(2, ["0102", "0304"])]])]
BAD = [("aa(bbcc|dd)", 9), ("aa(bb|ccdd)", 7), ("aa(bbcc|ddeeff)11", 9),                        # unequal widths: where it begins
       ("11(" + "|".join(alts(2, 33)) + ")", 3), ("11!(" + "|".join(alts(2, 33)) + ")", 3),  # width 33: the ( or !
       ("aabb(" + "|".join(alts(257)) + ")", 5), ("11!(" + "|".join(alts(257)) + ")", 3),     # 257 alternatives
       ("11" + "(0102|0304)" * 17, 3 + 11 * 16), ("11" + "(0102|0304)" * 16 + "!(0506)", 3 + 11 * 16),   # a 17th group
       ("aa(bbc|dd)", 6), ("aa(bbcc|)", 9), ("aa(bbcc", 8), ("aa(bbcc|ddee", 13), ("aa()", 4), ("aa(bbcc,ddee)", 8),
       ("(aabb|ccdd)", 1), ("(aabb|ccdd)??*11", 1),                                           # a part without an exact byte
       ("??(aabb|ccdd)11", 1), ("11(aabb|ccdd)??", 16),                                        # ?? at an end stays refused
       ("11(aabb|ccdd)*", 15), ("aa!bbcc", 3)]


def test_good_bodies(lib):
    for k, (body, parts, gaps, groups) in enumerate(GOOD):
        assert gm.parse_body_groups(body) == (parts, gaps, groups), body
        a = Automaton()
        a.add(b"first")
        assert a.add_signature(body, iid=40 + k, groups=True) == 0, body
        assert a.num_patterns == 1 + len(parts) and a.num_sequences == 1
        ps, gs, iid = a.sequence(0)
        assert ps == list(range(1, 1 + len(parts))) and gs == gaps and iid == 40 + k, body
        for j, p in enumerate(ps):
            w = wm.Pattern(parts[j])
            assert a.pattern(p)[:2] == (w.anchor, 40 + k)
            assert a.wildcard(p) == (parts[j][:w.pre], parts[j][w.at + w.L:]), body
            assert a.wildcard_groups(p) == groups[j], body
            assert lib.acm_automaton_pattern_groups(a.h, p) == len(groups[j])
        assert a.has_groups == any(groups)
        a.compile()                                                       # groups do not enter compile
        assert a.wildcard_groups(1) == groups[0]


def test_bad_bodies_name_the_column(lib):
    for body, col in BAD:
        with pytest.raises(sm.BodyError) as me:
            gm.parse_body_groups(body)
        assert me.value.column == col, body
        a = Automaton()
        a.add(b"first")
        with pytest.raises(AcmError) as e:
            a.add_signature(body, groups=True)
        assert e.value.code == ERR_PARSE and "column %d:" % col in str(e.value), (body[:40], str(e.value))
        assert a.num_patterns == 1 and a.num_sequences == 0 and not a.has_groups, body
    # every body of the extended syntax reads the same with the bit
    from test_host_wildcards import BAD as BAD_EX, GOOD as GOOD_EX
    for body, parts, gaps in GOOD_EX:
        assert gm.parse_body_groups(body) == (parts, gaps, [[] for _ in parts]), body
        a, b = Automaton(), Automaton()
        assert a.add_signature(body, extended=True) == b.add_signature(body, groups=True) == 0
        assert snapshot(a) == snapshot(b) and not b.has_groups
    changed = {"(aabb|ccdd)": 1, "(aa|bbcc)": 5, "aa(bb|)": 7}
    for body, col in BAD_EX:
        col = changed.get(body, col)
        with pytest.raises(sm.BodyError) as me:
            gm.parse_body_groups(body)
        assert me.value.column == col, body
        with pytest.raises(AcmError) as e:
            Automaton().add_signature(body, groups=True)
        assert e.value.code == ERR_PARSE and "column %d:" % col in str(e.value), (body[:40], str(e.value))


def test_syntax_bits(lib):
    h = lambda: Automaton().h                                             # noqa: E731
    assert lib.acm_automaton_add_signature_ex(h(), b"aa(bbcc|ddee)", 0, 0, GROUPS) == ERR_ARG      # the bit alone
    assert lib.acm_automaton_add_signature_ex(h(), b"aa", 0, 0, GROUPS) == ERR_ARG
    assert lib.acm_automaton_load_signature_file_ex(h(), b"x", 0, GROUPS) == ERR_ARG
    assert lib.acm_automaton_add_logical_signature(h(), b"0;aa", 0, 0, GROUPS) == ERR_ARG
    assert lib.acm_automaton_load_logical_file(h(), b"x", 0, GROUPS) == ERR_ARG
    assert lib.acm_automaton_add_signature_ex(h(), b"aa", 0, 0, 4) == ERR_ARG
    assert lib.acm_automaton_add_signature_ex(h(), b"aa", 0, 0, EXT | GROUPS | 4) == ERR_ARG
    keep = Automaton()
    assert lib.acm_automaton_add_signature_ex(keep.h, b"aa(bbcc|ddee)", 0, 0, EXT | GROUPS) == 0 and keep.has_groups
    assert _lib.SIG_GROUPS == GROUPS and _lib.SIG_EXTENDED == EXT
    # the extended syntax alone is what it was
    with pytest.raises(AcmError) as e:
        Automaton().add_signature("(aabb|ccdd)", extended=True)
    assert e.value.code == ERR_PARSE and "column 4:" in str(e.value)
    with pytest.raises(AcmError) as e:
        Automaton().add_signature("aa(bbcc|ddee)", extended=False)
    assert e.value.code == ERR_PARSE


# ------------------------------------------------------------------ the C interface

def test_add_and_getters(lib):
    a = Automaton()
    positions = [ANY, ANY, 0x41, 0x42, ANY, ANY, ANY, {1, 2}, ANY, ANY]
    groups = [(0, [b"xy", b"zw"], False), (4, [b"abc"], True), (8, [b"pq", b"pq", b"rs", b"pq"], False)]
    assert a.add_wildcard(positions, iid=9, groups=groups) == 0
    assert a.pattern(0)[:2] == (b"AB", 9) and a.wildcard_lengths(0) == (2, 6) and a.has_wildcards and a.has_groups
    assert a.wildcard_groups(0) == [(0, [b"xy", b"zw"], False), (4, [b"abc"], True), (8, [b"pq", b"rs"], False)]
    assert wm.anchor_of([wm.as_set(p) for p in positions]) == (2, 2)       # the sets alone decide the anchor
    a.add(b"plain")
    assert a.wildcard_groups(1) == [] and lib.acm_automaton_pattern_groups(a.h, 1) == 0
    at, w, cnt, neg = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.acm_automaton_pattern_group(a.h, 0, 1, C.byref(at), C.byref(w), C.byref(cnt), C.byref(neg), None) == 0
    assert (at.value, w.value, cnt.value, neg.value) == (4, 3, 1, 1)
    assert lib.acm_automaton_pattern_group(a.h, 0, 2, None, None, None, None, None) == 0
    for index, j in ((0, 3), (0, -1), (1, 0), (2, 0), (-1, 0)):
        assert lib.acm_automaton_pattern_group(a.h, index, j, None, None, None, None, None) == ERR_ARG
    assert lib.acm_automaton_pattern_groups(a.h, 2) == ERR_ARG and lib.acm_automaton_pattern_groups(None, 0) == ERR_ARG
    assert lib.acm_automaton_groups(None) == 0
    b = Automaton()
    b.add_wildcard([0x41, ANY, {1, 2}])
    assert not b.has_groups and b.has_wildcards
    # a pattern of 256 strings of 32 bytes, and 16 groups
    wide = [bytes([k]) * 32 for k in range(256)]
    assert b.add_wildcard([0x41] + [ANY] * 32, groups=[(1, wide + wide[:7], True)]) == 1
    assert b.wildcard_groups(1) == [(1, wide, True)]
    assert b.add_wildcard([0x41] + [ANY] * 32, groups=[(1 + 2 * k, [b"ab", b"cd"], False) for k in range(16)]) == 2


def test_errors_apply_nothing(lib):
    a = Automaton()
    a.add(b"first")
    a.add_wildcard([0x41, ANY, ANY], groups=[(1, [b"ab", b"cd"], False)])
    before = snapshot(a)
    P = [0x41, ANY, ANY, ANY, ANY, 0x42]
    two = [b"ab", b"cd"]
    bad = [(P, [(1, two, False), (2, two, False)], ERR_ARG),               # overlap
           (P, [(3, two, False), (1, two, False)], ERR_ARG),               # not ascending
           (P, [(1, two, False), (1, two, False)], ERR_ARG),
           (P, [(-1, two, False)], ERR_ARG), (P, [(5, two, False)], ERR_ARG), (P, [(6, two, False)], ERR_ARG),   # out of range
           (P, [(4, two, False)], ERR_ARG), (P, [(0, two, False)], ERR_ARG),                                     # on an exact byte
           ([0x41, ANY, {1, 2}, 0x42], [(1, two, False)], ERR_ARG),        # a covered position that is not full
           ([0x41, ANY, ANY - {0}, 0x42], [(1, two, False)], ERR_ARG),
           (P, [(1, [b"a", b"b"], False)], ERR_ARG),                       # width 1
           ([0x41] + [ANY] * 40, [(1, [b"x" * 33], False)], ERR_LIMIT),    # width 33
           ([0x41] + [ANY] * 40, [(1, [bytes([k, 7]) for k in range(256)] + [b"zz"], False)], ERR_LIMIT),   # a 257th string
           ([0x41] + [ANY] * 40, [(1 + 2 * k, two, False) for k in range(17)], ERR_LIMIT),                   # a 17th group
           ([ANY, ANY], [(0, two, False)], ERR_ARG),                       # no exact byte
           ([0x41, ANY, ANY, []], [(1, two, False)], ERR_ARG)]             # an empty set
    for positions, groups, code in bad:
        with pytest.raises(AcmError) as e:
            a.add_wildcard(positions, groups=groups)
        assert e.value.code == code and snapshot(a) == before, (groups, str(e.value))
    sets = b"".join(Automaton.byte_set(p) for p in P)
    raw = b"abcd"
    g = (_lib.WildGroup * 1)(_lib.WildGroup(1, 2, 2, 0, raw))
    call = lib.acm_automaton_add_wildcard_groups
    assert call(a.h, sets, 6, g, -1, 0, 0) == ERR_ARG
    assert call(a.h, sets, 6, None, 1, 0, 0) == ERR_ARG
    assert call(a.h, sets, 6, g, 1, 0, 2) == ERR_ARG                        # unknown flags
    assert call(None, sets, 6, g, 1, 0, 0) == ERR_ARG and call(a.h, None, 6, g, 1, 0, 0) == ERR_ARG
    for field, value in (("count", 0), ("negated", 2), ("negated", -1), ("bytes", None)):
        h = (_lib.WildGroup * 1)(_lib.WildGroup(1, 2, 2, 0, raw))
        setattr(h[0], field, value)
        assert call(a.h, sets, 6, h, 1, 0, 0) == ERR_ARG, field
    assert snapshot(a) == before
    assert call(a.h, sets, 6, g, 1, 5, 1) == 2 and a.pattern_flags(2) == 1 and a.wildcard_groups(2) == [(1, two, False)]
    a.compile()
    with pytest.raises(AcmError) as e:
        a.add_wildcard(P, groups=[(1, two, False)])                        # it adds a pattern: only before compile
    assert e.value.code == ERR_ARG and a.num_patterns == 3


def test_no_groups_is_add_wildcard(lib):
    rng = np.random.default_rng(3)
    a, b = Automaton(), Automaton()
    for i in range(40):
        n = int(rng.integers(2, 9))
        positions = [ANY if rng.random() < 0.3 else int(rng.integers(97, 101)) for _ in range(n)]
        positions[int(rng.integers(n))] = int(rng.integers(97, 101))
        sets = b"".join(Automaton.byte_set(p) for p in positions)
        assert a.add_wildcard(positions, i) == lib.acm_automaton_add_wildcard_groups(b.h, sets, n, None, 0, i, 0) == i
    assert snapshot(a) == snapshot(b) and not b.has_groups
    assert [a.pattern(i) for i in range(40)] == [b.pattern(i) for i in range(40)]
    a.compile()
    b.compile()
    assert np.array_equal(a.reference_table(), b.reference_table())
    st = [(C.c_uint32 * 21)(), (C.c_uint32 * 21)()]
    ok = lib.acm_sieve_selftest(a.h, st[0])
    assert lib.acm_sieve_selftest(b.h, st[1]) == ok and list(st[0]) == list(st[1])
    # and with groups compile still sees the anchors alone
    c = Automaton()
    for i in range(40):
        anchor = a.pattern(i)[0]
        pre, post = a.wildcard(i)
        c.add_wildcard(pre + list(anchor) + post + [ANY, ANY], i, groups=[(len(pre) + len(anchor) + len(post), [b"ab", b"cd"], False)])
    c.compile()
    assert c.has_groups and np.array_equal(c.reference_table(), a.reference_table())
    assert lib.acm_sieve_selftest(c.h, st[1]) == ok and list(st[0]) == list(st[1])


# ------------------------------------------------------------------ all-or-nothing loads

def test_files_apply_all_or_nothing(lib, tmp_path):
    good = tmp_path / "good.sig"
    good.write_bytes(b"# signatures\naabb\n 77:cc(0102|0304)ee  \n00*!(1112|1314)22\r\n")
    a = Automaton()
    a.add(b"first")
    assert a.load_signature_file(good, groups=True) == 3
    assert a.num_sequences == 3 and a.num_patterns == 5 and a.has_groups
    assert a.sequence(1) == ([2], [], 77) and a.wildcard_groups(2) == [(1, [b"\x01\x02", b"\x03\x04"], False)]
    assert a.wildcard_groups(4) == [(0, [b"\x11\x12", b"\x13\x14"], True)] and a.pattern(4)[0] == b"\x22"
    with pytest.raises(AcmError) as e:                                      # the same file without the bit: refused whole
        Automaton().load_signature_file(good, extended=True)
    assert e.value.code == ERR_PARSE and "good.sig:3:" in str(e.value) and "column 10:" in str(e.value)
    for k, (line, col) in enumerate([(b"aa(bbcc|dd)", 9), (b"5:11" + b"(0102|0304)" * 17, 5 + 11 * 16), (b"(aabb|ccdd)", 1)]):
        b = Automaton()
        b.add(b"first")
        f = tmp_path / ("bad%d.sig" % k)
        f.write_bytes(b"aa(0102|0304)\n" + line + b"\nccdd\n")
        with pytest.raises(AcmError) as e:
            b.load_signature_file(f, groups=True)
        assert e.value.code == ERR_PARSE and "bad%d.sig:2:" % k in str(e.value) and "column %d:" % col in str(e.value), str(e.value)
        assert snapshot(b)[:5] == (1, 0, 0, False, False), line
    # a file that needs a 257th set is refused whole, its groups with it
    full = Automaton()
    for k in range(0, 255, 5):
        full.add_wildcard([0x41] + [frozenset((j, (j + 1) % 256)) for j in range(k, k + 5)])
    before = snapshot(full)
    f = tmp_path / "sets.sig"
    f.write_bytes(b"aa(0102|0304)bb\ncc(01|02|03)\ndd(05|06|07)\n")          # ?? is the 256th, then two more
    with pytest.raises(AcmError) as e:
        full.load_signature_file(f, groups=True)
    assert e.value.code == ERR_LIMIT and snapshot(full) == before
    # logical signatures take the bit through their syntax argument
    r = Automaton()
    assert r.add_logical_signature("0&1;aa(bbcc|ddee)ff;11!(0102|0304)", iid=4, groups=True) == 0
    assert r.num_rules == 1 and r.num_sequences == 2 and r.wildcard_groups(1) == [(1, [b"\x01\x02", b"\x03\x04"], True)]
    before = snapshot(r)
    with pytest.raises(AcmError) as e:
        r.add_logical_signature("0&1;aabb;11(0102|03)", groups=True)
    assert e.value.code == ERR_PARSE and "column 18:" in str(e.value) and snapshot(r) == before
    with pytest.raises(AcmError) as e:
        r.add_logical_signature("0;aa(bbcc|ddee)", extended=True)
    assert e.value.code == ERR_PARSE and snapshot(r) == before
    ldb = tmp_path / "rules.ldb"
    ldb.write_bytes(b"0|1;aa(bbcc|ddee);2233\n7:0;44!(0102)\n")
    assert r.load_logical_file(ldb, groups=True) == 2 and r.num_rules == 3
    bad = tmp_path / "bad.ldb"
    bad.write_bytes(b"0;aa(bbcc|ddee)\n0;aa(bbcc|dd)\n")
    before = snapshot(r)
    with pytest.raises(AcmError) as e:
        r.load_logical_file(bad, groups=True)
    assert e.value.code == ERR_PARSE and "bad.ldb:2" in str(e.value) and snapshot(r) == before


# ------------------------------------------------------------------ the model against re

def random_body(rng, letters):
    """a body of one part over the letters: exact bytes, ??, sets and one to three groups, an exact byte for sure"""
    tok, n_groups = [], 0
    for _ in range(int(rng.integers(2, 6))):
        r = rng.random()
        if r < 0.45 and n_groups < 3:
            w = int(rng.integers(2, 4))
            k = int(rng.integers(1, 4))
            strings = ["".join("%02x" % int(rng.choice(letters)) for _ in range(w)) for _ in range(k)]
            neg = rng.random() < 0.4
            if len(set(strings)) == 1 and not neg:
                strings.append("".join("%02x" % (letters[0] + 7) for _ in range(w)))      # (never in the text)
            tok.append(("!(" if neg else "(") + "|".join(strings) + ")")
            n_groups += 1
        elif r < 0.6:
            tok.append("??")
        elif r < 0.7:
            tok.append("(%02x|%02x)" % (letters[0], letters[1]))
        else:
            tok.append("%02x" % int(rng.choice(letters)))
    if n_groups == 0:
        tok.append("(%02x%02x|%02x%02x)" % (letters[0], letters[1], letters[1], letters[2]))
    return "%02x" % int(rng.choice(letters)) + "".join(tok) + "%02x" % int(rng.choice(letters))


def test_model_against_re(lib):
    rng = np.random.default_rng(77)
    letters = [0x61, 0x62, 0x63]
    kept_by_group = dropped_by_group = 0
    for trial in range(220):
        body = random_body(rng, letters)
        (w,), gaps = gm.body_patterns(body)
        assert gaps == [] and w.groups
        t = bytes(rng.choice(np.array(letters, dtype=np.uint8), size=int(rng.integers(0, 60))))
        n = len(w.positions)
        want = {k + w.at + w.L - 1 for k in gm.regex_starts(body, t)}
        assert {o for o, _ in wm.brute_force([w], [t])} == want, (body, t)
        assert {o - w.post for o in gm.regex_ends(body, t)} == want, (body, t)
        # the rule over the anchor's records says the same
        model = gm.GroupModel([w])
        states, offs, _ = model.walk(t)
        p, o, und = model.filter(states, offs, wm.STATE, True, t, open_end=len(t))
        assert und == 0 and set(o.tolist()) == want, (body, t)
        # occurrences of the sets alone: the groups decide these
        for k in range(len(t) - n + 1):
            if w.context_holds(t, k):
                kept_by_group += w.holds(t, k)
                dropped_by_group += not w.holds(t, k)
    assert kept_by_group >= 50 and dropped_by_group >= 50, (kept_by_group, dropped_by_group)


def test_the_issue_body(lib):
    body = "aa(bbcc|ddee)ff*!(0102|0304)11"
    pats, gaps = gm.body_patterns(body)
    assert gaps == [(0, None)] and [len(p.positions) for p in pats] == [4, 3]
    t = bytes.fromhex("aabbccff 0102 11 aaddeeff 0103 11 0304 11 aabbcdff 9999 11 aaddeeff 11".replace(" ", ""))
    want = {e for e, _ in wm.span_sequences(pats, [([0, 1], gaps)], [t])}
    assert want == set(gm.regex_ends(body, t)) and len(want) == 3
