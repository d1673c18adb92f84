"""Ordered multi-part signatures on the host: acm_automaton_add_sequence and its getters, the signature parser
and file loader, that compile does not see sequences, and the model of tests/sequence_model.py against a brute
force and a regular expression.  No device needed."""
import ctypes as C
import os

import numpy as np
import pytest

import sequence_model as sm
from gpu_pattern_matching_amd import AcmError, Automaton

HERE = os.path.dirname(os.path.abspath(__file__))
PATS = [b"abc", b"bcd", b"c", b"abcabc", b"xyz", b"", b"dd", b"e"]
ERR_ARG, ERR_LIMIT, ERR_IO, ERR_PARSE = -1, -5, -6, -7
UNB = 0x7FFFFFFF


def fresh(pats=PATS):
    a = Automaton()
    for i, p in enumerate(pats):
        a.add(p, i)
    return a


def sieve_stats(lib, a):
    st = (C.c_uint32 * 21)()
    rc = lib.acm_sieve_selftest(a.h, st)
    return rc, list(st)


def snapshot(a):
    return (a.num_patterns, a.num_sequences, [a.sequence(i) for i in range(a.num_sequences)],
            [a.pattern_sequence(p) for p in range(a.num_patterns)])


def test_round_trip(lib):
    a = fresh()
    assert a.num_sequences == 0 and all(a.pattern_sequence(p) is None for p in range(len(PATS)))
    assert a.add_sequence([2], [], iid=70) == 0
    assert a.add_sequence([0, 1], [(0, 3)], iid=-5) == 1
    assert a.add_sequence([3, 4, 6], [(1, None), (0, 0)], iid=9) == 2
    assert a.add_sequence([7], iid=1) == 3
    assert a.num_sequences == 4
    assert a.sequence(0) == ([2], [], 70)
    assert a.sequence(1) == ([0, 1], [(0, 3)], -5)
    assert a.sequence(2) == ([3, 4, 6], [(1, None), (0, 0)], 9)
    assert a.sequence(3) == ([7], [], 1)
    assert [a.pattern_sequence(p) for p in range(8)] == [(1, 0), (1, 1), (0, 0), (2, 0), (2, 1), None, (2, 2), (3, 0)]
    # any of the getter's pointers may be NULL
    n = C.c_int32()
    assert lib.acm_automaton_sequence(a.h, 2, None, C.byref(n), None, None, None) == 0 and n.value == 3
    assert lib.acm_automaton_pattern_sequence(a.h, 0, None, None) == 1
    assert lib.acm_automaton_num_sequences(None) == 0
    # lo > hi is legal
    b = fresh()
    assert b.add_sequence([0, 1], [(5, 2)]) == 0 and b.sequence(0)[1] == [(5, 2)]
    # the limit itself
    c = fresh([b"p%02d" % i for i in range(33)])
    assert c.add_sequence(list(range(32)), [(1, 1)] * 31) == 0
    assert c.pattern_sequence(31) == (0, 31) and c.pattern_sequence(32) is None


def test_argument_errors_apply_nothing(lib):
    a = fresh()
    a.add_sequence([0, 1], [(0, 3)], iid=4)
    before = snapshot(a)
    bad = [([], [], ERR_ARG),                       # nparts < 1
           ([8], [], ERR_ARG), ([-1], [], ERR_ARG),   # a bad index
           ([2, 0], [(0, 0)], ERR_ARG),              # a part already used
           ([2, 3, 2], [(0, 0), (0, 0)], ERR_ARG),   # twice in one call
           ([2, 5], [(0, 0)], ERR_ARG),              # a part of length 0
           ([2, 3], [(-1, 4)], ERR_ARG), ([2, 3], [(0, -2)], ERR_ARG)]
    for parts, gaps, code in bad:
        with pytest.raises(AcmError) as e:
            a.add_sequence(parts, gaps)
        assert e.value.code == code, (parts, gaps)
        assert snapshot(a) == before, (parts, gaps)
    c = fresh([b"p%02d" % i for i in range(40)])
    with pytest.raises(AcmError) as e:
        c.add_sequence(list(range(33)), [(0, 0)] * 32)
    assert e.value.code == ERR_LIMIT and c.num_sequences == 0 and c.pattern_sequence(0) is None
    one = (C.c_int32 * 2)(2, 3)
    assert lib.acm_automaton_add_sequence(None, one, one, one, 2, 0) == ERR_ARG
    assert lib.acm_automaton_add_sequence(a.h, None, one, one, 2, 0) == ERR_ARG
    assert lib.acm_automaton_add_sequence(a.h, one, None, one, 2, 0) == ERR_ARG
    assert lib.acm_automaton_add_sequence(a.h, one, one, None, 2, 0) == ERR_ARG
    assert snapshot(a) == before
    assert lib.acm_automaton_add_sequence(a.h, one, None, None, 1, 0) == 1      # one part: the gap arrays are ignored
    for i in (-1, 2):
        assert lib.acm_automaton_sequence(a.h, i, None, None, None, None, None) == ERR_ARG
    for p in (-1, 8):
        assert lib.acm_automaton_pattern_sequence(a.h, p, None, None) == ERR_ARG


@pytest.mark.parametrize("pats", [[b"abcd", b"bcde", b"abc", b"cdefgh"], PATS[:5]], ids=["sparse", "chain"])
def test_compile_does_not_see_sequences(lib, pats):
    seqs = [([0, 1], [(0, 7)]), ([3], [])]
    plain = sm.build(pats, [])
    before = sm.build(pats, seqs)
    after = sm.build(pats, seqs, compile_first=True)
    assert plain.num_sequences == 0 and before.num_sequences == 2 and after.num_sequences == 2
    assert before.sequence(0) == after.sequence(0) == ([0, 1], [(0, 7)], 0)
    for a in (before, after):
        assert np.array_equal(a.reference_table(), plain.reference_table())
        assert sieve_stats(lib, a) == sieve_stats(lib, plain)
        assert a.byte_classes()[0] == plain.byte_classes()[0] and a.num_states == plain.num_states
        assert not a.positioned and not a.mixed_case


# ------------------------------------------------------------------ the parser

GOOD = [("aabb", [b"\xaa\xbb"], []),
        ("AaBb{2-10}ccdd*eeff??0011", [b"\xaa\xbb", b"\xcc\xdd", b"\xee\xff", b"\x00\x11"], [(2, 10), (0, None), (1, 1)]),
        ("00{5}11", [b"\x00", b"\x11"], [(5, 5)]),
        ("00{-7}11", [b"\x00", b"\x11"], [(0, 7)]),
        ("00{3-}11", [b"\x00", b"\x11"], [(3, None)]),
        ("00{0}11", [b"\x00", b"\x11"], [(0, 0)]),
        ("00{9-2}11", [b"\x00", b"\x11"], [(9, 2)]),                     # lo > hi: legal, never matches
        ("00????11", [b"\x00", b"\x11"], [(2, 2)]),                       # adjacent gap tokens add
        ("00??{2-4}{-3}11", [b"\x00", b"\x11"], [(3, 8)]),
        ("00??{2-4}*11", [b"\x00", b"\x11"], [(3, None)]),               # a sum with an unbounded term
        ("00*{6}11", [b"\x00", b"\x11"], [(6, None)]),
        ("00{2147483646}11", [b"\x00", b"\x11"], [(2147483646, 2147483646)])]
BAD = [("", 1), ("a", 1), ("aab", 3), ("a?", 1), ("?a", 1), ("aa?bcc", 3), ("aa?", 3), ("(aa|bb)", 1), ("aa(bb|cc)dd", 3),
       ("aa!bb", 3), ("!aa", 1), ("aa bb", 3), ("aag0", 3), ("??aa", 1), ("*aa", 1), ("{3}aa", 1), ("aa??", 5), ("aa*", 4),
       ("aa{3}", 6), ("aa{}bb", 3), ("aa{-}bb", 3), ("aa{3-4bb", 3), ("aa{x}bb", 3), ("aa{3-4-5}bb", 3), ("aa{ 3}bb", 3),
       ("aa{2147483647}bb", 3), ("aa{2147483646}??bb", 15), ("aa{1-2147483646}{1}bb", 17), ("aa}bb", 3),
       ("00" + "*11" * 32, 99)]


def test_parser_token_forms(lib):
    for k, (body, parts, gaps) in enumerate(GOOD):
        assert sm.parse_body(body) == (parts, gaps), body
        a = Automaton()
        a.add(b"first")
        assert a.add_signature(body, iid=40 + k) == 0
        assert a.num_patterns == 1 + len(parts) and a.num_sequences == 1
        ps, gs, iid = a.sequence(0)
        assert ps == list(range(1, 1 + len(parts))) and gs == gaps and iid == 40 + k, body
        for j, p in enumerate(ps):
            assert a.pattern(p)[:2] == (parts[j], 40 + k) and a.pattern_flags(p) == 0
        a.compile()
    a = Automaton()
    assert a.add_signature("616263{1-2}4445", iid=3, nocase=True) == 0 and a.add_signature(b"7a") == 1
    assert [a.pattern_flags(p) for p in range(3)] == [1, 1, 0] and a.sequence(1) == ([2], [], 0)
    thirty_two = "00" + "*11" * 31
    assert len(sm.parse_body(thirty_two)[0]) == 32 and Automaton().add_signature(thirty_two) == 0


def test_parser_rejects_with_the_column(lib):
    for body, col in BAD:
        with pytest.raises(sm.BodyError) as me:
            sm.parse_body(body)
        assert me.value.column == col, body
        a = Automaton()
        a.add(b"first")
        with pytest.raises(AcmError) as e:
            a.add_signature(body)
        assert e.value.code == ERR_PARSE and "column %d:" % col in str(e.value), (body, str(e.value))
        assert a.num_patterns == 1 and a.num_sequences == 0, body      # parsed completely before anything is added
    a = Automaton()
    a.add(b"first")
    a.compile()
    with pytest.raises(AcmError) as e:
        a.add_signature("aabb")                                        # it adds patterns: only before compile
    assert e.value.code == ERR_ARG and a.num_patterns == 1 and a.num_sequences == 0
    assert lib.acm_automaton_add_signature(Automaton().h, b"aa", 0, 2) == ERR_ARG
    assert lib.acm_automaton_add_signature(Automaton().h, None, 0, 0) == ERR_ARG


def test_signature_file(lib, tmp_path):
    good = tmp_path / "good.sig"
    good.write_bytes(b"# signatures\n\naabb\n  77:ccdd{2-4}ee  \n   # indented\r\n00*11??22\r\n4294967295\n12:34\n")
    a = Automaton()
    a.add(b"first")
    assert a.load_signature_file(good) == 5
    assert a.num_sequences == 5 and a.num_patterns == 1 + 1 + 2 + 3 + 1 + 1
    assert a.sequence(0) == ([1], [], 0)                               # no "<iid>:": the sequence index
    assert a.sequence(1) == ([2, 3], [(2, 4)], 77)
    assert a.sequence(2) == ([4, 5, 6], [(0, None), (1, 1)], 2)
    assert a.sequence(3) == ([7], [], 3) and a.pattern(7)[0] == bytes.fromhex("4294967295")   # digits alone are hex
    assert a.sequence(4) == ([8], [], 12) and a.pattern(8)[:2] == (b"\x34", 12)
    assert a.load_signature_file(good, nocase=True) == 5 and a.num_sequences == 10
    assert a.sequence(5) == ([9], [], 5) and a.pattern_flags(9) == 1 and a.pattern_flags(1) == 0
    empty = tmp_path / "empty.sig"
    empty.write_bytes(b"# nothing\n\n")
    assert a.load_signature_file(empty) == 0
    for k, (line, col) in enumerate([(b"aab", 3), (b"5:aa??", 7), (b"aa(bb)", 3), (b"9:", 3), (b"99999999999:aa", 11)]):
        b = Automaton()
        b.add(b"first")
        f = tmp_path / ("bad%d.sig" % k)
        f.write_bytes(b"# c\naabb\n" + line + b"\nccdd\n")
        with pytest.raises(AcmError) as e:
            b.load_signature_file(f)
        assert e.value.code == ERR_PARSE and "bad%d.sig:3:" % k in str(e.value), (line, str(e.value))
        assert "column %d:" % col in str(e.value), (line, str(e.value))
        assert b.num_patterns == 1 and b.num_sequences == 0, line       # nothing of a bad file is applied
    with pytest.raises(AcmError) as e:
        a.load_signature_file(tmp_path / "missing.sig")
    assert e.value.code == ERR_IO
    c = Automaton().compile()
    with pytest.raises(AcmError) as e:
        c.load_signature_file(good)
    assert e.value.code == ERR_ARG and c.num_sequences == 0


def test_clamav_fixture_loads_as_it_is(lib, tmp_path):
    with open(os.path.join(HERE, "data", "clamav", "15000.txt"), "rb") as f:
        lines = f.read().split(b"\n")[:2000]
    part = tmp_path / "2000.txt"
    part.write_bytes(b"\n".join(lines) + b"\n")
    a = Automaton()
    assert a.load_signature_file(part) == 2000
    assert a.num_sequences == 2000 and a.num_patterns == 2000
    for i in (0, 1, 999, 1999):
        assert a.sequence(i) == ([i], [], i) and a.pattern(i)[0] == bytes.fromhex(lines[i].decode())
    a.compile()


# ------------------------------------------------------------------ the model

MODEL_PATS = [b"a", b"ab", b"ba", b"b", b"aa", b"bab", b"a", b"b", b"abb"]
MODEL_SEQS = [([0], []), ([1, 2], [(0, 2)]), ([3, 4, 5], [(1, None), (0, 1)]), ([6, 7], [(2, 1)]), ([8], [])]


def entries_of(pats, t):
    """(patterns, offsets) of every occurrence in t, in offset order, the patterns of an offset in index order"""
    recs = sorted((k + len(p) - 1, i) for i, p in enumerate(pats) if p for k in sm.occurrences(t, p))
    return np.array([i for _, i in recs], dtype=np.int64), np.array([o for o, _ in recs], dtype=np.int64)


@pytest.mark.parametrize("alphabet", [b"ab", b"abc"])
def test_model_against_brute_force(lib, alphabet):
    rng = np.random.default_rng(len(alphabet))
    model = sm.SequenceModel([len(p) for p in MODEL_PATS], MODEL_SEQS)
    seen = {q: 0 for q in range(len(MODEL_SEQS))}
    for _ in range(150):
        t = bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=int(rng.integers(0, 25))))
        p, o = entries_of(MODEL_PATS, t)
        q, e, info = model.run(p, o)
        got = set(zip(e.tolist(), q.tolist()))
        assert len(got) == q.size
        assert got == sm.brute_force(MODEL_PATS, MODEL_SEQS, [t]), t
        assert got == sm.regex_force(MODEL_PATS, MODEL_SEQS, t), t
        assert info[0] == p.size and info[1] >= q.size
        for x in q.tolist():
            seen[x] += 1
    assert seen[3] == 0 and all(seen[x] > 0 for x in (0, 1, 2, 4))   # lo > hi never matches; the others do


def test_model_texts(lib):
    """no chain crosses a text start, a part does not start in front of its T0, the lead text may begin anywhere"""
    pats = [b"ab", b"cd", b"abc"]
    seqs = [([0, 1], [(0, None)]), ([2], [])]
    model = sm.SequenceModel([2, 2, 3], seqs)
    texts = [b"ab..cd", b"ab", b"cd", b"", b"abcd", b"bc"]
    base = np.cumsum([0] + [len(t) for t in texts])
    p, o = entries_of(pats, b"".join(texts))
    q, e, _ = model.run(p, o, starts=base[:-1])
    assert set(zip(e.tolist(), q.tolist())) == sm.brute_force(pats, seqs, texts) == {(5, 0), (13, 0), (12, 1)}
    q, e, _ = model.run(p, o)                                            # one text: the chains cross
    assert set(zip(e.tolist(), q.tolist())) == sm.brute_force(pats, seqs, [b"".join(texts)])
    assert (9, 0) in set(zip(e.tolist(), q.tolist()))
    # "abc" ends at 2 of a lead text that began at 1: it starts in front of it
    q, e, _ = model.run([2, 2], [2, 3], lead_begin=1)
    assert e.tolist() == [3]
    q, e, _ = model.run([2, 2], [2, 3], lead_begin=-(2 ** 40))
    assert e.tolist() == [2, 3]
