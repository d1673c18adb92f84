"""Rules on the host: acm_automaton_add_rule and its getters, the expression parser with its columns, the
empty-text refusal, logical signatures and their file loader, that compile does not see rules, and the model
of tests/rule_model.py against a second evaluation.  No device needed."""
import ctypes as C
import re

import numpy as np
import pytest

import rule_model as rm
from gpu_pattern_matching_amd import AcmError, Automaton

ERR_ARG, ERR_LIMIT, ERR_IO, ERR_PARSE = -1, -5, -6, -7
CODE = {"arg": ERR_ARG, "limit": ERR_LIMIT, "parse": ERR_PARSE}


def fresh(n=8):
    """n one-pattern sequences"""
    a = Automaton()
    for i in range(n):
        a.add(b"pat%03d" % i, i)
        a.add_sequence([i], [], iid=100 + i)
    return a


def snapshot(a):
    return (a.num_patterns, a.num_sequences, a.num_rules, [a.rule(i) for i in range(a.num_rules)],
            [a.sequence_rule(q) for q in range(a.num_sequences)])


# ------------------------------------------------------------------ the model against a second evaluation


class V:
    """a (count, truth) pair with the operators of the expression language"""

    def __init__(self, c, t=None):
        self.c, self.t = c, (c > 0 if t is None else t)

    def __and__(self, o):
        return V(self.c + o.c, self.t and o.t)

    def __or__(self, o):
        return V(self.c + o.c, self.t or o.t)

    def eq(self, n):
        return V(self.c, self.c == n)

    def gt(self, n):
        return V(self.c, self.c > n)

    def lt(self, n):
        return V(self.c, self.c < n)


def to_python(expr):
    """the expression, token by token, as a Python expression over V objects c[j]: an operand is c[j], a
    comparison a method call on the term in front of it -- which Python's own parser finds"""
    out, toks = [], re.findall(r"\d+|[()&|=<>]", expr)
    k = 0
    while k < len(toks):
        t = toks[k]
        if t in "=<>":
            out.append(".%s(%s)" % ({"=": "eq", ">": "gt", "<": "lt"}[t], toks[k + 1]))
            k += 2
            continue
        out.append("c[%s]" % t if t.isdigit() else t)
        k += 1
    return "".join(out)


def random_expr(rng, nops, depth=0):
    def term():
        if depth < 3 and rng.random() < 0.3:
            t = "(" + random_expr(rng, nops, depth + 1) + ")"
        else:
            t = "%d" % rng.integers(nops)
        if rng.random() < 0.3:
            t += "%s%d" % ("=><"[rng.integers(3)], rng.integers(0, 5))
        return t
    op = "&|"[rng.integers(2)]
    pad = [" ", "", "\t"][rng.integers(3)]
    return (pad + op + pad).join(term() for _ in range(int(rng.integers(1, 4))))


def test_model_against_python_eval():
    rng = np.random.default_rng(7)
    seen = 0
    for _ in range(400):
        nops = int(rng.integers(1, 6))
        e = random_expr(rng, nops)
        py = to_python(e)
        empty = eval(py, {"c": [V(0)] * nops}).t
        try:
            tree = rm.parse(e, nops)
        except rm.RuleError as err:
            assert err.kind == "arg" and empty, e
            continue
        assert not empty, e
        for _ in range(5):
            counts = [int(x) for x in rng.integers(0, 4, nops)]
            got = rm.evaluate(tree, counts)
            want = eval(py, {"c": [V(x) for x in counts]})
            assert got == (want.c, want.t), (e, counts)
            seen += got[1]
    assert seen > 200


def test_values():
    ev = lambda e, c: rm.evaluate(rm.parse(e, len(c)), c)
    assert ev("0&1", [2, 3]) == (5, True) and ev("0&1", [2, 0]) == (2, False)
    assert ev("0|1", [0, 3]) == (3, True)
    assert ev("(0|1)>3", [2, 2]) == (4, True) and ev("(0|1)>3", [4, 0]) == (4, True) and ev("(0|1)>3", [3, 0]) == (3, False)
    assert ev("0&1=0", [1, 0]) == (1, True) and ev("0&1=0", [1, 1]) == (2, False)
    assert ev("0<2&1", [1, 1])[1] and not ev("0<2&1", [2, 1])[1] and not ev("0<2&1", [0, 0])[1]


# ------------------------------------------------------------------ the parser of the library

# (expression, operands, error kind, column)
BAD = [("", 2, "parse", 1), ("  ", 2, "parse", 3), ("0&", 2, "parse", 3), ("&0", 2, "parse", 1),
       ("0&1|0", 2, "parse", 4), ("0|1&0", 2, "parse", 4), ("(0&1|0)", 2, "parse", 5), ("0 & 1 | 0", 2, "parse", 7),
       ("0=1,2", 2, "parse", 4), ("(0|1)=2,1", 2, "parse", 8),
       ("2", 2, "parse", 1), ("0&(1|7)", 3, "parse", 6), ("0&12", 12, "parse", 3),
       ("(0", 2, "parse", 3), ("(0&1", 2, "parse", 5), ("0)", 2, "parse", 2), ("()", 2, "parse", 2),
       ("0=", 2, "parse", 3), ("0>x", 2, "parse", 3), ("0=1=2", 2, "parse", 4), ("0 1", 2, "parse", 3),
       ("a", 2, "parse", 1), ("0&-1", 2, "parse", 3), ("0;1", 2, "parse", 2), ("0&&1", 2, "parse", 3),
       ("0=2147483648", 2, "parse", 3), ("0>99999999999999999999", 2, "parse", 3), ("4294967296", 2, "parse", 1),
       ("0\n", 2, "parse", 2),
       ("(" * 9 + "0" + ")" * 9, 2, "limit", 9), ("0&" + "(" * 9 + "1" + ")" * 9, 2, "limit", 11),
       ("0=0", 1, "arg", None), ("0<5", 1, "arg", None), ("(0|1)=0", 2, "arg", None), ("0=0|1", 2, "arg", None),
       ("(0&1)<1", 2, "arg", None)]

GOOD = ["0", "0&1", "0|1|2", "(0&1)|2>3", "0&1=0", " ( 0\t| 1 ) > 3 ", "0=2", "0>2", "0<2&1", "0&0&0", "(0)",
        "(" * 8 + "0" + ")" * 8, "0=2147483647&1", "((0|1)>1&2)|(3&4=0)", "0>0"]


@pytest.mark.parametrize("expr,nops,kind,col", BAD)
def test_parse_errors(lib, expr, nops, kind, col):
    with pytest.raises(rm.RuleError) as m:
        rm.parse(expr, nops)
    assert (m.value.kind, m.value.column) == (kind, col)
    a = fresh(max(nops, 1))
    before = snapshot(a)
    with pytest.raises(AcmError) as e:
        a.add_rule(list(range(nops)), expr)
    assert e.value.code == CODE[kind], lib.acm_last_error()
    if col is not None:
        assert b"column %d:" % col in lib.acm_last_error(), lib.acm_last_error()
    assert snapshot(a) == before


def test_good_expressions(lib):
    for e in GOOD:
        rm.parse(e, 5)
        a = fresh(5)
        assert a.add_rule([0, 1, 2, 3, 4], e, iid=3) == 0, e
        assert a.rule(0) == ([0, 1, 2, 3, 4], e, 3)


def test_limits(lib):
    a = fresh(66)
    assert a.add_rule(list(range(64)), "|".join("%d" % j for j in range(64))) == 0      # the limits themselves
    b = fresh(66)
    before = snapshot(b)
    with pytest.raises(AcmError) as e:
        b.add_rule(list(range(65)), "0")
    assert e.value.code == ERR_LIMIT and snapshot(b) == before
    with pytest.raises(rm.RuleError) as m:
        rm.parse("0", 65)
    assert m.value.kind == "limit"
    with pytest.raises(AcmError) as e:
        b.add_rule([0], "(" * 9 + "0" + ")" * 9)
    assert e.value.code == ERR_LIMIT and snapshot(b) == before
    assert b.add_rule([0], "(" * 8 + "0" + ")" * 8) == 0


def test_round_trip_and_argument_errors(lib):
    a = fresh()
    assert a.num_rules == 0 and all(a.sequence_rule(q) is None for q in range(8))
    assert a.add_rule([5, 2], "0&1", iid=-4) == 0
    assert a.add_rule([0], "0>2", iid=77) == 1
    a.compile()
    assert a.add_rule([7, 1, 3], "(0|1)>3|2", iid=9) == 2                              # behind compile too
    assert a.num_rules == 3
    assert a.rule(0) == ([5, 2], "0&1", -4) and a.rule(1) == ([0], "0>2", 77) and a.rule(2) == ([7, 1, 3], "(0|1)>3|2", 9)
    assert [a.sequence_rule(q) for q in range(8)] == [(1, 0), (2, 1), (0, 1), (2, 2), None, (0, 0), None, (2, 0)]
    n = C.c_int32()
    assert lib.acm_automaton_rule(a.h, 2, None, C.byref(n), None, None) == 0 and n.value == 3
    assert lib.acm_automaton_sequence_rule(a.h, 0, None, None) == 1
    assert lib.acm_automaton_num_rules(None) == 0
    before = snapshot(a)
    for seqs, expr in (([], "0"), ([8], "0"), ([-1], "0"), ([4, 2], "0&1"),          # a sequence used in another rule
                       ([4, 6, 4], "0&1&2"), ([4, 4], "0|1")):                        # twice in one list
        with pytest.raises(AcmError) as e:
            a.add_rule(seqs, expr)
        assert e.value.code == ERR_ARG, (seqs, expr)
        assert snapshot(a) == before
    assert lib.acm_automaton_add_rule(a.h, None, 1, b"0", 0) == ERR_ARG
    assert lib.acm_automaton_add_rule(a.h, (C.c_int32 * 1)(4), 1, None, 0) == ERR_ARG
    assert lib.acm_automaton_rule(a.h, 3, None, None, None, None) == ERR_ARG
    assert lib.acm_automaton_sequence_rule(a.h, 8, None, None) == ERR_ARG
    assert snapshot(a) == before and a.add_rule([4, 6], "0&1=0") == 3


# ------------------------------------------------------------------ logical signatures


def test_logical_signature(lib):
    a = Automaton()
    a.add(b"plain", 1)
    assert a.add_logical_signature("(0&1)|2>3;aabb;ccdd{2-4}ee;ff00ff", iid=40) == 0
    assert a.num_patterns == 5 and a.num_sequences == 3 and a.num_rules == 1
    assert a.rule(0) == ([0, 1, 2], "(0&1)|2>3", 40)
    assert a.sequence(1) == ([2, 3], [(2, 4)], 40) and a.pattern(1)[0] == b"\xaa\xbb"
    assert a.add_logical_signature("0;a?(bb|cc)dd", iid=41, extended=True, nocase=True) == 1
    assert a.has_wildcards and a.rule(1)[0] == [3]
    before = snapshot(a)
    #        what                                      code       column
    bad = [("0&1;aabb;ccdd;zz", ERR_PARSE, 15),                                    # the third body
           ("0&1;aabb;ccdd;ee{", ERR_PARSE, 17),
           ("0&2;aabb;ccdd", ERR_PARSE, 3),                                         # an operand without a body
           ("0&|1;aabb;ccdd", ERR_PARSE, 3),
           ("0;EOF-10:aabb", ERR_PARSE, 9), ("0;aabb::i", ERR_PARSE, 7), ("0&1;aabb;0,5:ccdd", ERR_PARSE, 13),
           ("0", ERR_PARSE, 2), ("0;", ERR_PARSE, 3), ("0&1;aabb;", ERR_PARSE, 10), (";aabb", ERR_PARSE, 1),
           ("0=0;aabb", ERR_ARG, None),
           ("0;a?", ERR_PARSE, 3)]                                                  # extended syntax without the flag
    for line, code, col in bad:
        with pytest.raises(AcmError) as e:
            a.add_logical_signature(line)
        assert e.value.code == code, (line, lib.acm_last_error())
        if col is not None:
            assert b"column %d:" % col in lib.acm_last_error(), (line, lib.acm_last_error())
        assert snapshot(a) == before, line
    with pytest.raises(AcmError) as e:
        a.add_logical_signature(";".join(["0"] + ["aabb"] * 65))
    assert e.value.code == ERR_LIMIT and snapshot(a) == before
    # the room for wildcard sets is asked before anything is added
    sets = ";".join("(%02x|%02x)aa" % (i, j) for i in range(17) for j in range(i + 1, 17))[:64 * 10 - 1]
    assert sets.count(";") == 63
    b = Automaton()
    for k in range(4):
        b.add_logical_signature("0;" + ";".join("(%02x|%02x)bb" % (k + 20, j) for j in range(30, 80)), extended=True)
    snap = snapshot(b)
    with pytest.raises(AcmError) as e:
        b.add_logical_signature("0;" + sets, extended=True)
    assert e.value.code == ERR_LIMIT and snapshot(b) == snap
    a.compile()
    with pytest.raises(AcmError) as e:
        a.add_logical_signature("0;aabb")
    assert e.value.code == ERR_ARG


def test_logical_file(lib, tmp_path):
    good = tmp_path / "good.ldb"
    good.write_text("# a comment\n\n7:0&1;aabb;ccdd\n   \n0|1;eeff*00;1122\n  # indented comment\n900:0>1;abcd\r\n")
    a = Automaton()
    assert a.load_logical_file(good) == 3
    assert a.num_rules == 3 and a.num_sequences == 5
    assert [a.rule(i)[2] for i in range(3)] == [7, 1, 900]                         # no id: the rule index
    assert a.rule(1) == ([2, 3], "0|1", 1) and a.sequence(2)[0] == [2, 3]
    assert a.sequence(4)[2] == 900
    before = snapshot(a)
    bad = tmp_path / "bad.ldb"
    for text, code, needle in (("0;aabb\n0&1;aabb;cc\n0;zz\n", ERR_PARSE, b":3: column 3:"),
                               ("0;aabb\n\n# x\n12:0&&1;aa;bb\n", ERR_PARSE, b":4: column 6:"),
                               ("0;aabb\n0<1;bb\n", ERR_ARG, b":2:"),
                               ("0;aabb\n99999999999:0;bb\n", ERR_PARSE, b":2:")):
        bad.write_text(text)
        with pytest.raises(AcmError) as e:
            a.load_logical_file(bad)
        assert e.value.code == code and needle in lib.acm_last_error(), (text, lib.acm_last_error())
        assert snapshot(a) == before
    with pytest.raises(AcmError) as e:
        a.load_logical_file(tmp_path / "missing.ldb")
    assert e.value.code == ERR_IO
    ext = tmp_path / "ext.ldb"
    ext.write_text("0&1;a?bb;(cc|dd)ee\n")
    with pytest.raises(AcmError):
        a.load_logical_file(ext)
    assert snapshot(a) == before and a.load_logical_file(ext, extended=True) == 1 and a.rule(3)[2] == 3


# ------------------------------------------------------------------ compile does not see rules


def test_compile_does_not_see_rules(lib):
    rng = np.random.default_rng(9)
    pats = [bytes(rng.integers(97, 103, size=int(rng.integers(3, 9)), dtype=np.uint8)) for _ in range(60)]
    plain, ruled, late = Automaton(), Automaton(), Automaton()
    for a in (plain, ruled, late):
        for i, p in enumerate(pats):
            a.add(p, i)
            a.add_sequence([i], [], iid=i)
    for r in range(10):
        ruled.add_rule(list(range(6 * r, 6 * r + 6)), "(0&1)|(2|3)>2|(4&5=0)", iid=r)
    for a in (plain, ruled, late):
        a.compile()
    late.add_rule([0, 1], "0|1")
    assert ruled.num_rules == 10 and plain.num_rules == 0
    for a in (ruled, late):
        assert a.num_states == plain.num_states and np.array_equal(a.reference_table(), plain.reference_table())
        assert a.byte_classes()[0] == plain.byte_classes()[0]
        st = [(C.c_uint32 * 21)(), (C.c_uint32 * 21)()]
        assert lib.acm_sieve_selftest(plain.h, st[0]) == lib.acm_sieve_selftest(a.h, st[1]) == 1
        assert list(st[0]) == list(st[1])
        ct = [(C.c_uint32 * 32)(), (C.c_uint32 * 32)()]
        assert lib.acm_compact_selftest(plain.h, 160 * 1024, ct[0]) == lib.acm_compact_selftest(a.h, 160 * 1024, ct[1])
        assert list(ct[0]) == list(ct[1])
