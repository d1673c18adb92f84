"""Approximate patterns on the host (acm_automaton_add_approx and its accessors) and the model of
tests/approx_model.py against an independent brute force.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import approx_model as am
from gpu_pattern_matching_amd import AcmError, Automaton, _lib

ERR_ARG = -1


def planted_case(seed=21, size=2400):
    """2400 random bytes over {a, b, c}, 15 patterns with (n, k) from (4, 1) to (32, 15), and near-copies of every
    pattern planted with 0 .. k substitutions so that the long ones match too"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abc", dtype=np.uint8)
    text = rng.choice(letters, size=size).copy()
    pats = [(bytes(rng.choice(letters, size=4 + 2 * (k - 1))), k) for k in range(1, 16)]
    at = 10
    for p, k in pats:
        for d in sorted({0, 1, k // 2, k - 1, k, k + 1}):
            copy = np.frombuffer(p, dtype=np.uint8).copy()
            for i in rng.choice(len(p), size=min(d, len(p)), replace=False).tolist():
                copy[i] = letters[(int(np.flatnonzero(letters == copy[i])[0]) + 1) % 3]
            if at + copy.size > size:
                break
            text[at:at + copy.size] = copy
            at += copy.size + 3
    assert at < size
    return bytes(text), pats


# ------------------------------------------------------------------ the pieces


def test_piece_boundaries_for_every_n_and_k():
    for k in range(0, 16):
        for n in range(k + 1, 41):
            a = Automaton()
            pat = bytes((7 * i + k) % 251 for i in range(n))
            a.add(b"zz", 5)
            first = a.add_approx(pat, k, iid=n)
            assert first == 1
            b = am.piece_bounds(n, k)
            q, r = divmod(n, k + 1)
            assert b[0] == 0 and b[-1] == n and [b[i + 1] - b[i] for i in range(k + 1)] == [q + 1] * r + [q] * (k + 1 - r)
            assert a.num_patterns == 1 + k + 1
            for j in range(k + 1):
                assert a.pattern(first + j)[0] == pat[b[j]:b[j + 1]]
                if k:
                    assert a.pattern_approx(first + j) == (0, j, b[j], n - b[j + 1])
            assert a.pattern_approx(0) is None
            if k:
                assert a.num_approx == 1 and a.approx(0) == (first, pat, k, n, 0)
                assert a.approx_reach == (n, n - b[1])
            else:
                assert a.num_approx == 0 and a.pattern_approx(first) is None and a.approx_reach == (0, 0)
            a.close()


def test_limits_and_errors_leave_nothing_applied():
    lib = _lib.load()
    a = Automaton()
    a.add(b"abc", 1)

    def rc(p, n, k, flags=0, h=None):
        return lib.acm_automaton_add_approx(a.h if h is None else h, p, n, k, 9, flags)
    big = bytes(5000)
    limit = rc(big, 4097, 1)
    assert limit < 0 and limit != ERR_ARG                       # ACM_ERR_LIMIT
    assert rc(big, 100, 16) == limit
    assert rc(big, 3, 3) == ERR_ARG and rc(big, 1, 1) == ERR_ARG and rc(big, 0, 1) == ERR_ARG    # n < k + 1
    assert rc(big, 10, -1) == ERR_ARG and rc(None, 4, 1) == ERR_ARG and rc(big, -1, 0) == ERR_ARG
    assert rc(big, 10, 2, flags=2) == ERR_ARG and rc(big, 10, 0, flags=4) == ERR_ARG
    assert lib.acm_automaton_add_approx(None, big, 10, 2, 0, 0) == ERR_ARG
    assert a.num_patterns == 1 and a.num_approx == 0 and a.approx_reach == (0, 0)
    # the limits themselves are legal
    assert a.add_approx(big[:4096], 15, 3) == 1 and a.num_patterns == 17
    assert a.add_approx(b"0123456789abcdef", 15) == 17 and a.num_patterns == 33
    assert a.approx_reach == (4096, 4096 - 256)
    with pytest.raises(AcmError):
        a.approx(2)
    with pytest.raises(AcmError):
        a.pattern_approx(33)
    assert lib.acm_automaton_approx(a.h, -1, None, None, None, None, None, None) == ERR_ARG
    assert lib.acm_automaton_approx(a.h, 1, None, None, None, None, None, None) == 0
    assert lib.acm_automaton_approx_reach(None, None, None) == ERR_ARG
    a.compile()
    assert rc(b"abcdef", 6, 1) == ERR_ARG and rc(b"abcdef", 6, 0) == ERR_ARG       # a compiled automaton
    assert a.num_patterns == 33 and a.num_approx == 2
    with pytest.raises(AcmError):
        a.add_approx(b"abcdef", 1)
    a.close()


def test_k0_is_add_ex_and_flags():
    a, b = Automaton(), Automaton()
    for i, (p, nc) in enumerate([(b"hello", False), (b"World", True), (b"", False), (b"x", False)]):
        assert a.add_approx(p, 0, iid=i, nocase=nc) == i
        b.add(p, i, nocase=nc)
    assert a.num_approx == 0
    for i in range(4):
        assert a.pattern(i) == b.pattern(i) and a.pattern_flags(i) == b.pattern_flags(i)
    a.compile()
    b.compile()
    assert a.mixed_case and np.array_equal(a.reference_table(), b.reference_table())
    # a folding approximate pattern: every piece carries the flag, and the bytes stay as added
    c = Automaton()
    f = c.add_approx(b"HelloWorld", 2, iid=3, nocase=True)
    assert [c.pattern_flags(f + j) for j in range(3)] == [_lib.PATTERN_NOCASE] * 3
    assert c.approx(0) == (0, b"HelloWorld", 2, 3, _lib.PATTERN_NOCASE)
    assert [c.pattern(j)[0] for j in range(3)] == [b"Hell", b"oWo", b"rld"] and [c.pattern(j)[1] for j in range(3)] == [3] * 3
    c.compile()
    assert c.nocase and not c.mixed_case
    for x in (a, b, c):
        x.close()


def test_compile_sees_the_pieces_alone():
    """an automaton with approximate patterns is the automaton of their pieces; one without any is what it was"""
    lib = _lib.load()
    text, pats = planted_case()
    model = am.ApproxModel(pats)
    a = Automaton()
    for x, (p, k) in enumerate(pats):
        assert a.add_approx(p, k, iid=x) == model.first[x]
    a.compile()
    plain = model.a
    assert a.num_approx == len(pats) and a.num_patterns == plain.num_patterns and a.num_states == plain.num_states
    assert np.array_equal(a.reference_table(), plain.reference_table())
    assert a.byte_classes()[0] == plain.byte_classes()[0] and np.array_equal(a.byte_classes()[1], plain.byte_classes()[1])
    st = [(C.c_uint32 * 21)(), (C.c_uint32 * 21)()]
    assert lib.acm_sieve_selftest(plain.h, st[0]) == lib.acm_sieve_selftest(a.h, st[1])
    assert list(st[0]) == list(st[1])
    for i in range(a.num_patterns):
        assert a.pattern_approx(i)[:2] == (model.owner[i], model.piece[i])
    assert a.approx_reach == (32, 32 - am.piece_bounds(32, 15)[1])
    a.close()


# ------------------------------------------------------------------ the rule against brute force


def test_model_against_brute_force():
    text, pats = planted_case()
    model = am.ApproxModel(pats)
    brute = am.brute_force(pats, [text])
    assert model.matches([text]) == brute
    # the classes the rule tells apart all occur
    p, o = model.all_entries(text)
    full = text
    matches = several = over = shadowed = 0
    for pp, oo in zip(p.tolist(), o.tolist()):
        x, s = model.span(pp, oo)
        w, j = model.pats[x], model.piece[pp]
        if s < 0 or s + w.n > len(full):
            continue
        mis = w.mismatches(full[s:s + w.n])
        m = [int(mis[w.bounds[i]:w.bounds[i + 1]].sum()) for i in range(w.k + 1)]
        assert m[j] == 0
        if sum(m) > w.k:
            over += 1
        elif any(x == 0 for x in m[:j]):
            shadowed += 1
        else:
            matches += 1
            several += sum(1 for x in m if x == 0) > 1
    print("candidates %d matches %d with several exact pieces %d over budget %d" % (p.size, matches, several, over))
    assert p.size > 0 and matches == len(brute) > 0 and several > 0 and over > 0 and shadowed > 0
    by = {}
    for x, s, d in brute:
        by.setdefault(x, set()).add(d)
    assert any(by.get(x, set()) == set(range(k + 1)) for x, (_, k) in enumerate(pats) if k <= 3)
    assert all(x in by for x in range(len(pats))), "the planted copies make every pattern match"


def test_model_folds_like_the_library():
    """the fold is case_fold.h's: a..z only, '@' and '`', '[' and '{' stay different"""
    pats = [(b"a@[z", 1, True), (b"A`{Z", 1, True), (b"a@[z", 1, False)]
    texts = [b"A@[Z a`[z A`{z a@{Z .@[z a@[. A@[Z"]
    model = am.ApproxModel(pats)
    brute = am.brute_force(pats, texts)
    assert model.matches(texts) == brute
    d0 = {x: sorted(s for y, s, d in brute if y == x and d == 0) for x in range(3)}
    assert d0[0] == [0, 30] and d0[1] == [10] and d0[2] == []
    assert am.fold(b"az@`[{\xe1") == b"AZ@`[{\xe1"
