"""Edit patterns on the host (acm_automaton_add_edit, acm_automaton_approx_mode, the reach) and the model of
tests/edit_model.py against a brute-force Sellers matrix that knows nothing of pieces.  No GPU."""
import numpy as np
import pytest

import approx_model as am
import edit_model as em
from edit_model import Edit
from gpu_pattern_matching_amd import AcmError, Automaton, _lib

ERR_ARG = -1

# k = 1 .. 4 at n = k + 1 (pieces of one byte), 3 (k + 1) and an uneven length
PLANTED = [Edit(b"ab", 1), Edit(b"abcabc", 1), Edit(b"cab", 2), Edit(b"bcaabcbac", 2), Edit(b"abca", 3),
           Edit(b"cbabcaabbcac", 3), Edit(b"bcabc", 4), Edit(b"acbbcabacabccba", 4), Edit(b"abcbacbcabcabacbb", 2)]


def test_errors_and_limits_leave_nothing_applied():
    lib = _lib.load()
    a = Automaton()
    a.add(b"abc", 1)

    def rc(p, n, k, flags=0, h=None):
        return lib.acm_automaton_add_edit(a.h if h is None else h, p, n, k, 9, flags)
    big = bytes(5000)
    limit = rc(big, 4097, 1)
    assert limit < 0 and limit != ERR_ARG                       # ACM_ERR_LIMIT
    assert rc(big, 100, 5) == limit and rc(big, 100, 15) == limit and rc(big, 100, 16) == limit
    assert rc(big, 3, 3) == ERR_ARG and rc(big, 1, 1) == ERR_ARG and rc(big, 0, 1) == ERR_ARG    # n < k + 1
    assert rc(big, 10, -1) == ERR_ARG and rc(None, 4, 1) == ERR_ARG and rc(big, -1, 0) == ERR_ARG
    assert rc(big, 10, 2, flags=2) == ERR_ARG and rc(big, 10, 0, flags=4) == ERR_ARG
    assert lib.acm_automaton_add_edit(None, big, 10, 2, 0, 0) == ERR_ARG
    assert a.num_patterns == 1 and a.num_approx == 0 and a.approx_reach == (0, 0)
    assert lib.acm_automaton_approx_mode(a.h, 0) == ERR_ARG and lib.acm_automaton_approx_mode(None, 0) == ERR_ARG
    # the limits themselves are legal
    assert a.add_edit(big[:4096], 4, 3) == 1 and a.num_patterns == 6
    assert a.add_edit(b"01234", 4) == 6 and a.num_patterns == 11
    assert a.approx_reach == (4096 + 8, 4096 - 820 + 4)         # pieces of 820, 819, ..: n + 2k, post + k
    with pytest.raises(AcmError):
        a.approx_mode(2)
    a.compile()
    assert rc(b"abcdef", 6, 1) == ERR_ARG and rc(b"abcdef", 6, 0) == ERR_ARG       # a compiled automaton
    with pytest.raises(AcmError):
        a.add_edit(b"abcdef", 1)
    assert a.num_patterns == 11 and a.num_approx == 2
    a.close()


def test_pieces_are_add_approx_s_and_the_mode():
    for k in range(1, 5):
        for n in (k + 1, 3 * (k + 1), 17, 64):
            pat = bytes((7 * i + k) % 251 for i in range(n))
            a, b = Automaton(), Automaton()
            for x in (a, b):
                x.add(b"zz", 5)
            assert a.add_edit(pat, k, iid=n) == b.add_approx(pat, k, iid=n) == 1
            assert a.num_patterns == b.num_patterns == k + 2 and a.num_approx == b.num_approx == 1
            assert a.approx(0) == b.approx(0) == (1, pat, k, n, 0)
            for i in range(a.num_patterns):
                assert a.pattern(i) == b.pattern(i) and a.pattern_approx(i) == b.pattern_approx(i)
            assert (a.approx_mode(0), b.approx_mode(0)) == (1, 0)
            bounds = am.piece_bounds(n, k)
            assert b.approx_reach == (n, n - bounds[1]) and a.approx_reach == (n + 2 * k, n - bounds[1] + k)
            a.compile()
            b.compile()
            assert np.array_equal(a.reference_table(), b.reference_table())
            a.close()
            b.close()


def test_reach_grows_for_edit_patterns_only():
    a = Automaton()
    a.add_approx(b"abcdefghijklmnopqrst", 3)      # n = 20, post = 15
    assert a.approx_reach == (20, 15)
    a.add_edit(b"abcdefgh", 2)                    # 8 + 4, 5 + 2: smaller
    assert a.approx_reach == (20, 15) and [a.approx_mode(x) for x in range(2)] == [0, 1]
    a.add_edit(b"abcdefghijklmnopqr", 1, nocase=True)   # 18 + 2, 9 + 1
    assert a.approx_reach == (20, 15)
    a.add_edit(b"abcdefghijklmnopqrs", 1)         # 19 + 2, 9 + 1
    assert a.approx_reach == (21, 15)
    assert a.approx(2)[4] == _lib.PATTERN_NOCASE
    a.close()


def test_k0_is_a_plain_add():
    a, b = Automaton(), Automaton()
    for i, (p, nc) in enumerate([(b"hello", False), (b"World", True), (b"", False), (b"x", False)]):
        assert a.add_edit(p, 0, iid=i, nocase=nc) == i
        b.add(p, i, nocase=nc)
    assert a.num_approx == 0 and a.approx_reach == (0, 0)
    for i in range(4):
        assert a.pattern(i) == b.pattern(i) and a.pattern_flags(i) == b.pattern_flags(i) and a.pattern_approx(i) is None
    a.compile()
    b.compile()
    assert np.array_equal(a.reference_table(), b.reference_table())
    a.close()
    b.close()


def test_a_set_without_edit_patterns_is_what_it_was():
    pats = [(b"abcabc", 1), (b"bcabcaabc", 2), (b"cab", 0)]
    a, b = Automaton(), Automaton()
    for x, (p, k) in enumerate(pats):
        a.add_approx(p, k, iid=x)
        b.add_approx(p, k, iid=x)
    b.add_edit(b"zz", 0, iid=9)                   # k == 0 through the new call: a plain pattern
    a.add(b"zz", 9)
    a.compile()
    b.compile()
    assert np.array_equal(a.reference_table(), b.reference_table())
    assert a.approx_reach == b.approx_reach == (9, 6) and [b.approx_mode(x) for x in range(2)] == [0, 0]
    c = Automaton()
    c.add(b"abc", 0)
    assert c.approx_reach == (0, 0) and c.num_approx == 0
    for x in (a, b, c):
        x.close()


# ------------------------------------------------------------------ the model against brute force


def test_sellers_by_hand():
    C = em.sellers(b"abc", b"xabcx")
    assert C[3].tolist() == [3, 3, 2, 1, 0, 1] and C[0].tolist() == [0] * 6 and C[:, 0].tolist() == [0, 1, 2, 3]
    assert em.sellers(b"abc", b"ABC")[3][3] == 3 and em.sellers(b"abc", b"ABC", nocase=True)[3][3] == 0
    assert em.sellers(b"abc", b"xabc", anchored=True)[3].tolist() == [3, 3, 3, 2, 1]
    assert em.shortest(b"abc", b"zzabc", 0) == 3 and em.shortest(b"abc", b"zzac", 1) == 2 and em.shortest(b"abc", b"ab", 1) == 2
    assert em.sellers(b"abc", b"zzzzzz", limit=1) is None


def test_model_against_brute_force_on_planted_texts():
    text, where = em.planted(PLANTED)
    model = em.EditModel(PLANTED)
    gp, ge, gd, gl, und, cands = model.scan([text])
    assert und == 0 and cands > gp.size > 0
    recs = [(model.owner[p], e, d, ln) for p, e, d, ln in zip(gp.tolist(), ge.tolist(), gd.tolist(), gl.tolist())]
    near = em.check(PLANTED, [text], recs)
    assert near >= len(recs)
    # every planted copy within the budget is found at its own end, the indels with a span that is not n bytes
    D, _ = em.brute_force(PLANTED, [text])
    by = {(x, e + 1): (d, ln) for x, e, d, ln in recs}
    lengths = set()
    for x, name, at, v in where:
        p, e = model.pats[x], at + len(v)
        if name == "over budget":
            continue
        assert D[x][e] <= p.k, (x, name)
        hit = [by[(x, f)] for f in range(e - 2 * p.k, e + 2 * p.k + 1) if (x, f) in by]
        assert hit and min(hit)[0] <= D[x][e], (x, name, at)
        if name == "exact":
            assert by[(x, e)] == (0, p.n)
        lengths |= {ln - p.n for _, ln in hit}
    assert min(lengths) < 0 < max(lengths)


def test_indels_are_what_the_hamming_rule_misses():
    """a dropped, a doubled and a padded byte are one error each to the edit rule and shift every byte behind them
    for the Hamming rule, which finds only the copies with substitutions"""
    A, k = b"thequickbrownfox", 2
    copies = [A, A[:5] + A[6:], A[:9] + b"w" + A[9:], A[1:], A[:3] + b"#" + A[3:12] + A[13:], A[:7] + b"#" + A[8:]]
    text = b"....".join(copies) + b"...."
    ends, at = [], 0
    for c in copies:
        ends.append(at + len(c) - 1)
        at += len(c) + 4
    model = em.EditModel([Edit(A, k)])
    gp, ge, gd, gl, und, _ = model.scan([text])
    recs = list(zip(ge.tolist(), gd.tolist(), gl.tolist()))
    assert und == 0 and em.check([Edit(A, k)], [text], [(0,) + r for r in recs]) >= 6
    got = dict((e, (d, ln)) for e, d, ln in recs)
    assert [got.get(e) for e in ends] == [(0, 16), (1, 15), (1, 17), (1, 15), (2, 16), (1, 16)]
    ham = {s + 15 for _, s, _ in am.ApproxModel([(A, k)]).matches([text])}
    assert ham == {ends[0], ends[3], ends[5]}          # (a first byte dropped is a substituted one with the byte in front)


def test_model_with_two_texts_and_folding():
    pats = [Edit(b"AbCaBc", 1, True), Edit(b"bcaabc", 2), (b"abcab", 1), b"ca"]
    texts = [b"xabcabcxaBcbcx", b"", b"bcabcabcaabcabc", b"abcab", b"c"]
    model = em.EditModel(pats)
    gp, ge, gd, gl, und, _ = model.scan(texts)
    recs = [(model.owner[p], e, d, ln) for p, e, d, ln in zip(gp.tolist(), ge.tolist(), gd.tolist(), gl.tolist())]
    assert und == 0 and em.check(pats, texts, recs) > 4
    assert {x for x, *_ in recs} == {0, 1, 2, 3}
    # the Hamming pattern's records are approx_model's, normalised
    want = {(2, s + 4, d, 5) for x, s, d in am.brute_force([(b"abcab", 1)], texts)}
    assert {r for r in recs if r[0] == 2} == want
