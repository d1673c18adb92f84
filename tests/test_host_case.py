"""Case sensitivity per pattern on the host (acm_automaton_add_ex and friends) -- no GPU: the flags, what
compile makes of them (nocase, mixed or unchanged automata), the Python model of the case pass
(tests/case_model.py) against a brute force, and the slice compares of the compare sweep
(tests/case_compare.py) against the model."""
import ctypes as C

import numpy as np
import pytest

import case_compare as cc
import case_model as cm
from gpu_pattern_matching_amd import AcmError, Automaton, _lib

WORDS = [(b"abc", False), (b"ABC", False), (b"aBc", True), (b"b", False), (b"C", True), (b"", False), (b"bca", True),
         (b"a@b", False), (b"a`b", False), (b"[ab{", True), (b"\xe1b\xc1", False), (b"cabcab", False), (b"BCABCA", True)]
LONG = [(b"abcabca", False), (b"Abcabcab", True), (b"aBcabcabc", False), (b"abc", True), (b"ABc", False),
        (b"bcabcabcabcabcab", False)]


def sieve_stats(lib, a):
    st = (C.c_uint32 * 21)()
    rc = lib.acm_sieve_selftest(a.h, st)
    return rc, list(st)


@pytest.mark.parametrize("seed", range(6))
def test_model_against_brute_force(lib, seed):
    rng = np.random.default_rng(seed)
    model = cm.CaseModel(WORDS)
    alphabet = np.frombuffer(b"abcABC@`[{\xe1\xc1", dtype=np.uint8)
    for n in (0, 1, 2, 5, 40, 300):
        text = bytes(rng.choice(alphabet, size=n, p=[.2, .2, .2, .08, .08, .08, .03, .03, .025, .025, .025, .025]))
        for before in (b"", b"a", b"cabca"):
            exp = cm.brute_force(WORDS, text, before)
            init = model.walk(before)[2]
            offs, pats, _ = model.records(text, True, init_state=init, before=before)
            got = list(zip(offs.tolist(), pats.tolist()))
            assert len(got) == len(set(got)) and set(got) == exp, (n, before)
            assert offs.tolist() == sorted(offs.tolist())
            ho, hp, _ = model.records(text, False, init_state=init, before=before)
            first = {}
            for o, p in got:
                first.setdefault(o, p)
            assert list(zip(ho.tolist(), hp.tolist())) == sorted(first.items())
    # most candidates fail, and some hold: the texts tell the rules apart
    text = bytes(rng.choice(alphabet[:6], size=400))
    every = cm.CaseModel([(p, True) for p, _ in WORDS]).records(text, True)[0].size
    kept = model.records(text, True)[0].size
    assert 0 < kept < every


def test_model_before_and_origin(lib):
    model = cm.CaseModel([(b"abc", False), (b"BC", True)])
    s = model.walk(b"xab")[2]
    # the exact pattern reaches back into before: kept with it, dropped without; the caseless one stays
    o, p, _ = model.records(b"c..", True, init_state=s, before=b"ab", origin=100)
    assert sorted(zip(o.tolist(), p.tolist())) == [(100, 0), (100, 1)]
    o, p, _ = model.records(b"c..", True, init_state=s, before=b"b", origin=100)
    assert list(zip(o.tolist(), p.tolist())) == [(100, 1)]
    o, p, _ = model.records(b"c..", True, init_state=s, before=b"Ab", origin=100)
    assert list(zip(o.tolist(), p.tolist())) == [(100, 1)]
    pl = cm.planes([5, 6, 7], [1, 2, 3], 4, -7, 9)
    assert pl[0].tolist() == [3, 5, 6, 9] and pl[1].tolist() == [3, 1, 2, 9]
    assert cm.planes([5], [1], 5, -7, 9)[0].tolist() == [1, 5, 9, -7, -7]


def test_compare_sweep_expectations(lib):
    """what tests/test_gpu_case_compare.py expects of the device, without one: the slice compares of
    case_compare equal CaseModel.filter on the same planes, texts and befores, in both forms; an unaltered copy
    keeps every suffix (brute_force); an entry is kept iff no altered byte lies under it"""
    model = cm.CaseModel(cc.PATS)
    state_of = {"M": model.walk(cc.M)[2], "M13": model.walk(cc.M13)[2]}
    lists = {s: model.list_of(s) for s in state_of.values()}
    assert set(lists[state_of["M"]]) == cc.OF_M and set(lists[state_of["M13"]]) == cc.OF_M13
    assert len(lists[state_of["M"]]) == len(cc.OF_M) and len(lists[state_of["M13"]]) == len(cc.OF_M13)
    # the unaltered copies, with no automaton at all
    for master, name, of in ((cc.M, "M", cc.OF_M), (cc.M13, "M13", cc.OF_M13)):
        text = b".;" + master + b"-"
        end = 1 + len(master)
        at_end = {p for o, p in cm.brute_force(cc.PATS, text) if o == end}
        assert at_end == of
        ep, eo = cc.expect(cc.PATS, lists, [(state_of[name], end)], text, 0, len(text), True)
        assert set(ep.tolist()) == of and ep.tolist() == lists[state_of[name]] and set(eo.tolist()) == {end}
        assert cc.expect(cc.PATS, lists, [(state_of[name], end)], text, 0, len(text), False)[0].tolist() == ep.tolist()[:1]
    # text only
    text, copies = cc.text_only()
    assert len(copies) == 4 * 2 * 34 and {(o - 32) % 4 for o, _, _ in copies} == {0, 1, 2, 3}
    sM = state_of["M"]
    for origin in (0, 1001):
        records = [(sM, origin + o) for o, _, _ in copies]
        for all_patterns in (False, True):
            ep, eo = cc.expect(cc.PATS, lists, records, text, origin, origin + len(text), all_patterns)
            mp, mo = model.filter([s for s, _ in records], [o for _, o in records], text, all_patterns, origin)
            assert np.array_equal(ep, mp) and np.array_equal(eo, mo), (origin, all_patterns)
    kept = {}
    for p, o in zip(ep.tolist(), (eo - origin).tolist()):
        kept.setdefault(o, set()).add(p)
    for o, j, bit in copies:
        under = {p for p in cc.OF_M if cc.PATS[p][1] or j is None or j < 33 - len(cc.PATS[p][0])}
        assert kept[o] == under, (o, j, bit)
    # across the seam
    seen = set()
    for seam in cc.seams_13() + cc.seams_33():
        for origin in (0, 1001):
            records = seam.records(state_of, origin)
            for all_patterns in (False, True):
                ep, eo = seam.expect(lists, state_of, origin, all_patterns)
                mp, mo = model.filter([s for s, _ in records], [o for _, o in records], seam.text, all_patterns, origin,
                                      seam.before)
                assert np.array_equal(ep, mp) and np.array_equal(eo, mo), (seam.name, seam.k, seam.j, seam.mode)
        first = eo == records[0][1]
        longest = max(cc.OF_M if seam.name == "M" else cc.OF_M13, key=lambda p: len(cc.PATS[p][0]))
        assert (longest in ep[first].tolist()) == (seam.j is None and (seam.mode != "fewer" or seam.k == 0))
        assert int((~first).sum()) == 2 * len(cc.OF_M) + len(cc.OF_M13)       # the plain matches behind the seam
        seen.add((seam.name, seam.k, seam.j, seam.mode))
    assert len(seen) == 14 * 14 * 3 - 14 + 34 * 3 - 2


def test_flags_round_trip(lib):
    a = Automaton()
    a.add(b"abc", 3)
    a.add(b"DEF", 4, nocase=True)
    a.add(b"", 5, nocase=True)
    assert [a.pattern_flags(i) for i in range(3)] == [0, _lib.PATTERN_NOCASE, _lib.PATTERN_NOCASE]
    assert not a.mixed_case            # not compiled yet
    a.compile()
    assert [a.pattern_flags(i) for i in range(3)] == [0, 1, 1]
    assert a.iids().tolist() == [3, 4, 5]
    for bad in (-1, 3):
        assert lib.acm_automaton_pattern_flags(a.h, bad) == -1
        with pytest.raises(AcmError):
            a.pattern_flags(bad)
    assert lib.acm_automaton_pattern_flags(None, 0) == -1
    assert lib.acm_automaton_mixed_case(None) == 0


def test_unknown_flag_and_add_after_compile(lib):
    a = Automaton()
    for flags in (2, 3, 0x80000000):
        assert lib.acm_automaton_add_ex(a.h, b"abc", 3, 0, flags) == -1
    assert a.num_patterns == 0
    assert lib.acm_automaton_add_ex(a.h, b"abc", 3, 0, 1) == 0
    assert lib.acm_automaton_add_ex(a.h, None, 3, 0, 0) == -1
    assert lib.acm_automaton_add_ex(a.h, b"abc", -1, 0, 0) == -1
    a.compile()
    with pytest.raises(AcmError) as e:
        a.add(b"x", nocase=True)
    assert e.value.code == -1 and "compiled" in str(e.value)
    with pytest.raises(AcmError) as e2:
        a.add(b"x")
    assert str(e2.value).split(":", 1)[1] == str(e.value).split(":", 1)[1]
    assert a.num_patterns == 1


@pytest.mark.parametrize("pats", [LONG, [(p, nc) for p, nc in WORDS if len(p) != 1]], ids=["long", "words"])
def test_all_flagged_is_the_nocase_automaton(lib, pats):
    flagged = cm.build([(p, True) for p, _ in pats])
    whole = cm.build([(p, False) for p, _ in pats], nocase=True)
    both = cm.build(pats, nocase=True)       # set_nocase(1): the flags do not matter
    for a in (flagged, both):
        assert a.nocase and not a.mixed_case
        assert np.array_equal(a.reference_table(), whole.reference_table())
        assert sieve_stats(lib, a) == sieve_stats(lib, whole)
        assert a.byte_classes()[0] == whole.byte_classes()[0]
        assert np.array_equal(a.byte_classes()[1], whole.byte_classes()[1])
        assert [a.pattern(i) for i in range(a.num_patterns)] == [whole.pattern(i) for i in range(a.num_patterns)]
    assert sieve_stats(lib, whole)[0] == (1 if all(len(p) >= 3 for p, _ in pats) else 0)


def test_unflagged_is_todays_automaton(lib):
    plain = Automaton()
    for i, (p, _) in enumerate(LONG):
        check = lib.acm_automaton_add(plain.h, p, len(p), i)
        assert check == 0
    plain.compile()
    ex = cm.build([(p, False) for p, _ in LONG])
    assert not ex.nocase and not ex.mixed_case and not plain.nocase and not plain.mixed_case
    assert np.array_equal(ex.reference_table(), plain.reference_table())
    assert sieve_stats(lib, ex) == sieve_stats(lib, plain)
    # and it is case-sensitive: not the nocase table
    assert not np.array_equal(ex.reference_table(), cm.build([(p, True) for p, _ in LONG]).reference_table())


def test_mixed(lib):
    a = cm.build(LONG)
    whole = cm.build([(p, False) for p, _ in LONG], nocase=True)
    assert a.mixed_case and not a.nocase
    assert np.array_equal(a.reference_table(), whole.reference_table())
    assert [a.pattern(i)[0] for i in range(a.num_patterns)] == [p for p, _ in LONG]
    assert [a.state_matches(s) for s in range(a.num_states)] == [whole.state_matches(s) for s in range(whole.num_states)]
    st = (C.c_uint32 * 9)()
    assert lib.acm_compact_selftest(a.h, 0, st) == 1
    rc, stats = sieve_stats(lib, a)
    assert rc == 1 and stats == sieve_stats(lib, whole)[1]
    # an empty pattern does not decide: flagged or not, with the others all flagged the automaton is nocase
    b = cm.build([(b"abc", True), (b"", False)])
    assert b.nocase and not b.mixed_case
    c = cm.build([(b"abc", False), (b"", True)])
    assert not c.nocase and not c.mixed_case


def test_load_file_ex_appends(lib, tmp_path):
    exact, loose = tmp_path / "exact.txt", tmp_path / "loose.txt"
    exact.write_bytes(b"Alpha\nbeta\n")
    loose.write_bytes(b"Gamma\ndelta\nEps\n")
    a = Automaton()
    assert a.load_file(exact) == 2
    assert a.load_file(loose, nocase=True) == 3
    assert lib.acm_automaton_load_file_ex(a.h, str(loose).encode(), 0, -1, 4) == -1
    assert a.num_patterns == 5
    a.compile()
    assert [a.pattern(i)[0] for i in range(5)] == [b"Alpha", b"beta", b"Gamma", b"delta", b"Eps"]
    assert [a.pattern_flags(i) for i in range(5)] == [0, 0, 1, 1, 1]
    assert a.mixed_case
    hx = tmp_path / "hex.txt"
    hx.write_bytes(b"4142\n")
    h = Automaton()
    assert lib.acm_automaton_load_file_ex(h.h, str(hx).encode(), 1, -1, 1) == 1
    assert h.pattern(0)[0] == b"AB" and h.pattern_flags(0) == 1
