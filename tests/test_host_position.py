"""Position constraints per pattern on the host (acm_automaton_set_position and friends) -- no GPU: the
windows, their argument errors, the position file, that compile does not see them, and the Python model of
the position pass (tests/position_model.py) against a brute force."""
import ctypes as C

import numpy as np
import pytest

import position_model as pm
from gpu_pattern_matching_amd import AcmError, Automaton, _lib

PATS = [b"abc", b"ab", b"b", b"abc", b"cab", b"a", b"aa", b"aaa", b"aaaa", b"", b"bca", b"abc"]


def sieve_stats(lib, a):
    st = (C.c_uint32 * 21)()
    rc = lib.acm_sieve_selftest(a.h, st)
    return rc, list(st)


def test_round_trip_and_defaults(lib):
    a = Automaton()
    for i, p in enumerate(PATS):
        a.add(p, i)
    assert not a.positioned
    assert all(a.position(i) == (0, None, False) for i in range(len(PATS)))
    a.set_position(0, 5, 9)
    assert a.positioned and a.position(0) == (5, 9, False)
    a.set_position(0)                                   # back to the default: no constraint
    assert not a.positioned and a.position(0) == (0, None, False)
    a.compile()                                         # after compile as well
    a.set_position(3, 3, 3, from_end=True)
    a.set_position(4, 7, 2)                             # lo > hi is legal
    a.set_position(5, 0, None, from_end=True)           # a constraint: not the default triple
    a.set_position(6, 0, 0)
    a.set_position(7, 0x7FFFFFFE, None)
    assert a.position(3) == (3, 3, True) and a.position(4) == (7, 2, False)
    assert a.position(5) == (0, None, True) and a.position(6) == (0, 0, False)
    assert a.position(7) == (0x7FFFFFFE, None, False)
    assert a.positioned
    for i in (3, 4, 6, 7):
        a.set_position(i)
    assert a.positioned                                 # (0, unbounded, from_end) still is one
    a.set_position(5)
    assert not a.positioned
    lo, hi, fl = C.c_int32(7), C.c_int32(7), C.c_uint(7)
    assert lib.acm_automaton_pattern_position(a.h, 1, lo, hi, fl) == 0
    assert (lo.value, hi.value, fl.value) == (0, _lib.POS_UNBOUNDED, 0)
    assert lib.acm_automaton_pattern_position(a.h, 1, None, None, None) == 0
    assert lib.acm_automaton_positioned(None) == 0


def test_argument_errors(lib):
    a = Automaton()
    a.add(b"abc")
    a.add(b"de")
    for args in ((-1, 0, 5, 0), (2, 0, 5, 0), (0, -1, 5, 0), (0, 0, -1, 0), (0, -2 ** 31, 0, 0), (0, 0, 5, 2),
                 (0, 0, 5, 3), (0, 0, 5, 0x80000000)):
        assert lib.acm_automaton_set_position(a.h, *args) == -1, args
        assert lib.acm_last_error()
    assert lib.acm_automaton_set_position(None, 0, 0, 5, 0) == -1
    assert not a.positioned and a.position(0) == (0, None, False)
    for bad in (-1, 2):
        assert lib.acm_automaton_pattern_position(a.h, bad, None, None, None) == -1
        with pytest.raises(AcmError):
            a.position(bad)
    assert lib.acm_automaton_pattern_position(None, 0, None, None, None) == -1
    with pytest.raises(AcmError) as e:
        a.set_position(0, -3)
    assert e.value.code == -1
    assert lib.acm_automaton_load_position_file(None, b"x") == -1
    assert lib.acm_automaton_load_position_file(a.h, None) == -1


def test_position_file(lib, tmp_path):
    a = Automaton()
    for i, p in enumerate(PATS[:5]):
        a.add(p, i)
    good = tmp_path / "good.pos"
    good.write_bytes(b"# windows\n\n0 0 0\n  1 4 *  \n2 3 3 end\n\t3\t10\t2147483647\r\n   # indented comment\n4 0 * end\n0 2 7\n")
    assert a.load_position_file(good) == 6
    assert a.position(0) == (2, 7, False)               # the later line wins
    assert a.position(1) == (4, None, False) and a.position(2) == (3, 3, True)
    assert a.position(3) == (10, None, False) and a.position(4) == (0, None, True)
    empty = tmp_path / "empty.pos"
    empty.write_bytes(b"# nothing\n\n")
    assert a.load_position_file(empty) == 0
    bad_lines = [b"5 0 0", b"-1 0 0", b"0 -1 5", b"0 1", b"0", b"x 1 2", b"0 1 2 start", b"0 1 2 end end", b"0 1 2 3",
                 b"0 1 **", b"0 1 2147483648", b"0 1 2x", b"0 1 *end", b"0x1 1 2", b"99999999999 0 0"]
    for k, line in enumerate(bad_lines):
        b = Automaton()
        for i, p in enumerate(PATS[:5]):
            b.add(p, i)
        f = tmp_path / ("bad%d.pos" % k)
        f.write_bytes(b"# c\n1 1 1\n" + line + b"\n2 2 2\n")
        with pytest.raises(AcmError) as e:
            b.load_position_file(f)
        assert e.value.code == -7, line
        assert "%s:3:" % f in str(e.value), (line, str(e.value))
        assert not b.positioned, line                    # nothing of a bad file is applied
    with pytest.raises(AcmError) as e:
        a.load_position_file(tmp_path / "missing.pos")
    assert e.value.code == -6


@pytest.mark.parametrize("pats", [[b"abcd", b"bcde", b"abc", b"cdefgh"], PATS], ids=["sparse", "chain"])
def test_compile_does_not_see_windows(lib, pats):
    windows = {0: (0, 0, False), 1: (3, 9, True), 2: (5, 2, False)}
    plain = pm.build(pats, {})
    before = Automaton()
    for i, p in enumerate(pats):
        before.add(p, i)
    for i, w in windows.items():
        before.set_position(i, *w)
    before.compile()
    after = pm.build(pats, windows)
    assert not plain.positioned and before.positioned and after.positioned
    for a in (before, after):
        assert np.array_equal(a.reference_table(), plain.reference_table())
        assert sieve_stats(lib, a) == sieve_stats(lib, plain)
        assert a.byte_classes()[0] == plain.byte_classes()[0]
        assert [a.state_matches(s) for s in range(a.num_states)] == [plain.state_matches(s) for s in range(plain.num_states)]
        st1, st2 = (C.c_uint32 * 9)(), (C.c_uint32 * 9)()
        assert lib.acm_compact_selftest(a.h, 0, st1) == lib.acm_compact_selftest(plain.h, 0, st2)
        assert list(st1) == list(st2)
    assert sieve_stats(lib, plain)[0] == (1 if all(len(p) >= 3 for p in pats) else 0)


def random_windows(rng, n, share=0.7):
    w = {}
    for i in range(n):
        if rng.random() < share:
            lo = int(rng.integers(0, 8))
            hi = None if rng.random() < 0.25 else int(rng.integers(0, 12))
            w[i] = (lo, hi, bool(rng.random() < 0.5))
    return w


@pytest.mark.parametrize("seed", range(8))
def test_model_against_brute_force(lib, seed):
    """duplicated byte strings with different windows (abc three times) and the suffix chain a, aa, aaa, aaaa"""
    rng = np.random.default_rng(seed)
    windows = random_windows(rng, len(PATS))
    windows[0], windows[3], windows[11] = (0, 1, False), (2, 5, False), (3, 4, True)
    model = pm.PositionModel(PATS, windows)
    alphabet = np.frombuffer(b"abc", dtype=np.uint8)
    texts = [bytes(rng.choice(alphabet, size=n, p=[.5, .3, .2])) for n in (0, 1, 2, 3, 0, 7, 19, 40, 0)]
    exp = pm.brute_force(PATS, windows, texts)
    offs, pats, _, und = model.records(texts, True)
    got = list(zip(offs.tolist(), pats.tolist()))
    assert und == 0 and len(got) == len(set(got)) and set(got) == exp
    assert offs.tolist() == sorted(offs.tolist())
    every = pm.PositionModel(PATS, {}).records(texts, True)
    assert 0 < len(got) < every[0].size
    assert set(zip(every[0].tolist(), every[1].tolist())) == pm.brute_force(PATS, {}, texts)
    # the first form: the first kept entry of each offset, in the order of the state's match list
    ho, hp, _, _ = model.records(texts, False)
    first = {}
    for o, p in got:
        first.setdefault(o, p)
    assert list(zip(ho.tolist(), hp.tolist())) == sorted(first.items())
    # an unknown end: the end-anchored entries of the last text are undecided, everything else stands
    o2, p2, _, und2 = model.records(texts[:-1], True, open_end=None)
    base = sum(len(t) for t in texts[:-2])
    exp2 = {(o, p) for o, p in pm.brute_force(PATS, windows, texts[:-1]) if o < base or not (p in windows and windows[p][2])}
    assert set(zip(o2.tolist(), p2.tolist())) == exp2
    cand = pm.brute_force(PATS, {}, texts[:-1])
    assert und2 == sum(1 for o, p in cand if o >= base and p in windows and windows[p][2])


def test_model_planes_and_runs(lib):
    model = pm.PositionModel([b"ab", b"b", b"ab"], {0: (1, 1, False), 2: (0, 0, True)})
    # HEAD input: runs of equal offsets; record 0 of the second run is dropped, record 1 kept
    cells, offs = [0, 1, 0, 1, 2, 7, -1], [1, 1, 2, 2, 2, 2, 2]
    p, o, und = model.filter(cells, offs, pm.HEAD, True, starts=[0], text_end=10, open_end=None)
    assert (p.tolist(), o.tolist(), und) == ([1, 0, 1], [1, 2, 2], 1)
    p, o, und = model.filter(cells, offs, pm.HEAD, False, starts=[0], text_end=10, open_end=None)
    assert (p.tolist(), o.tolist(), und) == ([1, 0], [1, 2], 0)   # the undecided entry lies behind a kept one
    p, o, und = model.filter(cells, offs, pm.HEAD, True, starts=[0, 3], text_end=10, open_end=None)
    assert (p.tolist(), o.tolist(), und) == ([1, 0, 1], [1, 2, 2], 0)   # Tend = 3: 3 - 1 = 2, not in [0, 0]
    p, o, und = model.filter(cells, offs, pm.HEAD, True, starts=[0, 11], text_end=10, open_end=10)
    assert und == 0 and p.tolist() == [1, 0, 1]
    pl = pm.planes([5, 6, 7], [1, 2, 3], 4, -7, 9)
    assert pl[0].tolist() == [3, 5, 6, 9] and pl[1].tolist() == [3, 1, 2, 9]
