"""ASCII case-insensitive automata on the host (acm_automaton_set_nocase), no GPU needed.

The spec: a nocase automaton of patterns P scans text T exactly as the automaton of fold(P) scans
fold(T), fold = toupper in the C locale (bytes >= 0x80 untouched).  The reference side of every
check is the existing oracle built from the folded patterns.
"""
import ctypes as C

import numpy as np
import pytest

import fixtures
import orc
from gpu_pattern_matching_amd import AcmError, Automaton

SETS = ["tests", "sentiment", "clamav2000"]

FOLD = np.arange(256, dtype=np.uint8)
FOLD[ord("a"):ord("z") + 1] -= 0x20


def fold(b):
    if isinstance(b, np.ndarray):
        return FOLD[b]
    return bytes(FOLD[np.frombuffer(b, dtype=np.uint8)]) if b else b""


def scramble(text, seed):
    """text with the case of its ASCII letters flipped at random"""
    t = np.array(text, dtype=np.uint8, copy=True)
    letter = ((t | 0x20) >= ord("a")) & ((t | 0x20) <= ord("z"))
    flip = np.random.default_rng(seed).random(t.size) < 0.5
    t[letter & flip] ^= 0x20
    return t


def nocase_product(name):
    path, hx, max_len = fixtures.set_source(name)
    a = Automaton(nocase=True)
    a.load_file(path, hx, max_len)
    return a.compile()


def folded_oracle(name):
    o = orc.Oracle()
    for p, iid in fixtures.oracle_for(name).patterns():
        o.add(fold(p), iid)
    return o.compile()


def serial_walk(table, text, s=0):
    """The reference's serial kernel over an exported table: (positions, patterns, final state)."""
    pos, pat = [], []
    for x, c in enumerate(text.tolist()):
        v = int(table[s, 0, c])
        if v < 0:
            pos.append(x)
            pat.append(int(table[s, 1, c]))
            v = -v
        s = v
    return np.array(pos, dtype=np.uint32), np.array(pat, dtype=np.int32), s


def test_fold_is_c_locale_toupper():
    assert fold(bytes(range(256))) == bytes(range(0x61)) + bytes(range(0x41, 0x5B)) + bytes(range(0x7B, 256))


@pytest.mark.parametrize("name", SETS)
def test_same_automaton_as_folded_patterns(lib, name):
    a = nocase_product(name)
    o = folded_oracle(name)
    assert a.nocase
    assert a.num_patterns == o.num_patterns
    assert a.num_states == o.num_states
    assert a.max_pattern_len == o.max_pattern_len
    t, ot = a.reference_table(), o.table()
    upper = np.r_[0:0x61, 0x7B:256]
    assert np.array_equal(t[:, :, upper], ot[:, :, upper])
    for s in range(0, a.num_states, max(1, a.num_states // 500)):
        assert a.state_output(s) == o.head_index(s)
        assert a.state_matches(s) == o.match_list(s)[:len(a.state_matches(s))]


@pytest.mark.parametrize("name", SETS)
def test_lowercase_columns_repeat_uppercase(lib, name):
    t = nocase_product(name).reference_table()
    for c in range(ord("a"), ord("z") + 1):
        assert np.array_equal(t[:, :, c], t[:, :, c - 0x20]), chr(c)


@pytest.mark.parametrize("name", SETS)
def test_serial_walk_of_exported_table(lib, name):
    a = nocase_product(name)
    o = folded_oracle(name)
    pats = fixtures.patterns_of(name)
    rng = np.random.default_rng(7)
    # planted patterns in random bytes, then every letter's case flipped at random
    parts = []
    for i in rng.integers(0, len(pats), 300):
        parts.append(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))
        parts.append(np.frombuffer(pats[i], dtype=np.uint8))
    text = scramble(np.concatenate(parts), 11)
    got = serial_walk(a.reference_table(), text)
    exp = o.scan(fold(text))
    assert got[0].size > 0
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[2] == exp[2]


@pytest.mark.parametrize("name", SETS)
def test_pattern_returns_original_bytes(lib, name):
    a = nocase_product(name)
    o = fixtures.oracle_for(name)
    assert any(fold(p) != p for p, _ in o.patterns()) or name == "clamav2000"
    for i in range(0, a.num_patterns, max(1, a.num_patterns // 300)):
        b, iid, _ = a.pattern(i)
        assert (b, iid) == o.pattern(i)


def test_pattern_keeps_case_and_high_bytes(lib):
    a = Automaton(nocase=True)
    pats = [b"Virus", b"vIRUS", b"\xe9t\xc9", b"a-Z[`{@"]
    for i, p in enumerate(pats):
        a.add(p, i)
    a.compile()
    assert [a.pattern(i)[0] for i in range(len(pats))] == pats
    # two patterns that fold to the same bytes behave as two identical patterns
    o = orc.Oracle()
    for i, p in enumerate(pats):
        o.add(fold(p), i)
    o.compile()
    text = np.frombuffer(b"xxVIRUSvirusViRuS\xe9T\xc9\xe9t\xc9\xc9t\xe9A-z[`{@a-z{`{@", dtype=np.uint8)
    got = serial_walk(a.reference_table(), text)
    exp = o.scan(fold(text))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[2] == exp[2]
    # '[' and '{', '@' and '`' are not letters; \xc9 and \xe9 are not folded into each other
    assert got[0].tolist() == [6, 11, 16, 19, 22, 32]


@pytest.mark.parametrize("name", ["tests", "sentiment"])
def test_byte_class_map_folds(lib, name):
    a = nocase_product(name)
    n, m = a.byte_classes()
    assert n < 256
    for c in range(ord("a"), ord("z") + 1):
        assert m[c] == m[c - 0x20]
    for c in list(range(0x61)) + list(range(0x7B, 256)):
        # every other byte keeps its own class (or the class of unused bytes)
        assert m[c] == 0 or sum(1 for d in range(256) if m[d] == m[c]) == (2 if 0x41 <= c <= 0x5A else 1)
    # the classes are those of the folded set
    o = Automaton()
    for p, iid in fixtures.oracle_for(name).patterns():
        o.add(fold(p), iid)
    o.compile()
    n2, m2 = o.byte_classes()
    assert n == n2
    upper = np.r_[0:0x61, 0x7B:256]
    assert np.array_equal(m[upper], m2[upper])


def test_compact_selftest_sentiment(lib):
    a = nocase_product("sentiment")
    st = (C.c_uint32 * 9)()
    assert lib.acm_compact_selftest(a.h, 0, st) == 1


def test_set_after_compile_fails(lib):
    a = Automaton()
    a.add(b"abc", 0)
    a.set_nocase(True)
    a.set_nocase(False)
    assert not a.nocase
    a.set_nocase(True)
    a.compile()
    with pytest.raises(AcmError) as e:
        a.set_nocase(False)
    assert e.value.code == -1 and "compiled" in str(e.value)
    assert a.nocase
    assert lib.acm_automaton_set_nocase(None, 1) == -1
    assert lib.acm_automaton_nocase(None) == 0


@pytest.mark.parametrize("name", ["tests", "sentiment", "clamav2000"])
def test_flag_off_is_unchanged(lib, golden, name):
    path, hx, max_len = fixtures.set_source(name)
    a = Automaton(nocase=False)
    a.load_file(path, hx, max_len)
    a.compile()
    assert not a.nocase
    g = golden["sets"][name]
    t = a.reference_table()
    assert np.array_equal(t, fixtures.oracle_for(name).table())
    if "table_digest" in g:
        assert "%016x" % orc.table_digest(t) == g["table_digest"]
