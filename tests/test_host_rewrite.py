"""Match rewriting without a device: the model of tests/rewrite_model.py against re.sub, the replacement setters and
getters, the replacement file, that compile does not see replacements, and what acm_grep says about -r and -O before
it touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rewrite_model as rw
from gpu_pattern_matching_amd import AcmError, Automaton, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gpu_pattern_matching_amd", "acm_grep")

PATS = [b"abc", b"ab", b"b", b"cab", b"a", b"aa", b"aaa", b"", b"bca", b"dddd"]


def build(pats=PATS):
    a = Automaton()
    for i, p in enumerate(pats):
        a.add(p, i)
    return a


def random_repl(rng, k):
    """a replacement per pattern: none, bytes of 0 to 6 bytes (upper case: never a pattern), or a fill"""
    out = []
    for _ in range(k):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            out.append(None)
        elif kind == 1:
            out.append((bytes([int(rng.integers(0x2A, 0x30))]), True))
        else:
            out.append((bytes(rng.integers(0x41, 0x5B, int(rng.integers(0, 7))).astype(np.uint8)), False))
    return out


def test_model_against_re_sub():
    rng = np.random.default_rng(3)
    words = [b"a", b"ab", b"abc", b"b", b"bc", b"bcd", b"cd", b"dddd", b"ca", b"dab", b"abcdabcd"]
    for case in range(300):
        pats = [words[i] for i in rng.permutation(len(words))[:int(rng.integers(1, len(words) + 1))]]
        nocase = case % 3 == 2
        alphabet = b"abcdABCD" if nocase else b"abcde"
        text = bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), int(rng.integers(0, 60)))])
        repl = random_repl(rng, len(pats))
        cells, offs = rw.selected(pats, [text], nocase)
        out, info, at, _ = rw.RewriteModel([len(p) for p in pats], repl).run(text, cells, offs)
        assert out == rw.re_sub(pats, repl, text, nocase), (case, pats, text)
        assert info[0] == cells.size and info[1] == 0 and info[2] == len(out) and info[6:] == [0, 0]
        for k, a in enumerate(at):                           # every replacement stands where at says
            r = repl[int(cells[k])]
            if r is not None and not r[1]:
                assert out[a:a + len(r[0])] == r[0], case


def test_model_hand_cases():
    m = rw.RewriteModel([3, 1, 2], [(b"XY", False), (b"*", True), None])
    #       0123456789
    text = b"abc.x.de.x"
    cells, offs = [0, 1, 2, 1], [2, 4, 7, 9]
    out, info, at, seg = m.run(text, cells, offs, seg_start=[-5, 0, 1, 3, 4, 5, 9, 10, 99])
    assert out == b"XY.*.de.*" and info == [4, 0, 9, 0, 7, 0, 0, 0] and at == [0, 3, 5, 8]
    assert seg == [0, 0, 0, 2, 3, 4, 8, 9, 9]                # a start inside a span: every used record with s < x counts
    # records that are no pattern, of length 0, or outside the text are skipped; origin shifts the offsets
    m = rw.RewriteModel([3, 0, 1], [(b"", False), (b"Q", False), (b"1234", False)])
    out, info, at, _ = m.run(b"abcabc", [0, 1, -1, 7, 2, 2, 0, 2], [102, 102, 103, 103, 103, 99, 106, 105], origin=100, cap=3)
    #   0 @102: [100, 102] deleted; 1: length 0; -1, 7: no pattern; 2 @103 used; 2 @99: in front of the text; 0 @106: ends
    #   behind it; 2 @105 used
    assert out == b"1234b1234" and info == [3, 5, 9, 0, 5, 0, 1, 0] and at == [0, 0, 5]
    assert m.run(b"abcabc", [0], [102], origin=100, cap=3)[1] == [1, 0, 3, 0, 3, 0, 0, 0]
    assert m.run(b"abcabc", [2], [105], origin=100, cap=3, have_out=False)[1][6] == 0


def test_setters_and_getters(lib):
    a = build()
    assert not a.has_replacements and all(a.replacement(i) is None for i in range(len(PATS)))
    a.set_replacement(0, b"hello")
    a.set_replacement(1, fill=0x2A)
    a.set_replacement(2, fill=b"#")
    a.set_replacement(3, b"")
    assert a.has_replacements
    assert [a.replacement(i) for i in range(5)] == [(b"hello", False), (b"*", True), (b"#", True), (b"", False), None]
    a.compile()                                              # after compile as well
    a.set_replacement(4, bytes(range(256)))
    assert a.replacement(4) == (bytes(range(256)), False)
    big = bytes(np.arange(_lib.REPLACEMENT_MAX_LEN, dtype=np.uint32).astype(np.uint8))
    a.set_replacement(5, big)
    assert a.replacement(5) == (big, False)
    with pytest.raises(AcmError) as e:
        a.set_replacement(6, big + b"x")                     # 65536 bytes
    assert e.value.code == -5 and a.replacement(6) is None
    # "delete" through the raw call: NULL, 0, 0
    assert lib.acm_automaton_set_replacement(a.h, 6, None, 0, 0) == 0
    assert a.replacement(6) == (b"", False)
    for i in range(7):
        a.clear_replacement(i)
    assert not a.has_replacements and a.replacement(0) is None
    n, fl = C.c_int(7), C.c_uint(7)
    assert lib.acm_automaton_pattern_replacement(a.h, 0, None, n, fl) == 0 and (n.value, fl.value) == (0, 0)
    assert lib.acm_automaton_pattern_replacement(a.h, 0, None, None, None) == 0
    assert lib.acm_automaton_has_replacements(None) == 0


def test_argument_errors(lib):
    a = build([b"abc", b"de"])
    bad = [(-1, b"x", 1, 0), (2, b"x", 1, 0), (0, b"x", 1, 2), (0, b"x", 1, 0x80000000), (0, b"xy", 2, 1), (0, b"", 0, 1),
           (0, None, 0, 1), (0, b"x", -1, 0), (0, None, 1, 0), (0, None, -1, 0)]
    for args in bad:
        assert lib.acm_automaton_set_replacement(a.h, *args) == -1, args
        assert lib.acm_last_error()
    assert lib.acm_automaton_set_replacement(None, 0, b"x", 1, 0) == -1
    assert lib.acm_automaton_set_replacement(a.h, 0, b"x" * 65536, 65536, 0) == -5
    assert not a.has_replacements
    for bad_index in (-1, 2):
        assert lib.acm_automaton_pattern_replacement(a.h, bad_index, None, None, None) == -1
        assert lib.acm_automaton_clear_replacement(a.h, bad_index) == -1
        with pytest.raises(AcmError):
            a.replacement(bad_index)
    assert lib.acm_automaton_pattern_replacement(None, 0, None, None, None) == -1
    assert lib.acm_automaton_clear_replacement(None, 0) == -1
    with pytest.raises(ValueError):
        a.set_replacement(0)
    with pytest.raises(ValueError):
        a.set_replacement(0, b"x", fill=1)
    assert lib.acm_automaton_load_replacement_file(None, b"x") == -1
    assert lib.acm_automaton_load_replacement_file(a.h, None) == -1


def test_replacement_file(lib, tmp_path):
    a = build(PATS[:6])
    good = tmp_path / "good.repl"
    good.write_bytes(b"# replacements\n\n0 58595a\n  1 fill 2a  \n2\n\t3\tfill\t00\r\n   # indented comment\n4 4A4b\n0 51\n5 \n")
    assert a.load_replacement_file(good) == 7
    assert a.replacement(0) == (b"Q", False)                 # the later line wins
    assert a.replacement(1) == (b"*", True) and a.replacement(2) == (b"", False)
    assert a.replacement(3) == (b"\x00", True) and a.replacement(4) == (b"JK", False) and a.replacement(5) == (b"", False)
    long_line = tmp_path / "long.repl"
    long_line.write_bytes(b"1 " + b"ab" * 65535 + b"\n")
    assert a.load_replacement_file(long_line) == 1 and a.replacement(1) == (b"\xab" * 65535, False)
    empty = tmp_path / "empty.repl"
    empty.write_bytes(b"# nothing\n\n")
    assert a.load_replacement_file(empty) == 0
    bad_lines = [b"6 41", b"-1 41", b"x 41", b"0 4", b"0 414", b"0 4g", b"0 41 42", b"0 fill", b"0 fill 4", b"0 fill 414",
                 b"0 fill 41 42", b"0 fill zz", b"0 filler", b"0 FILL 41", b"0x1 41", b"99999999999 41", b"0 0x41",
                 b"0 " + b"ab" * 65536]
    for k, line in enumerate(bad_lines):
        b = build(PATS[:6])
        f = tmp_path / ("bad%d.repl" % k)
        f.write_bytes(b"# c\n1 41\n" + line + b"\n2 fill 2a\n")
        with pytest.raises(AcmError) as e:
            b.load_replacement_file(f)
        assert e.value.code == -7, line[:20]
        assert "%s:3:" % f in str(e.value), (line[:20], str(e.value))
        assert not b.has_replacements, line[:20]             # nothing of a bad file is applied
    with pytest.raises(AcmError) as e:
        a.load_replacement_file(tmp_path / "missing.repl")
    assert e.value.code == -6


def sieve_stats(lib, a):
    st = (C.c_uint32 * 21)()
    rc = lib.acm_sieve_selftest(a.h, st)
    return rc, list(st)


@pytest.mark.parametrize("pats", [[b"abcd", b"bcde", b"abc", b"cdefgh"], PATS], ids=["sparse", "chain"])
def test_compile_does_not_see_replacements(lib, pats):
    plain = build(pats)
    plain.compile()
    before = build(pats)
    before.set_replacement(0, b"longer than the pattern")
    before.set_replacement(1, fill=0)
    before.set_replacement(2, b"")
    before.compile()
    after = build(pats)
    after.compile()
    after.set_replacement(1, b"x")
    assert not plain.has_replacements and before.has_replacements and after.has_replacements
    for a in (before, after):
        assert np.array_equal(a.reference_table(), plain.reference_table())
        assert sieve_stats(lib, a) == sieve_stats(lib, plain)
        assert a.byte_classes()[0] == plain.byte_classes()[0]
        assert [a.state_matches(s) for s in range(a.num_states)] == [plain.state_matches(s) for s in range(plain.num_states)]
        assert [a.pattern(i) for i in range(len(pats))] == [plain.pattern(i) for i in range(len(pats))]
        st1, st2 = (C.c_uint32 * 9)(), (C.c_uint32 * 9)()
        assert lib.acm_compact_selftest(a.h, 0, st1) == lib.acm_compact_selftest(plain.h, 0, st2)
        assert list(st1) == list(st2)


@pytest.mark.parametrize("name", ["tests", "tests1", "sentiment", "clamav2000", "clamav2000_m12"])
def test_fixture_sets_are_unchanged(lib, golden, name):
    """the fixture sets with replacements set on every pattern (and, the second time, cleared again): states, longest
    pattern and table digest are the values tests/golden/golden.json pins for the set without them"""
    import fixtures
    import orc
    path, hx, max_len = fixtures.set_source(name)
    g = golden["sets"][name]
    for clear in (False, True):
        a = Automaton()
        n = a.load_file(path, hx, max_len)
        longest = 0
        for k, i in enumerate(range(0, n, max(1, n // 300))):
            if k % 3:
                a.set_replacement(i, b"replaced %d" % i)
                longest = max(longest, len(b"replaced %d" % i))
            else:
                a.set_replacement(i, fill=i % 256)
        assert a.has_replacements
        if clear:
            for i in range(n):
                a.clear_replacement(i)
            assert not a.has_replacements
        a.compile()
        assert (n, a.num_states, a.max_pattern_len) == (g["patterns"], g["states"], g["max_pattern_len"])
        if "table_digest" in g:
            assert "%016x" % orc.table_digest(a.reference_table()) == g["table_digest"]
        assert lib.acm_automaton_max_replacement_len(a.h) == (0 if clear else longest)


def test_usage_names_rewrite():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert "  -r " in r.stdout and "  -O " in r.stdout and "replacement" in r.stdout


def test_refused_combinations(tmp_path):
    """every refused combination is a usage error: its ERROR: line, the usage text and a failure, no device needed"""
    pats = tmp_path / "p.txt"
    pats.write_text("ab\nabc\n")
    repl = tmp_path / "r.txt"
    repl.write_text("0 2a\n")
    sigs = tmp_path / "s.txt"
    sigs.write_text("6162*6364\n")
    rules = tmp_path / "r.ldb"
    rules.write_text("0;6162\n")
    data = tmp_path / "d.txt"
    data.write_text("abcd\n")
    out = tmp_path / "out"
    base = [CLI, "-f", str(data), "-p", str(pats), "-B", "64", "-D", "0", "-G", "16", "-L", "64"]
    both = base + ["-r", str(repl), "-O", str(out)]
    for extra in (["-t"], ["-A"], ["-c"], ["-n"], ["-Q", str(sigs)], ["-K", str(rules), "-S"], ["-Q", str(sigs), "-E"], ["-F"]):
        r = subprocess.run(both + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, extra
        assert "ERROR: -r cannot be combined with -t, -A, -c, -n, -Q, -K, -E or -F" in r.stdout, (extra, r.stdout[:300])
        assert "Usage:" in r.stdout, extra
    for args, msg in ((base + ["-r", str(repl)], "ERROR: -r needs -O"), (base + ["-O", str(out)], "ERROR: -O needs -r")):
        r = subprocess.run(args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stdout and "Usage:" in r.stdout, (args, r.stdout[:300])
    assert not out.exists()


def test_refused_output_paths(tmp_path):
    """two inputs of one name would share an output, and an output that is an input would be cut while it is read:
    both are refused before a device is touched, and no file is written or changed"""
    pats = tmp_path / "p.txt"
    pats.write_text("ab\nabc\n")
    repl = tmp_path / "r.txt"
    repl.write_text("0 2a\n")
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
        (tmp_path / d / "same.txt").write_text("abcd %s\n" % d)
    out = tmp_path / "out"
    base = [CLI, "-p", str(pats), "-B", "64", "-D", "0", "-G", "16", "-L", "64", "-r", str(repl)]
    r = subprocess.run(base + ["-f", "%s,%s" % (tmp_path / "a" / "same.txt", tmp_path / "b" / "same.txt"), "-O", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "ERROR: -O:" in r.stderr and "would both be written" in r.stderr and not out.exists()
    for data, where in ((tmp_path / "a", tmp_path / "a"), (tmp_path / "a" / "same.txt", tmp_path / "a")):
        r = subprocess.run(base + ["-f", str(data), "-O", str(where)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "ERROR: -O:" in r.stderr and "is an input file" in r.stderr
        assert (tmp_path / "a" / "same.txt").read_text() == "abcd a\n"
