"""Matcher.scan_normalized through every branch it has: the sparse and the chain pipeline over a normalised text, a
nocase automaton, a mixed automaton (the case pass reads the normalised bytes), with and without all_patterns, one text
and many.  The expectation is the model's normalisation of every text (tests/normalize_model.py), bytes.find of every
pattern on its output (upper-cased on both sides for a folding pattern) and the model's first[] / last[] to map back.

The normalised text is given exactly m bytes (out_capacity = m) and m % 16 is 1 or 15: the scan reads the 16-byte rounded
tail behind m.  Every buffer the pipeline allocates, d_out among them, is filled with 'f' before it is used (the
pipeline's alloc is wrapped), and the input ends in "a hre": a scan that took the byte behind m for text would report
"a href" there."""
import functools

import numpy as np
import pytest

import normalize_model as nm
from gpu_pattern_matching_amd import Automaton, Matcher, api
from normalize_model import PERCENT, SQUEEZE, STRIP

pytestmark = pytest.mark.gpu

SIZE = 200 * 1024
TOKENS = [b"a", b"b", b"x", b" ", b"  ", b"\t", b"%20", b"%09", b"%4", b"%", b"0A", b"href", b"HREF", b"Href", b"%48ref", b"a href",
          b"a%20href", b"A HREF", b"%41", b"=q", b"a b", b" b "]
TAIL = b"a hre"
POISON = 0x66                      # 'f'

# (pattern, it ignores case).  In the sets that are scanned without all_patterns no pattern is a suffix of another (after
# folding, where any folds): a record then has one pattern, whatever the scan reports for a state with several
PLAIN = [(p, False) for p in (b"a href", b"Href", b"a b", b"0A ", b"HREF", b" b ", b"x A", b"ref=q", b"0AA")]         # all >= 3 bytes: sparse
NOCASE = [(p, True) for p in (b"a href", b"a b", b"0A ", b" b ", b"x A", b"ref=q", b"b%4", b"0AA")]
MIXED = [(b"a href", False), (b"ref=q", True), (b"0Ah", False), (b"b hre", True), (b"x A", False), (b"a b", True), (b" 0A", False), (b"0AA", False)]
MIXED_ALL = MIXED + [(b"href", True), (b"HREF", False), (b"ref", False), (b"A", False), (b"f", True)]

# name: (patterns, set_nocase, scan mode, all_patterns)
CASES = {"sparse": (PLAIN, False, "sparse", False), "chain": (PLAIN, False, "chain", False), "nocase": (NOCASE, True, None, False),
         "mixed": (MIXED, False, None, False), "mixed-all": (MIXED_ALL, False, None, True), "chain-all": (PLAIN + [(b"f", False), (b"ref", False)], False, "chain", True)}
# (one text or many, m % 16, flags)
SHAPES = [("one", 1, PERCENT | SQUEEZE), ("one", 15, PERCENT | SQUEEZE), ("texts", 15, PERCENT | SQUEEZE), ("texts", 1, PERCENT | STRIP)]


def no_suffixes(pats):
    folded = [p.upper() if any(f for _, f in pats) else p for p, _ in pats]
    return not any(i != j and a.endswith(b) for i, a in enumerate(folded) for j, b in enumerate(folded))


PLANTED = ((SIZE // 3, b"x%20href"), (SIZE // 2, b"x  \t  a href"))   # where cut() cuts a triple and a run


def body(seed):
    rng = np.random.default_rng(seed)
    t = bytearray(b"".join(TOKENS[i] for i in rng.integers(0, len(TOKENS), SIZE // 2))[:SIZE - len(TAIL)] + TAIL)
    for at, what in PLANTED:
        t[at:at + len(what)] = what
    return bytes(t)


def cut(text, seed):
    """about 40 parts: cut at random places, inside a triple, at both ends of and inside a blank run (a part of blanks
    only), and twice at one place (an empty part)"""
    rng = np.random.default_rng(seed)
    cuts = set(rng.integers(1, len(text) - 1, 34).tolist())
    (t, _), (r, _) = PLANTED
    cuts |= {t + 2, t + 3, r + 1, r + 3, r + 6}                      # x% | 2 | 0 ...; x |   | \t  | a
    cuts = sorted(cuts)
    cuts.insert(5, cuts[5])
    cuts.insert(20, cuts[20])
    return [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]


@functools.lru_cache(maxsize=None)
def inputs(shape, phase, flags):
    """(the texts, the model's result per text): padded in front with letters until the normalised length is `phase`
    modulo 16"""
    text = body(7 + phase)
    parts = cut(text, phase) if shape == "texts" else [text]
    m = sum(nm.normalize(p, flags).m for p in parts)
    parts[0] = b"z" * ((phase - m) % 16) + parts[0]
    return parts, [nm.normalize(p, flags) for p in parts]


def expected(pats, parts, norms):
    """{(pattern, first byte, last byte)} in the coordinates of the concatenation, and counts from the model: matches that
    end on a triple, matches that start on the one blank of a squeezed run, candidates of exact patterns that are no
    matches, matches of folding patterns in another case than the pattern's"""
    found, base = set(), 0
    seen = dict(triple=0, run=0, dropped=0, folded=0)
    for t, x in zip(parts, norms):
        up = x.out.upper()
        for i, (p, fold) in enumerate(pats):
            hay, needle = (up, p.upper()) if fold else (x.out, p)
            k = hay.find(needle)
            while k >= 0:
                e = k + len(p) - 1
                found.add((i, base + int(x.first[k]), base + int(x.last[e])))
                seen["triple"] += int(x.last[e] - x.first[e] == 2)
                seen["run"] += int(x.out[k] == 0x20 and k + 1 < x.m and x.first[k + 1] > x.last[k] + 1 and t[x.last[k] + 1] in nm.DEFAULT_BLANKS)
                seen["folded"] += int(fold and x.out[k:e + 1] != p)
                k = hay.find(needle, k + 1)
            if not fold:
                seen["dropped"] += up.count(p.upper()) - x.out.count(p)
        base += len(t)
    return found, seen


def check_inputs(shape, phase, flags):
    """what the inputs are meant to be, from the model alone"""
    parts, norms = inputs(shape, phase, flags)
    m = sum(x.m for x in norms)
    assert m % 16 == phase and sum(len(p) for p in parts) >= SIZE and parts[-1].endswith(TAIL)
    assert norms[-1].out.endswith(TAIL.replace(b" ", b"") if flags & STRIP else TAIL)
    if shape == "texts":
        assert 38 <= len(parts) <= 45 and sum(1 for p in parts if not p) >= 2
        assert any(p.endswith(b"%") for p in parts) and any(p == b"2" for p in parts)      # cut inside a triple
        blank = [k for k, p in enumerate(parts) if p and not p.strip(b" \t")]
        assert blank and all(norms[k].m == (0 if flags & STRIP else 1) for k in blank)        # parts of a run: nothing under strip
    return parts, norms, m


def check_expected(name, shape, phase, flags):
    pats, set_nocase, mode, all_patterns = CASES[name]
    parts, norms, m = check_inputs(shape, phase, flags)
    exp, seen = expected(pats, parts, norms)
    assert len(exp) > 1000 and seen["triple"] >= 1 and (seen["run"] >= 1 or not flags & SQUEEZE), (len(exp), seen)
    assert all_patterns or (no_suffixes(pats) and len({e for _, _, e in exp}) == len(exp))
    if name.startswith("mixed"):
        assert seen["dropped"] > 100 and seen["folded"] > 100, seen          # HREF, Href, %48ref: exact dropped, folding kept
    return parts, exp, m


@pytest.fixture(scope="module")
def matchers(gpu):
    made = {}

    def get(name):
        if name not in made:
            pats, set_nocase, mode, _ = CASES[name]
            a = Automaton()
            if set_nocase:
                a.set_nocase()
            for i, (p, fold) in enumerate(pats):
                a.add(p, i, nocase=fold and not set_nocase)
            a.compile()
            assert a.mixed_case == name.startswith("mixed") and a.nocase == set_nocase
            m = Matcher(a, 0, max_text=1 << 18)
            a.close()
            if mode:
                assert (m.sparse_eligible() or mode != "sparse") and m.set_mode(mode) == mode
            made[name] = m
        return made[name]
    yield get
    for m in made.values():
        m.close()


@pytest.fixture
def poisoned(monkeypatch):
    """every buffer a pipeline allocates holds 'f' bytes: the normalised text's room behind m among them"""
    real, filled = api._Pipeline.alloc, []

    def alloc(self, nbytes):
        b = real(self, nbytes)
        b.fill(POISON, self.stream)
        filled.append(nbytes)
        return b
    monkeypatch.setattr(api._Pipeline, "alloc", alloc)
    return filled


@pytest.mark.parametrize("shape,phase,flags", SHAPES, ids=["one-1", "one-15", "texts-15", "texts-1-strip"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_scan_normalized_branches(matchers, poisoned, name, shape, phase, flags):
    pats, _, mode, all_patterns = CASES[name]
    parts, exp, m = check_expected(name, shape, phase, flags)
    mt = matchers(name)
    assert mt.mixed == name.startswith("mixed")
    kw = dict(percent=True, squeeze=bool(flags & SQUEEZE), strip=bool(flags & STRIP), all_patterns=all_patterns, out_capacity=m)
    res = mt.scan_normalized(parts[0], **kw) if shape == "one" else mt.scan_normalized(texts=parts, **kw)
    assert (m + 15) // 16 * 16 + 16 in poisoned                       # the normalised text's buffer was one of them
    if mode:
        assert mt.path_taken(m) == mode
    got = set(zip(res[0].tolist(), res[1].tolist(), res[2].tolist()))
    assert res[3] == m and res[0].size == len(got)
    assert got == exp, "missing %s, not expected %s (the first five)" % (sorted(exp - got)[:5], sorted(got - exp)[:5])
