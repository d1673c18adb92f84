"""The regime generators of variants.py keep their promises (no GPU needed): shortest and longest
pattern, byte-class count, state count, LDS qualification (acm_compact_selftest: 1 with exact tables,
or 0), and the texts they make.  test_gpu_variants.py picks its kernels through these properties; a
regime that drifts would quietly move a row to another instantiation."""
import ctypes as C

import numpy as np
import pytest

import variants
from gpu_pattern_matching_amd import _lib

SHORTEST = {3, 4, 5, 6, 8, 9, 10, 12, 13, 16}
CLASSES = {2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129}


def longest_bucket(n):
    return "<=16" if n <= 16 else "17-64" if n <= 64 else "65-96" if n <= 96 else "97-192" if n <= 192 \
        else "193-256" if n <= 256 else ">256"


@pytest.mark.parametrize("name", sorted(variants.REGIMES))
def test_regime_promises(lib, name):
    spec = variants.REGIMES[name]
    vs = variants.regime(name)
    assert vs.shortest == spec["shortest"] and vs.longest == spec["longest"]
    assert all(spec["shortest"] <= len(p) <= spec["longest"] for p in vs.patterns)
    a, o = vs.compiled()
    assert a.nocase == vs.nocase
    ncls, cmap = a.byte_classes()
    assert ncls == vs.classes
    if "classes" in spec:   # exactly classes - 1 bytes used; 129 and more: the identity table
        assert ncls == (spec["classes"] if spec["classes"] <= 128 else 256)
        assert variants.log_stride(spec["classes"]) == (8 if ncls == 256 else max(1, int(np.ceil(np.log2(ncls)))))
    if spec.get("alphabet") == "binary":
        used = set(b"".join(vs.patterns))
        assert 0x00 in used and 0xFF in used and ncls == 256
    if vs.nocase:   # a lowercase letter shares its uppercase letter's class
        assert all(cmap[c] == cmap[c - 0x20] for c in range(ord("a"), ord("z") + 1))
        assert any(c in b"".join(vs.patterns) for c in b"abcdefghijklmnopqrstuvwxyz")
    lo, hi = vs.states
    assert lo <= a.num_states <= hi
    assert a.num_states == o.num_states
    st = (C.c_uint32 * 9)()
    rc = lib.acm_compact_selftest(a.h, 0, st)
    assert rc in (0, 1), _lib.load().acm_last_error()
    assert (rc == 1 and vs.longest <= 33) == vs.lds, (rc, vs.longest)
    assert vs.stride == {3: 1, 4: 2, 5: 2}.get(vs.shortest, 4 if vs.shortest < 10 else 8)
    a.close()
    o.close()


def test_regimes_cover_the_dispatch():
    """every sieve (W, D, LG), every longest-pattern bucket, every class count step, LDS-resident and not,
    non-final states below and above hot_max, each alphabet -- nocase included"""
    sets = {k: variants.regime(k) for k in variants.REGIMES}
    assert SHORTEST <= {v.shortest for v in sets.values()}
    sieve = {(v.stride, min(v.shortest, 10), v.key_len, v.nocase) for v in sets.values()}
    for w, lg in ((1, 3), (2, 3), (4, 3), (4, 6), (8, 3), (8, 6)):
        for nc in (False, True):
            assert any(s[0] == w and s[2] == lg and s[3] == nc for s in sieve), (w, lg, nc)
    assert {"<=16", "17-64", "65-96", "97-192", ">256"} <= {longest_bucket(v.longest) for v in sets.values()}
    assert CLASSES <= {variants.REGIMES[k].get("classes") for k in sets}
    assert {True, False} == {v.lds for v in sets.values()}
    assert any(variants.REGIMES[k].get("big") for k in sets)
    assert {True, False} == {v.nocase for v in sets.values()}


@pytest.mark.parametrize("name", ["s3_binary_l192", "c128", "c129", "big_c17", "c17", "lds16_letters"])
def test_non_final_states_against_hot_max(lib, name):
    """hot_max = the chain walk's LDS rows for the set's log_stride: some sets fit, some do not"""
    vs = variants.regime(name)
    a, _ = vs.compiled()
    nonfinal = sum(1 for r in range(a.num_states) if not a.state_matches(r))
    above = nonfinal > variants.hot_max(vs.classes)
    assert above == (name in ("s3_binary_l192", "c128", "c129", "big_c17")), (nonfinal, variants.hot_max(vs.classes))


@pytest.mark.parametrize("name", ["s3_letters", "s5_binary", "s9_mixed", "l300_c5"])
def test_texts(lib, name):
    vs = variants.regime(name)
    _, o = vs.compiled()
    n = 1 << 16
    rnd = variants.text(vs, n, 1, "random")
    assert rnd.size == n
    allowed = set(vs.alphabet.tolist()) | ({vs.outside} if vs.outside is not None else set())
    if vs.nocase:
        allowed |= {c ^ 0x20 for c in allowed if 0x41 <= (c & 0xDF) <= 0x5A}
    assert set(np.unique(rnd).tolist()) <= allowed
    if vs.outside is not None:
        assert vs.outside in rnd
    pl = variants.text(vs, n, 2, "planted")
    pos, pat, _ = o.scan(vs.text_of(pl))
    assert pos.size >= n // 96 // 2 and int(pos[-1]) == n - 1   # a match ends with the text
    at_border = [int(p) for p, q in zip(pos, pat) if any(
        (int(p) // b) != ((int(p) - len(vs.patterns[q - 1]) + 1) // b) for b in (64, 4096))]
    assert len(at_border) >= 8
    runs = vs.text_of(variants.text(vs, n, 3, "runs"))     # (folded: a nocase run is in mixed case)
    assert np.max(np.diff(np.flatnonzero(np.diff(runs.astype(np.int16)) != 0))) >= 64
    dense = variants.text(vs, n, 4, "dense")
    d = o.scan(vs.text_of(dense))[0]
    assert d.size > n // (4 * vs.longest)
    if vs.nocase:
        lower = (pl >= ord("a")) & (pl <= ord("z"))
        upper = (pl >= ord("A")) & (pl <= ord("Z"))
        assert lower.any() and upper.any()
