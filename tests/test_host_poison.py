"""The poisoned tails of test_gpu_poison.py can fail a scan that reads past n (no GPU needed).

For every regime of variants.py and the fixture sets, at every cut the GPU test scans a row's text at,
the oracle over t[:n] and over t[:n + k] (the view's next k bytes) must differ -- in a record or in the
final state -- for the "complete" tail with some k <= 16 and for the "continue" tail (the text that
really follows) with some k inside the poisoned 4 KiB.  A kernel that went on past n would then give
an answer other than the oracle's; if no tail could change the answer, a passing GPU row would prove
nothing."""
import numpy as np
import pytest

import fixtures
import orc
import poison
import variants
import word_model as wm
from test_gpu_variants import ROWS

FIXTURE_SETS = ("clamav2000", "sentiment", "tests")
FIXTURE_N = 64 * 1024 + 11


def row_cases(name):
    """(n_row, S, text kind) of every GPU row on this regime; a SMALL row with no chain bytes where none"""
    out = sorted({(r.n, r.S, r.kind) for r in ROWS if r.regime == name})
    return out or [(poison.SMALL, 0, "planted")]


def differs(o, text_of, h, n, init, longest, ks=range(1, 17)):
    """some k in ks: the oracle over h[:n + k] differs from the oracle over h[:n] (the last `longest`
    bytes and more before n decide both, so a window of the text stands in for the whole)"""
    lo = max(0, n - 2 * longest - 64)
    s = init if lo == 0 else 0
    base = o.scan(text_of(h[lo:n]), s)
    for k in ks:
        ext = o.scan(text_of(h[lo:n + k]), s)
        if ext[0].size != base[0].size or ext[2] != base[2]:
            return k
    return None


def check_cuts(o, text_of, pats, fold, t, cut_list, inits, longest, seed):
    for n, s in zip(cut_list, inits):
        for kind in ("complete", "continue"):
            lo = max(0, n - 2 * longest - 64)
            h = np.concatenate([t[lo:n], poison.tail_bytes(kind, t, n, poison.PAST_PAD, pats, fold, seed + n)])
            ks = range(1, 17) if kind == "complete" else list(range(1, 17)) + [1 << e for e in range(5, 13)]
            k = differs(o, text_of, h, n - lo, s if lo == 0 else 0, longest, ks)
            assert k is not None, "cut %d, %s tail: no k in %s changes the oracle's answer" % (n, kind, ks)


@pytest.mark.parametrize("name", sorted(variants.REGIMES))
def test_regime_tails_change_the_answer(name):
    vs = variants.regime(name)
    o = poison.oracle_of(vs)
    fold = variants.fold if vs.nocase else None
    seed = poison.row_seed(name)
    for n_row, S, kind in row_cases(name):
        if n_row > poison.SMALL:   # only the bytes around the one cut matter: a window of the row's text
            t, cut = poison.row_text(vs, n_row, seed, kind)
            cut_list = [cut]
        else:
            t, cut = poison.row_text(vs, n_row, seed, kind)
            cut_list = poison.cuts(n_row, S, cut)
        inits = poison.init_states(seed, len(cut_list), o.num_states)
        check_cuts(o, vs.text_of, vs.patterns, fold, t, cut_list, inits, vs.longest, seed)
    o.close()


@pytest.mark.parametrize("nocase", [False, True], ids=["case", "nocase"])
@pytest.mark.parametrize("name", FIXTURE_SETS)
def test_fixture_tails_change_the_answer(name, nocase):
    o = fixtures.oracle_for(name)
    pats = fixtures.patterns_of(name)
    if nocase:
        f = orc.Oracle()
        for p, iid in o.patterns():
            f.add(wm.fold(p), iid)
        o = f.compile()
    fold = wm.fold if nocase else None
    text_of = (lambda b: wm.FOLD[np.asarray(b, dtype=np.uint8)]) if nocase else (lambda b: b)
    t = wm.planted_text(pats, FIXTURE_N + 8192, 17)
    longest = max(len(p) for p in pats)
    plant_at = FIXTURE_N - 64 - len(max(pats, key=len)) // 2
    poison.plant(t, max(pats, key=len), plant_at)
    cut_list = poison.cuts(FIXTURE_N, 0, FIXTURE_N - 64)
    inits = poison.init_states(17, len(cut_list), o.num_states)
    check_cuts(o, text_of, pats, fold, t, cut_list, inits, longest, 17)


def test_completion():
    pats = [b"abcdef", b"xyz", b"cdq"]
    assert poison.completion(pats, b"...abc") == b"def"
    assert poison.completion(pats, b"...abcd") == b"ef"
    assert poison.completion(pats, b"...xy") == b"z"
    assert poison.completion(pats, b"...q") == b"xyz"
    assert poison.completion([b"ABCD"], b"..ab", variants.fold) == b"CD"
    h = poison.view_host(np.frombuffer(b"0123456789abcdefxy" * 4, dtype=np.uint8), 33, "complete", pats)
    assert h.size == 48 + poison.PAST_PAD and bytes(h[:33]) == (b"0123456789abcdefxy" * 2)[:33]
    assert bytes(h[33:34]) == b"f" and bytes(h[34:37]) in (b"abc", b"xyz", b"cdq")   # then whole patterns
