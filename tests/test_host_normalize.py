"""tests/normalize_model.py on the host: hand-written vectors, independent library restatements on random texts over an
alphabet rich in % 0-9 a-f A-F, blanks and NUL, and the locality the kernels rest on (whether byte i emits depends on
bytes i - 3 .. i + 2 and the text starts among them) restated and compared with the serial walk."""
import re
import urllib.parse

import numpy as np
import pytest

import normalize_model as nm
from normalize_model import PERCENT, SQUEEZE, STRIP

ALPHABET = b"%%%%0123456789abcdefABCDEF \t\n\v\f\r\x00gG+zZ"
BLANKS = b"\t\n\v\f\r "
MODES = [0, PERCENT, SQUEEZE, STRIP, PERCENT | SQUEEZE, PERCENT | STRIP]


def random_text(n, seed):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(ALPHABET, dtype=np.uint8)[rng.integers(0, len(ALPHABET), n)])


def squeeze(t):
    return re.sub(rb"[\t\n\v\f\r ]+", b" ", t)


def strip(t):
    return t.translate(None, BLANKS)


def test_hand_written_vectors():
    r = nm.normalize(b"a  \t b", SQUEEZE)
    assert r.out == b"a b" and r.first.tolist() == [0, 1, 5] and r.last.tolist() == [0, 1, 5] and r.info[:4] == [3, 3, 0, 1]
    r = nm.normalize(b"a%20b", PERCENT)
    assert r.out == b"a b" and r.first.tolist() == [0, 1, 4] and r.last.tolist() == [0, 3, 4] and r.info[:4] == [3, 0, 1, 0]
    assert r.keep.tolist() == [True, True, False, False, True]
    r = nm.normalize(b"a%20 %09href", PERCENT | SQUEEZE)
    assert r.out == b"a href" and r.first.tolist() == [0, 1, 8, 9, 10, 11] and r.last.tolist() == [0, 3, 8, 9, 10, 11]
    assert r.info[:4] == [6, 2, 2, 1]
    assert nm.normalize(b"%2541", PERCENT).out == b"%41"                      # decoding happens once
    for tail in (b"%", b"%4", b"%4g", b"%g4"):
        assert nm.normalize(b"x" + tail, PERCENT).out == b"x" + tail         # literal
    assert nm.normalize(b"%%41", PERCENT).out == b"%A"
    assert nm.normalize(b"%4%41", PERCENT).out == b"%4A"
    assert nm.normalize(b"A\0B\0C\0", STRIP, blanks=b"\0").out == b"ABC"
    assert nm.normalize(b" \t ", SQUEEZE).out == b" " and nm.normalize(b" \t ", STRIP).out == b""
    assert nm.normalize(b"a \nb", SQUEEZE, blank_byte=0x5F).out == b"a_b"
    assert nm.normalize(b"a b", SQUEEZE, blanks=b"a").out == b"  b"            # a custom set: the space is no blank
    assert nm.normalize(b"a \t b", 0).out == b"a \t b"
    # texts: a run never continues across a start, a triple never crosses one
    r = nm.normalize(b"a  " + b"  b", SQUEEZE, seg_start=[0, 3])
    assert r.out == b"a  b" and r.seg_out.tolist() == [0, 2] and r.first.tolist() == [0, 1, 3, 5]
    r = nm.normalize(b"x%4" + b"1y", PERCENT, seg_start=[0, 3])
    assert r.out == b"x%41y" and r.info[2] == 0
    r = nm.normalize(b"x%41y", PERCENT, seg_start=[-7, 2, 99])               # starts are clamped; byte 0 starts a text
    assert r.out == b"x%41y" and r.seg_out.tolist() == [0, 2, 5]
    r = nm.normalize(b"ab%41", PERCENT, origin=100, seg_start=[100, 102])
    assert r.out == b"abA" and r.first.tolist() == [100, 101, 102] and r.last.tolist() == [100, 101, 104]
    # the map
    r = nm.normalize(b"%41" * 700, PERCENT)
    assert r.m == 700 and r.block.tolist() == [0, 342, 683, 700] and r.keep_words.size == 33
    assert int(r.keep_words[0]) == sum(1 << i for i in range(0, 64, 3))
    assert nm.normalize(b"", SQUEEZE).block.tolist() == [0] and nm.normalize(b"x" * 1024, 0).block.tolist() == [0, 1024]
    assert nm.normalize(b"x" * 10, 0, out_capacity=9).info[4] == 1 and nm.normalize(b"x" * 10, 0, out_capacity=10).info[4] == 0


@pytest.mark.parametrize("seed", range(6))
def test_library_restatements(seed):
    for n in (0, 1, 2, 3, 7, 64, 500, 3000):
        t = random_text(n, 100 * seed + n)
        assert nm.normalize(t, PERCENT).out == urllib.parse.unquote_to_bytes(t)
        assert nm.normalize(t, SQUEEZE).out == squeeze(t)
        assert nm.normalize(t, STRIP).out == strip(t)
        assert nm.normalize(t, PERCENT | SQUEEZE).out == squeeze(urllib.parse.unquote_to_bytes(t))
        assert nm.normalize(t, PERCENT | STRIP).out == strip(urllib.parse.unquote_to_bytes(t))
        assert nm.normalize(t, 0).out == t
        assert nm.normalize(t, STRIP, blanks=b"\0%4").out == t.translate(None, b"\0%4")


@pytest.mark.parametrize("flags", MODES)
def test_segmented_is_per_text(flags):
    rng = np.random.default_rng(flags)
    t = random_text(4000, 7 + flags)
    starts = np.sort(rng.integers(0, 4001, 60)).tolist()
    starts = starts[:20] + starts[19:20] + starts[20:]                      # an empty text
    origin = -50 if flags & PERCENT else 0                                  # (starts in front of and behind the text)
    r = nm.normalize(t, flags, seg_start=starts, origin=origin)
    cl = [min(max(s, origin), origin + 4000) - origin for s in starts]
    cuts = sorted(set([0] + cl + [4000]))
    parts = [nm.normalize(t[a:b], flags).out for a, b in zip(cuts[:-1], cuts[1:])]
    assert r.out == b"".join(parts)
    ends = np.cumsum([0] + [len(p) for p in parts])
    assert r.seg_out.tolist() == [int(ends[cuts.index(c)]) for c in cl]


def test_cli_spec_and_refused_combinations(lib, tmp_path):
    """acm_grep refuses at start-up, before it looks for a device: the SPEC parser and every refused combination"""
    import test_gpu_normalize_cli as cli
    cli.check_refusals(cli.refusals(tmp_path))


def local_keep(t, flags, starts, blanks=BLANKS):
    """the local rule of DESIGN.md 6u: byte i by bytes i - 3 .. i + 2"""
    n = len(t)
    st = set(starts) | {0}
    blanks = set(blanks) if flags & (SQUEEZE | STRIP) else set()

    def head(i):
        return bool(flags & PERCENT) and 0 <= i and i + 2 < n and t[i] == 0x25 and t[i + 1] in nm.HEX and t[i + 2] in nm.HEX \
            and i + 1 not in st and i + 2 not in st

    def value(i):
        return int(t[i + 1:i + 3], 16) if head(i) else t[i]

    keep = np.zeros(n, dtype=bool)
    for i in range(n):
        if head(i - 1) or head(i - 2):
            continue
        if value(i) not in blanks:
            keep[i] = True
        elif flags & SQUEEZE:
            prev_blank = i not in st and ((value(i - 3) in blanks) if head(i - 3) else (t[i - 1] in blanks))
            keep[i] = not prev_blank
    return keep


@pytest.mark.parametrize("flags", MODES)
def test_the_local_rule_is_the_serial_walk(flags):
    rng = np.random.default_rng(40 + flags)
    for n in (1, 2, 3, 4, 5, 64, 2000):
        for k in range(8):
            t = random_text(n, 1000 * flags + 10 * n + k)
            starts = sorted(set(rng.integers(0, n + 1, rng.integers(0, max(n // 8, 2))).tolist()))
            r = nm.normalize(t, flags, seg_start=starts)
            assert np.array_equal(r.keep, local_keep(t, flags, [s for s in starts if s < n])), (n, k, t, starts)


# ------------------------------------------------------------------ the inputs of the GPU tests past one buffer


def test_scale_inputs_are_what_they_are_meant_to_be():
    """what test_gpu_normalize_scale.py states about its inputs, from the model alone: more starts and more output than
    the largest grid has threads, equal consecutive d_block cells in every text of dropped cells, the starts of the
    wildcard records on offset 0, at -1, on a triple and on a squeezed run's blank"""
    import test_gpu_normalize_scale as sc
    for flags in (PERCENT | SQUEEZE, PERCENT | STRIP):
        text, starts, x = sc.check_grid_case(flags)
        assert x.m > 262144 and starts.size == 300000
        sc.check_wild_case(flags)
    for name, t, modes, starts, least in sc.dropped_cell_texts():
        for flags in modes:
            x = nm.normalize(t.tobytes(), flags)
            assert sc.equal_cells(x) >= least >= 1, (name, flags)
            assert any(x.block[s // nm.BLOCK] == x.block[s // nm.BLOCK + 1] for s in starts if s < t.size), name   # a start in a dropped cell
    period, p = sc.tiled_period()
    offs = sc.tiled_offsets(p, period.size, sc.REPS)
    assert offs.max() == sc.REPS * p.m + 1 and 2000 < offs.size < 5000
    tiled = sc.Tiled(p, period.size, sc.REPS)
    assert tiled.last[p.m] == period.size + p.last[0] and tiled.first[tiled.m - 1] == (sc.REPS - 1) * period.size + p.first[-1]


def test_chain_inputs_are_what_they_are_meant_to_be():
    """what test_gpu_normalize_chain.py states about its inputs: m % 16 is 1 and 15, more than 1000 matches in every case,
    one that ends on a triple and one that starts on a squeezed run's blank, parts cut inside a triple and a run, empty
    parts and parts that strip to nothing, exact patterns dropped where folding ones are kept"""
    import test_gpu_normalize_chain as ch
    assert sorted({(s, ph) for s, ph, _ in ch.SHAPES}) == [("one", 1), ("one", 15), ("texts", 1), ("texts", 15)]
    for shape, phase, flags in ch.SHAPES:
        for name in ch.CASES:
            ch.check_expected(name, shape, phase, flags)
    assert ch.no_suffixes(ch.PLAIN) and ch.no_suffixes(ch.NOCASE) and ch.no_suffixes(ch.MIXED) and not ch.no_suffixes(ch.MIXED_ALL)
    assert all(len(p) >= 3 for p, _ in ch.PLAIN)
