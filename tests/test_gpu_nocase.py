"""ASCII case-insensitive matching on the device (acm_automaton_set_nocase): every pipeline, bit
for bit against the oracle of the folded patterns on the folded text.

Texts are the usual fixtures with the case of their ASCII letters flipped at random, and a text
with every byte value next to every letter.
"""
import os

import numpy as np
import pytest

import fixtures
import orc
import streams
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher
from gpu_pattern_matching_amd._lib import check
from test_host_nocase import fold, folded_oracle, scramble

pytestmark = pytest.mark.gpu

MiB = 1 << 20


def nocase_matcher(name, max_text, nocase=True):
    path, hx, max_len = fixtures.set_source(name)
    a = Automaton(nocase=nocase)
    a.load_file(path, hx, max_len)
    a.compile()
    m = Matcher(a, 0, max_text=max_text)
    a.close()
    return m


def assert_same(got, exp):
    assert got[0].size == exp[0].size, "record count %d != %d" % (got[0].size, exp[0].size)
    assert np.array_equal(got[0], exp[0]), "offsets differ"
    assert np.array_equal(got[1], exp[1]), "pattern indices differ"
    assert got[2] == exp[2], "final state %d != %d" % (got[2], exp[2])


def all_bytes_around_letters():
    """every byte value in front of and behind every letter, in both cases"""
    parts = []
    for c in range(ord("A"), ord("Z") + 1):
        for b in range(256):
            parts.append(bytes([b, c, b, c | 0x20, b]))
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


def text_of(name, n, seed):
    pats = fixtures.patterns_of(name)
    if name.startswith("clamav"):
        t = fixtures.text_for({"kind": "clamav", "n": n, "seed": seed, "n_plant": max(4, n // 2048)}, pats)
    elif name == "sentiment":
        t = fixtures.text_for({"kind": "words", "n": n, "seed": seed}, pats)
    else:
        t = np.fromfile(os.path.join(orc.DATA, "ref_tests", "input.txt"), dtype=np.uint8)
        t = np.tile(t, n // max(t.size, 1) + 1)[:n]
    return scramble(t, seed)


SIZES = [3, 17, 1000, 4096 + 7, 65536 + 13, MiB + 5]


@pytest.mark.parametrize("mode", ["auto", "sparse", "chain"])
def test_clamav2000_modes(gpu, mode):
    name = "clamav2000"
    o = folded_oracle(name)
    m = nocase_matcher(name, 32 * MiB)
    assert m.set_mode(mode) == mode
    for k, n in enumerate(SIZES + [32 * MiB - 3]):
        text = text_of(name, n, 100 + k)
        assert_same(m.scan(text), o.scan(fold(text)))
    text = all_bytes_around_letters()
    assert_same(m.scan(text), o.scan(fold(text)))
    m.close()


def test_sparse_path_is_taken(gpu):
    m = nocase_matcher("clamav2000", MiB)
    assert m.sparse_eligible()
    m.set_mode("sparse")
    text = text_of("clamav2000", MiB, 3)
    m.scan(text)
    assert m.path_taken(text.size) == "sparse"
    m.close()


@pytest.mark.parametrize("name", ["clamav15000_m12", "sentiment", "tests"])
@pytest.mark.parametrize("mode", ["auto", "chain"])
def test_sets(gpu, name, mode):
    o = folded_oracle(name)
    m = nocase_matcher(name, 4 * MiB)
    m.set_mode(mode)
    for k, n in enumerate([5, 333, 4096 * 3 + 1, MiB - 1, 4 * MiB]):
        text = text_of(name, n, 200 + k)
        assert_same(m.scan(text), o.scan(fold(text)))
    text = all_bytes_around_letters()
    assert_same(m.scan(text), o.scan(fold(text)))
    m.close()


def test_lds_walk_sentiment(gpu):
    name = "sentiment"
    o = folded_oracle(name)
    m = nocase_matcher(name, 32 * MiB)
    assert m.lds_resident()
    for k, n in enumerate(SIZES + [8 * MiB + 1, 32 * MiB]):
        text = text_of(name, n, 300 + k)
        assert_same(m.scan(text), o.scan(fold(text)))
    m.close()


@pytest.mark.parametrize("name,mode", [("clamav2000", "sparse"), ("clamav2000", "chain"), ("sentiment", "auto")])
def test_carry_across_a_split_text(gpu, name, mode):
    o = folded_oracle(name)
    m = nocase_matcher(name, MiB)
    m.set_mode(mode)
    text = text_of(name, MiB, 7)
    exp = o.scan(fold(text))
    for cut in (1, 4097, MiB // 2 + 3):
        p1 = m.scan(text[:cut])
        p2 = m.scan(text[cut:], init_state=p1[2])
        got = (np.concatenate([p1[0], p2[0] + cut]).astype(np.uint32), np.concatenate([p1[1], p2[1]]), p2[2])
        assert_same(got, exp)
    m.close()


@pytest.mark.parametrize("name", ["clamav2000", "sentiment"])
def test_launch_group_of_mixed_sizes(gpu, name):
    o = folded_oracle(name)
    m = nocase_matcher(name, 4 * MiB)
    sizes = [4 * MiB, 4 * MiB, 4 * MiB, MiB + 3, 4 * MiB, 100, 4 * MiB]
    texts = [text_of(name, n, 400 + k) for k, n in enumerate(sizes)]
    cap = 4 * MiB + 2
    ws_bytes = m.lib.acm_scan_workspace_bytes(m.dfa, 4 * MiB)
    d_texts = [DeviceArray.from_numpy(t) for t in texts]
    wss = [DeviceArray(ws_bytes) for _ in sizes]
    planes = [(DeviceArray(cap * 4), DeviceArray(cap * 4)) for _ in sizes]
    inits = [0, 0, 5, 0, 0, 0, 0]
    m.enqueue_many([m.make_batch(d_texts[k], sizes[k], m.stream, planes[k][0], planes[k][1], cap, (wss[k], ws_bytes),
                                 init_state=inits[k]) for k in range(len(sizes))])
    for k in range(len(sizes)):
        p = planes[k][0].to_numpy(np.int32, cap, stream=m.stream)
        q = planes[k][1].to_numpy(np.int32, cap, stream=m.stream)
        c = int(p[0])
        assert_same((q[1:1 + c].astype(np.uint32), p[1:1 + c], int(p[c + 1])), o.scan(fold(texts[k]), init_state=inits[k]))
    for b in d_texts + wss + [x for pr in planes for x in pr]:
        b.free()
    m.close()


@pytest.mark.parametrize("mode", ["auto", "chain", "sparse"])
def test_graph_mode(gpu, mode):
    """graph replay of a nocase scan on a stream of its own (the NULL stream is never captured): the text
    changes between the replays, and acm_scan_graph_stats shows one capture and R - 1 launches per key"""
    name = "clamav2000"
    o = folded_oracle(name)
    m = nocase_matcher(name, MiB)
    m.set_mode(mode)
    n = MiB
    d = DeviceArray(n)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.set_graphs(True)
        paths, keep = [], []
        for seed in range(4):
            text = text_of(name, n, 500 + seed)
            keep.append(text)
            check(m.lib.acm_rt_memcpy_h2d(d.ptr, text.ctypes.data, n, s), "h2d")
            m.pat_plane.fill(0xEE, s)
            m.off_plane.fill(0xEE, s)
            m.scan_async(d, n, stream=s)
            assert_same(m.fetch(stream=s), o.scan(fold(text)))
            paths.append(m.path_taken(n, stream=s))
        if mode != "auto":
            assert paths == [mode] * 4
        counts = [paths.count(p) for p in set(paths)]     # the pipeline is part of the key
        got = m.graph_stats()
        assert got == (sum(1 for c in counts if c >= 2), sum(c - 1 for c in counts)), (got, paths)
        assert got[1] > 0                                 # for one pipeline (1, 3)
        assert m.set_graphs(-1) is True                   # no silent fall-back
    finally:
        m.set_graphs(False)
        rig.close()
        d.free()
        m.close()


@pytest.mark.parametrize("name,mode", [("clamav2000", "sparse"), ("clamav2000", "chain"), ("sentiment", "auto")])
def test_shard_with_halo(gpu, name, mode):
    o = folded_oracle(name)
    m = nocase_matcher(name, 2 * MiB)
    m.set_mode(mode)
    halo = max(len(p) for p in fixtures.patterns_of(name)) - 1
    text = text_of(name, 2 * MiB, 9)
    pats = fixtures.patterns_of(name)
    # a pattern across the border between the shards, in mixed case
    border = MiB
    p = scramble(np.frombuffer(max(pats, key=len), dtype=np.uint8), 1)
    text[border - p.size // 2:border - p.size // 2 + p.size] = p
    whole = o.scan(fold(text))
    assert np.any((whole[0] >= border) & (whole[0] < border + p.size))
    pos_all, pat_all = [], []
    for lo, hi in ((0, border), (border, text.size)):
        h = min(halo, lo)
        d = DeviceArray.from_numpy(np.ascontiguousarray(text[lo - h:hi]))
        m.scan_async(d, hi - lo + h, halo=h, offset_shift=lo - h)
        pos, pat, _ = m.fetch()
        d.free()
        pos_all.append(pos)
        pat_all.append(pat)
    assert np.array_equal(np.concatenate(pos_all), whole[0])
    assert np.array_equal(np.concatenate(pat_all), whole[1])
    m.close()


@pytest.mark.parametrize("name", ["tests", "sentiment", "clamav2000"])
def test_all_patterns_expansion(gpu, name):
    o = folded_oracle(name)
    m = nocase_matcher(name, MiB)
    text = text_of(name, 256 * 1024, 12)
    got = m.scan_all(text)
    exp = o.scan_all(fold(text))
    assert_same(got, exp)
    m.close()


def test_nocase_and_case_sensitive_alive_together(gpu):
    """Two LDS-resident matchers of one set, the nocase one uploaded second, scanned in alternation;
    and a larger LDS-resident automaton uploaded before a smaller one keeps working."""
    name = "sentiment"
    o_fold = folded_oracle(name)
    o_plain = fixtures.oracle_for(name)
    big = nocase_matcher(name, 4 * MiB, nocase=False)
    small = nocase_matcher("tests", 4 * MiB, nocase=True)
    nc = nocase_matcher(name, 4 * MiB, nocase=True)
    assert big.lds_resident() and nc.lds_resident()
    o_small = folded_oracle("tests")
    for k in range(3):
        text = text_of(name, 4 * MiB - k, 600 + k)
        a = nc.scan(text)
        b = big.scan(text)
        c = small.scan(text)
        assert_same(a, o_fold.scan(fold(text)))
        assert_same(b, o_plain.scan(text))
        assert_same(c, o_small.scan(fold(text)))
        assert a[0].size != b[0].size
    for x in (big, small, nc):
        x.close()
