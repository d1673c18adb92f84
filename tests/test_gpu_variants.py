"""Every scan-path kernel instantiation against the oracle.

The host picks a template instantiation per launch from the pattern set, the text size, the launch
group, how dense the previous batch was and the nocase flag.  ROWS below has one row per
instantiation (and per block-total path of the chain scatter): the regime of its set (variants.py),
the mode, chain bytes, chains per lane, launch-group size, whether a dense batch goes first (the check
kernel's helper waves), and at most one of the knobs acm_dfa_upload reads each time.  Every row must
give the oracle's planes bit for bit -- offsets, pattern ids, count, final state -- for head records on
two texts with carried-in states, for all-patterns reporting, and for a text cut inside a match; nocase
rows against the oracle of the folded patterns on the folded text.  The small rows also check a shard
with a halo and an offset shift, and a segmented scan.
"""
import numpy as np
import pytest

import variants
from gpu_pattern_matching_amd import DeviceArray, Matcher
from test_host_segments import oracle_segments, random_starts

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SMALL = 256 * 1024 + 37
BIG_TOTALS = (1 << 28) + 40013      # chains of 16 bytes: > 65536 scatter blocks of 256 chains


class Row:
    def __init__(self, kernel, regime, mode, n=SMALL, S=0, C=4, group=1, dense=False, env=None, lds=False,
                 kind="planted", cap=None):
        self.kernel, self.regime, self.mode, self.n = kernel, regime, mode, n
        self.S, self.C, self.group, self.dense, self.env, self.lds = S, C, group, dense, env or {}, lds
        self.kind, self.cap = kind, cap

    @property
    def path(self):
        return "sparse" if self.mode == "sparse" else "chain"


def sieve_rows():
    """k_sieve<W, false, LG, NC> and k_sieve_check<W, HELPED, TPC, NC>: a row per check kernel; the sets'
    shortest patterns also give every bulk kernel (W, LG) and every D = min(shortest, 10)."""
    table = {   # (W, nocase): regime of the TPC 8 row, of the helped row, of the TPC 16 row
        (1, False): ("s3_letters", "s3_binary_l192", "s3_letters"),
        (2, False): ("s4_c9", "s5_binary", "s4_letters"),
        (4, False): ("s6_c33", "s8_binary", "s9_letters"),
        (8, False): ("s10_letters", "s13_binary_l300", "s16_letters"),
        (1, True): ("s3_mixed", "s3_mixed", "s3_mixed"),
        (2, True): ("s4_mixed", "s5_mixed", "s4_mixed"),
        (4, True): ("s6_mixed", "s9_mixed", "s8_mixed"),
        (8, True): ("s12_mixed", "s10_mixed", "s13_mixed"),
    }
    rows = []
    for (w, nc), (plain, helped, wide) in table.items():
        for reg, how in ((plain, "8u"), (helped, "helped"), (wide, "16u")):
            vs = variants.regime(reg)
            assert vs.stride == w and vs.nocase == nc
            name = "k_sieve_check<%d, %s, %s, %s> k_sieve<%d, false, %d%s>" % (
                w, "true" if how == "helped" else "false", "8u" if how == "helped" else how, str(nc).lower(),
                w, vs.key_len, ", true" if nc else "")
            rows.append(Row(name, reg, "sparse", dense=how == "helped", group=4 if how == "16u" else 1,
                            kind="runs" if how == "8u" else "planted"))
    # a set whose shortest pattern allows W = 8, sampled at W = 1 (D = 10, 3-byte keys)
    rows.append(Row("k_sieve<1, false, 3> with D = 10 (ACM_SIEVE_STRIDE)", "s16_letters", "sparse",
                    env={"ACM_SIEVE_STRIDE": "1"}))
    return rows


ROWS = sieve_rows() + [
    # the chain pipeline's walk kernels (cold planes: not LDS-resident, or kept off the LDS walk)
    Row("k_halo_walk<true, true, 4, 768>", "l16_letters", "chain", S=64, env={"ACM_SCAN_NO_LDSWALK": "1"}),
    Row("k_halo_walk<false, true, 4, 768>", "l32_binary", "chain", S=32),
    Row("k_spec_walk<4, true, true>", "l40_c33", "chain", S=64),
    Row("k_spec_walk<4, false, true>", "l16_binary", "chain", S=32, env={"ACM_SCAN_NO_PRELOAD": "1"}),
    Row("k_halo_walk<true, false, 4, 768> k_probe<false> k_resolve<false>", "l80_c17", "chain", S=64),
    Row("k_halo_walk<false, false, 4, 768>", "l16_binary", "chain", S=64, env={"ACM_SCAN_HALO": "0"}),
    Row("k_spec_walk<4, true, false>", "l150_letters", "chain", S=32),
    Row("k_spec_walk<4, false, false>", "l64_binary", "chain", S=16),
    Row("k_spec_walk<4, true, false> k_probe<true> k_resolve<true>", "l60_mixed", "chain", S=16),
    Row("k_spec_walk<2, true, false> k_scatter_all<2>", "l40_c65", "chain", S=32, C=2),
    Row("k_spec_walk<2, false, false>", "l16_binary", "chain", S=64, C=2),
    Row("k_spec_walk<4, true, false> chains of 256 B, longest > 256", "l300_c5", "chain", S=256),
    Row("k_halo_walk<true, false, 2, 1024> (wide pre)", "l150_c9", "chain", n=16 * MiB + 5),
    Row("k_halo_walk<false, false, 2, 1024> (wide pre)", "l120_binary", "chain", n=16 * MiB + 5),
    Row("k_halo_walk<true, true, 4, 768> over > 16384 states", "big_c17", "chain", S=32),
    # block totals of the chain scatter: folded (every row above), k_scan_top, acm_exclusive_scan_i32
    Row("k_scan_top", "l16_binary", "chain", n=40 * MiB + 7, S=16, cap=1 << 21),
    Row("acm_exclusive_scan_i32 over the block totals", "l16_binary", "chain", n=BIG_TOTALS, S=16, cap=1 << 21),
    # the LDS walk
    Row("k_lds_walk<2, true, 5>", "lds16_letters", "chain", lds=True, kind="runs"),
    Row("k_lds_walk<2, true, 5> nocase", "lds12_mixed", "chain", lds=True),
    Row("k_lds_walk<2, true, 6>", "lds33_c33", "chain", lds=True),
    Row("k_lds_walk<2, true, 6> launch group", "lds33_c33", "chain", lds=True, group=4),
]


def assert_same(got, exp, what=""):
    assert got[0].size == exp[0].size, "%s: record count %d != %d" % (what, got[0].size, exp[0].size)
    assert np.array_equal(got[0], exp[0]), "%s: offsets differ" % what
    assert np.array_equal(got[1], exp[1]), "%s: pattern ids differ" % what
    assert got[2] == exp[2], "%s: final state %d != %d" % (what, got[2], exp[2])


def oracle_all(o, t, init):
    cap = 4 * t.size // 16 + 4096
    while True:
        try:
            return o.scan_all(t, init, cap=cap)
        except OverflowError:
            cap *= 4


def big_text(vs, n, seed):
    """n bytes from a shifted 16 MiB piece (bounded host memory), patterns planted on scatter-block and chain
    borders up to the end"""
    piece = variants.text(vs, 16 * MiB, seed, "random")
    t = np.empty(n, dtype=np.uint8)
    for at in range(0, n, piece.size):
        k = min(piece.size, n - at)
        t[at:at + k] = np.roll(piece, at >> 20)[:k]
    rng = np.random.default_rng(seed)
    for b in (4096, 4096 * 8192, 4096 * 65536, 16):
        for at in range(b, n, max(b, n // 64)):
            p = np.frombuffer(vs.patterns[int(rng.integers(len(vs.patterns)))], dtype=np.uint8)
            lo = at - int(rng.integers(1, p.size + 1))
            if 0 <= lo and lo + p.size <= n:
                t[lo:lo + p.size] = p
    p = np.frombuffer(max(vs.patterns, key=len), dtype=np.uint8)
    t[n - p.size:] = p   # a match that ends with the text
    return t


@pytest.mark.parametrize("row", ROWS, ids=[r.kernel for r in ROWS])
def test_instantiation(gpu, monkeypatch, row):
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    vs = variants.regime(row.regime)
    a, o = vs.compiled()
    n = row.n
    m = Matcher(a, 0, max_text=n, plane_capacity=row.cap)
    rng = np.random.default_rng(n + len(row.kernel))
    try:
        assert m.set_mode(row.mode) == row.mode
        if row.S:
            assert m.set_chain_bytes(row.S) == row.S
        assert m.set_chains_per_lane(row.C) == row.C
        assert m.sparse_eligible() == (vs.shortest >= 3)
        lds = vs.lds and "ACM_SCAN_NO_LDSWALK" not in row.env
        assert m.lds_resident() == lds
        if row.mode == "chain":   # a row of the LDS walk, or of the cold-plane walk kernels
            assert lds == row.lds
        make = (lambda s, kind: big_text(vs, n, s)) if n > 16 * MiB + 5 else \
            (lambda s, kind: variants.text(vs, n, s, kind))
        dense = variants.text(vs, n, 7, "dense") if row.dense else None
        exp_dense = o.scan(vs.text_of(dense)) if row.dense else None

        def prime():   # a batch with more than a flagged sample per 512 bytes: the next launch gets helper waves
            if row.dense:
                assert_same(m.scan(dense), exp_dense, "dense batch")

        # 1. head records, carried-in states
        texts = [make(11, row.kind), make(12, "planted")]
        inits = [int(rng.integers(0, o.num_states)) for _ in texts]
        if row.group > 1:
            texts += [make(13, "random"), make(14, row.kind)]
            inits += [0, int(rng.integers(0, o.num_states))]
            grouped(m, texts, inits, vs, o)
        for t, s in zip(texts, inits):
            prime()
            exp = o.scan(vs.text_of(t), s, cap=row.cap)
            assert_same(m.scan(t, s), exp, "head records")
            assert m.path_taken(n) == row.path
        assert exp[0].size > 0
        # 2. all-patterns reporting
        t, s = texts[1], inits[1]
        prime()
        assert_same(m.scan_all(t, s, out_capacity=(row.cap or n) * 8), oracle_all(o, vs.text_of(t), s), "all patterns")
        assert m.path_taken(n) == row.path
        # 3. a text cut inside a match, the state carried over
        whole = o.scan(vs.text_of(t), s, cap=row.cap)
        lens = np.array([0] + [len(p) for p in vs.patterns])
        long_ones = np.flatnonzero(lens[whole[1]] >= 2)
        k = int(long_ones[int(rng.integers(long_ones.size))])
        end, ln = int(whole[0][k]), int(lens[whole[1][k]])
        cut = end - int(rng.integers(0, ln - 1))
        assert end - ln + 1 < cut <= end
        prime()
        p1 = m.scan(t[:cut], s)
        prime()
        p2 = m.scan(t[cut:], p1[2])
        got = (np.concatenate([p1[0], p2[0] + np.uint32(cut)]), np.concatenate([p1[1], p2[1]]), p2[2])
        assert_same(got, whole, "cut at %d" % cut)
        if n <= SMALL:
            shard_with_halo(m, vs, o, t)
            segments(m, vs, o, t, s, rng)
    finally:
        m.close()
        a.close()
        o.close()


def grouped(m, texts, inits, vs, o):
    """acm_scan_batches_async with equal-size batches: one launch group (k_sieve_check blocks of 16 tiles)"""
    n = texts[0].size
    ws_bytes = m.lib.acm_scan_workspace_bytes(m.dfa, n)
    cap = n + 2
    bufs = [DeviceArray.from_numpy(t) for t in texts]
    wss = [DeviceArray(ws_bytes) for _ in texts]
    planes = [(DeviceArray(cap * 4), DeviceArray(cap * 4)) for _ in texts]
    try:
        m.enqueue_many([m.make_batch(bufs[k], n, m.stream, planes[k][0], planes[k][1], cap, (wss[k], ws_bytes),
                                     init_state=inits[k]) for k in range(len(texts))])
        for k, (t, s) in enumerate(zip(texts, inits)):
            p = planes[k][0].to_numpy(np.int32, cap, stream=m.stream)
            q = planes[k][1].to_numpy(np.int32, cap, stream=m.stream)
            c = int(p[0])
            assert_same((q[1:1 + c].astype(np.uint32), p[1:1 + c], int(p[c + 1])), o.scan(vs.text_of(t), s),
                        "batch %d of a launch group" % k)
    finally:
        for b in bufs + wss + [x for pr in planes for x in pr]:
            b.free()


def shard_with_halo(m, vs, o, t):
    """two shards, the second with the longest pattern's halo in front of it and its offsets shifted"""
    whole = o.scan(vs.text_of(t))
    border = t.size // 2 + 5
    halo = vs.longest - 1
    pos_all, pat_all = [], []
    for lo, hi in ((0, border), (border, t.size)):
        h = min(halo, lo)
        d = DeviceArray.from_numpy(np.ascontiguousarray(t[lo - h:hi]))
        m.scan_async(d, hi - lo + h, halo=h, offset_shift=lo - h)
        pos, pat, _ = m.fetch()
        d.free()
        pos_all.append(pos)
        pat_all.append(pat)
    assert np.array_equal(np.concatenate(pos_all), whole[0]), "shard offsets differ"
    assert np.array_equal(np.concatenate(pat_all), whole[1]), "shard pattern ids differ"


def segments(m, vs, o, t, init, rng):
    starts = random_starts(t.size, rng, vs.longest)
    starts = starts[starts > 0] if starts.size > 1 else starts   # bytes before the first start carry init
    for all_patterns in (False, True):
        got = m.scan_segments((t, starts), init_state=init, all_patterns=all_patterns, counts=True)
        exp = oracle_segments(o, vs.text_of(t), starts, init, all_patterns=all_patterns)
        assert np.array_equal(got[0], exp[0]), "segment offsets differ"
        assert np.array_equal(got[1], exp[1]), "segment pattern ids differ"
        assert np.array_equal(got[2], exp[2]), "segment ids differ"
        assert got[3] == exp[4], "segmented final state"
        assert np.array_equal(got[4], exp[3]), "per-segment counts differ"
