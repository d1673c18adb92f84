"""The sparse pipeline's check kernel on sets and texts BUILT to force its lookup tables and loops into chosen
states (sieve_model.py; the promises are checked on the host by test_host_sieve_tables.py): gram chains through
the last bucket, prefix chains through the last slot, fan-outs either side of an edge level, unary runs either
side of a compare level and of the text's end, followers with hits either side of the four a lane keeps.

Every case scans in sparse mode, asserts that the sparse pipeline produced the planes, and compares offsets,
pattern ids and last state bit for bit with the oracle and with the chain pipeline's planes.  Every case runs
alone (blocks of 8 tiles) and as batch 2 of a launch group of four equal-size batches (blocks of 16 tiles), its
neighbours random text.  Which check kernel a launch gets depends on the flagged samples of the matcher's last batch
(more than one per 512 bytes: helper waves, sub-rows, blocks of 8 tiles even in a group) and the library does not
report it, so every run is put behind a batch that decides it: a quiet text (no flagged sample; the host test
proves that) in front of the plain runs, a sample-heavy one in front of the primed runs.
"""
import numpy as np
import pytest

import sieve_model as sm
from gpu_pattern_matching_amd import DeviceArray, Matcher

pytestmark = pytest.mark.gpu


def assert_same(got, exp, what):
    assert got[0].size == exp[0].size, "%s: record count %d != %d" % (what, got[0].size, exp[0].size)
    assert np.array_equal(got[0], exp[0]), "%s: offsets differ" % what
    assert np.array_equal(got[1], exp[1]), "%s: pattern ids differ" % what
    assert got[2] == exp[2], "%s: final state %d != %d" % (what, got[2], exp[2])


def planes_of(pat, off, cap, stream):
    p, q = pat.to_numpy(np.int32, cap, stream=stream), off.to_numpy(np.int32, cap, stream=stream)
    c = int(p[0])
    return q[1:1 + c].astype(np.uint32), p[1:1 + c].copy(), int(p[c + 1])


def in_a_group(m, t, exp, seed):
    """t as batch 2 of four equal-size batches in one launch group; the others are random bytes"""
    n = t.size
    rng = np.random.default_rng(seed)
    texts = [rng.integers(0, 256, size=n, dtype=np.uint8) for _ in range(4)]
    texts[2] = t
    ws_bytes = m.lib.acm_scan_workspace_bytes(m.dfa, n)
    cap = n + 2
    bufs = [DeviceArray.from_numpy(x) for x in texts]
    wss = [DeviceArray(ws_bytes) for _ in texts]
    planes = [(DeviceArray(cap * 4), DeviceArray(cap * 4)) for _ in texts]
    try:
        assert m.group_capable()
        m.enqueue_many([m.make_batch(bufs[k], n, m.stream, planes[k][0], planes[k][1], cap, (wss[k], ws_bytes))
                        for k in range(4)])
        assert_same(planes_of(planes[2][0], planes[2][1], cap, m.stream), exp, "batch 2 of a launch group")
        assert m.path_taken(n, workspace=(wss[2], ws_bytes)) == "sparse"
    finally:
        for b in bufs + wss + [x for pr in planes for x in pr]:
            b.free()


def run_case(name, states=False):
    c = sm.case(name)
    a, o = c.compiled()
    m = Matcher(a, 0, max_text=max(t.size for t in c.texts))
    try:
        assert m.sparse_eligible()
        for i, t in enumerate(c.texts):
            what = "%s text %d" % (name, i)
            exp = o.scan(c.oracle_text(t))
            assert m.set_mode("sparse") == "sparse"
            quiet = c.quiet_text(t.size)

            def behind_quiet():   # the next launch: no helper waves (one row per block; 16 tiles in a group)
                assert m.scan(quiet)[0].size == 0

            if i in c.primed:     # behind a sample-heavy batch: helper waves, blocks cut into sub-rows of 256 samples
                prime = c.priming_text(t.size)
                assert_same(m.scan(prime), o.scan(c.oracle_text(prime)), what + " priming batch")
                assert_same(m.scan(t), exp, what + " behind a priming batch")
                assert m.path_taken(t.size) == "sparse"
            behind_quiet()
            got = m.scan(t)
            assert m.path_taken(t.size) == "sparse"
            assert_same(got, exp, what + " alone")
            if states:   # the same through the final-state report (what all-patterns reporting expands)
                exp_all = o.scan_all(c.oracle_text(t))
                assert_same(m.scan_all(t, out_capacity=exp_all[0].size + 16), exp_all, what + " state report")
                assert m.path_taken(t.size) == "sparse"
            behind_quiet()
            in_a_group(m, t, exp, seed=i)
            assert m.set_mode("chain") == "chain"
            assert_same(m.scan(t), got, what + " chain pipeline")
            assert m.path_taken(t.size) == "chain"
    finally:
        m.close()
        a.close()
        o.close()


@pytest.mark.parametrize("shortest", sm.GRAM_SHORTEST)
def test_gram_chains(gpu, shortest):
    """W = 1, 2, 4, 8: patterns whose 3-gram sits at probe 1, 2 and 3 of a chain that wraps from the last bucket to
    bucket 0, the grams 000000 and FFFFFF, and absent grams the filter passes that walk the chain and are rejected"""
    run_case("gram_chain_s%d" % shortest)


@pytest.mark.parametrize("name", sorted(k for k in sm.BUILDERS if k.startswith("prefix_chain")))
def test_prefix_chains(gpu, name):
    """D = 3, 5, 8, 9, 10: keys at probe 1..4 of a chain through the last slot, absent keys at a chain's head behind a
    real gram, keys that differ in byte 8 or 9 only (D = 10), bytes behind a shorter key (D < 10); one nocase set"""
    run_case(name)


@pytest.mark.parametrize("k", sm.FANOUTS)
def test_fanout(gpu, k):
    """a node with k children, four edges a load level: every child, below the first, above the last, every gap;
    pattern ids and final states"""
    run_case("fanout_%d" % k, states=True)


@pytest.mark.parametrize("name", sorted((k for k in sm.BUILDERS if k.startswith("run_")), key=lambda s: (len(s), s)))
def test_runs(gpu, name):
    """unary runs of 63..200 bytes: whole, wrong at run byte 1, 63, 64, 65 and the last, and cut by the end of the
    text 0..80 bytes behind the depth-D byte (64-byte compares and the byte-wise tail)"""
    run_case(name)


@pytest.mark.parametrize("k", sm.HITS)
def test_hits_per_follower(gpu, k):
    """a follower with 3, 4, 5, 6 or 12 hits (four stay in registers, more take the count and write passes): alone,
    partly and wholly shadowed by a longer follower, and next to one-hit followers in the same round"""
    run_case("hits_%d" % k, states=True)


@pytest.mark.parametrize("which", sm.SEAMS)
def test_seams(gpu, which):
    """a count swept across each seam between two storage places or two loops of the check kernel: 30..35 flagged
    samples in one tile (32 in the dense head), 6..11 surviving hits in one row (8 in the dense head), 62..67 and
    126..130 followers in one block (64 a stage-2 round), a block whose stage-1 rounds add 512 followers to what the
    last round left (the queue of 576), 254..259 flagged samples in one block (sub-rows of 256) with and without a
    priming batch"""
    run_case("seam_%s" % which)
