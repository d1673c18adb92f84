"""The sparse pipeline's lookup tables on the host (csrc/sieve_image.cpp, acm_sieve_selftest) -- no GPU: every
fixture set and every sparse regime passes the self-test; sets that do not qualify are turned down; the Python
model of sieve_model.py reproduces the library's stats; and every constructed set and text keeps the promise
its GPU test (test_gpu_sieve_tables.py) relies on."""
import os

import numpy as np
import pytest

import fixtures
import orc
import sieve_model as sm
import variants
from gpu_pattern_matching_amd import Automaton

MODEL_STATS = ("W", "D", "LG", "bloom_log_words", "bloom_popcount", "keys", "grams", "gram_log_buckets", "full_buckets",
               "prefix_log_slots", "occupied_slots")


def check(lib, a):
    rc, st = sm.selftest(lib, a)
    assert rc in (0, 1), lib.acm_last_error()
    return rc, st


def assert_model(model, st):
    exp = model.expected_stats()
    assert {k: st[k] for k in MODEL_STATS} == {k: exp[k] for k in MODEL_STATS}


@pytest.mark.parametrize("name", ["clamav2000", "clamav10000", "clamav15000", "tests", "tests1", "tests2", "tests3"])
def test_fixture_sets(lib, name):
    path, hx, ml = fixtures.set_source(name)
    a = Automaton()
    a.load_file(path, hx, ml)
    a.compile()
    rc, st = check(lib, a)
    shortest = min(len(p) for p in fixtures.patterns_of(name))
    assert rc == (1 if shortest >= 3 else 0), (name, shortest, st)
    if rc:
        assert st["W"] == sm.sieve_stride(shortest) and st["D"] == min(shortest, 10)
        assert st["gram_probes"] >= 1 and st["prefix_probes"] >= 1 and st["occupied_slots"] > 0
        assert_model(sm.Model(fixtures.patterns_of(name)), st)
    a.close()


def test_clamav_sets_qualify(lib):
    """(the headline sets are on the sparse pipeline: the parametrised test above must not pass by rc == 0)"""
    for name in ("clamav2000", "clamav15000"):
        assert min(len(p) for p in fixtures.patterns_of(name)) >= 3


SPARSE_REGIMES = sorted(k for k in variants.REGIMES if k.startswith("s"))


@pytest.mark.parametrize("name", SPARSE_REGIMES)
def test_sparse_regimes(lib, name):
    vs = variants.regime(name)
    a, o = vs.compiled()
    rc, st = check(lib, a)
    assert rc == 1, st
    assert (st["W"], st["D"], st["LG"]) == (vs.stride, min(vs.shortest, 10), vs.key_len)
    assert_model(sm.Model(vs.patterns, vs.nocase), st)
    a.close()
    o.close()


def test_sets_that_do_not_qualify(lib):
    a = Automaton()
    a.load_file(os.path.join(orc.DATA, "sentiment", "patterns_categorical.txt"), False, -1)
    a.compile()
    rc, st = check(lib, a)
    assert rc == 0 and not any(st.values())       # a 2-byte pattern
    a.close()
    a = Automaton()
    a.compile()
    assert check(lib, a)[0] == 0                  # the empty set
    a.close()


@pytest.mark.parametrize("name", sorted(sm.BUILDERS))
def test_constructed_sets_keep_their_promise(lib, name):
    c = sm.case(name)
    a, o = c.compiled()
    rc, st = check(lib, a)
    assert rc == 1, st
    for key, (lo, hi) in c.promise.items():
        assert st[key] >= lo and (hi is None or st[key] <= hi), (key, st[key], lo, hi)
    assert_model(sm.Model(c.patterns, c.nocase), st)
    for t in c.texts:
        assert 8 * 1024 <= t.size <= 256 * 1024
        assert o.scan(c.oracle_text(t))[0].size > 0, "a text without a single record"
    a.close()
    o.close()


def test_gram_chain_texts(lib):
    """the gram-chain texts hold absent grams the filter flags, and the sets have the chain's wrap"""
    for s in sm.GRAM_SHORTEST:
        c = sm.case("gram_chain_s%d" % s)
        m = sm.Model(c.patterns)
        last = (1 << m.gram_log_buckets) - 1
        assert m.bucket_load[last] == 4 and m.bucket_load[0] == 4
        homes = [sm.sieve_gram_bucket(g, m.gram_log_buckets) for g in m.grams]
        assert homes.count(last) >= 9             # four in the last bucket, four in bucket 0, the ninth at probe 3
        assert 0 in m.grams and 0xFFFFFF in m.grams
        assert c.notes["absent"] >= 4


def test_prefix_chain_sets(lib):
    for name in sorted(k for k in sm.BUILDERS if k.startswith("prefix_chain")):
        c = sm.case(name)
        m = sm.Model(c.patterns, c.nocase)
        last = (1 << m.prefix_log_slots) - 1
        homes = list(m.slot_home.values())
        assert homes.count(last) >= 3 and m.slot_load[0] == 1 and m.slot_load[1] == 1, name


def test_run_cuts_reach_every_compare_path():
    """which of the follower's compares (64 bytes at once where the padded text has room, else byte by byte) each cut
    text is meant for: from n and the library's padding of n to a multiple of 16.  (The branch between the two in
    follow(), x + 65 <= n_pad, is the roomy condition itself while a level is 64 bytes: no text can reach it.)"""
    for r in sm.RUNS:
        paths = sm.case("run_%d" % r).notes["paths"]
        assert set(paths) == set(sm.RUN_CUTS)
        assert paths[80] == "roomy" and paths[65] == "roomy" and paths[64] == "roomy"
        assert all(paths[c] == "bytewise" for c in (0, 1, 15, 16, 17))
        assert paths[63] == "roomy"       # n = 8268, padded to 8272: the 64 bytes behind the depth-D byte are there


def in_block(per_tile, at, tiles):
    return int(per_tile[at // sm.TILE:at // sm.TILE + tiles].sum())


@pytest.mark.parametrize("name", sorted(sm.BUILDERS))
def test_constructed_texts_reach_their_state(lib, name):
    """For every constructed text: the flagged samples per tile (the model's filter), the followers and the hits the
    shadow leaves (derived from the pattern list, tied to the oracle by the record count) are what the GPU test of the
    case relies on -- the counts a seam case names, in the row of 8 tiles and in the row of 16; for every case that
    each follower's sample is one the filter flags, and that the text has followers and records at all."""
    c = sm.case(name)
    m = c.model()
    a, o = c.compiled()
    quiet = c.quiet_text(8192)
    assert m.flagged_positions(quiet).size == 0 and o.scan(c.oracle_text(quiet))[0].size == 0
    for i, t in enumerate(c.texts):
        flagged, fol, hit, fols, kept = sm.counts(m, t)
        rec = o.scan(c.oracle_text(t))
        kept_at = sorted(e for k in kept for e in k)
        assert kept_at == rec[0].tolist(), "%s text %d: the followers' surviving hits are not the oracle's records" % (name, i)
        assert len(fols) > 0 and rec[0].size > 0
        fl = set(m.flagged_positions(t).tolist())
        assert all(f[1] in fl for f in fols if f[1] + 3 <= t.size), "a follower's sample is not flagged"
        e = c.expect.get(i, {})
        at = sm.SEAM_AT
        if "tile_flagged" in e:
            tile, k = e["tile_flagged"]
            assert flagged[tile] == k, (flagged[tile], k)
            assert flagged[tile - 1] == 0 and flagged[tile + 1] == 0
        if "block_flagged" in e:
            assert in_block(flagged, at, 8) == e["block_flagged"] == in_block(flagged, at, 16)
            assert flagged[at // sm.TILE:at // sm.TILE + 8].max() > 32      # (and tiles beyond the dense head of 32)
        if "block_hits" in e:
            assert in_block(hit, at, 8) == e["block_hits"] == in_block(hit, at, 16)
        if "block_followers" in e:
            assert in_block(fol, at, 8) == e["block_followers"] == in_block(fol, at, 16)
        if "block_followers_over" in e:
            assert in_block(fol, at, 8) > e["block_followers_over"] and in_block(fol, at, 8) == in_block(fol, at, 16)
            per_sample = np.bincount(np.array([f[1] for f in fols]) // m.W)
            assert per_sample.max() == e["followers_per_sample"] == m.W
            # 64 consecutive samples with 8 followers each: a stage-1 round adds 512 to what the last round left
            full = (per_sample == m.W).astype(np.int64)
            runs = np.convolve(full, np.ones(64, dtype=np.int64), "valid")
            assert runs.max() == 64
        if i in c.primed:
            prime = c.priming_text(t.size)
            assert m.flagged_positions(prime).size > t.size // 512          # sparse.hip: kHeavyDivisor
        assert m.flagged_positions(c.quiet_text(t.size)).size == 0 if i == 0 else True
    a.close()
    o.close()


def test_every_seam_value_is_swept():
    want = dict(seam_tile=("tile_flagged", range(30, 36)), seam_hits=("block_hits", range(6, 12)),
                seam_followers=("block_followers", list(range(62, 68)) + list(range(126, 131))),
                seam_block=("block_flagged", range(254, 260)))
    for name, (key, ks) in want.items():
        c = sm.case(name)
        got = [c.expect[i][key] for i in range(len(c.texts))]
        got = [g[1] if isinstance(g, tuple) else g for g in got]
        assert got == list(ks), (name, got)
    assert len(sm.case("seam_block").primed) == 6 and len(sm.case("seam_queue").texts) >= 1


@pytest.mark.parametrize("k", sm.HITS)
def test_hit_settings(lib, k):
    """The follower of the nested path has k hits: alone it keeps all k; behind the `some` follower it keeps some but
    not all; behind the `whole` follower none (a lane with more than four hits that the shadow empties when k > 4);
    and a follower with k hits and one with a single hit are neighbours in follower order (the same stage-2 round)."""
    c = sm.case("hits_%d" % k)
    m = c.model()
    fols = sm.followers(m, c.texts[0])
    kept = sm.surviving(fols)
    assert len(fols) < 64                                        # one stage-2 round holds them all
    pairs = [(len(f[3]), len(kp)) for f, kp in zip(fols, kept)]
    assert (k, k) in pairs, pairs                                # alone
    assert any(h == k and 0 < kp < k for h, kp in pairs), pairs  # partly shadowed
    assert (k, 0) in pairs, pairs                                # wholly shadowed
    assert any({pairs[i][0], pairs[i + 1][0]} == {k, 1} and pairs[i][1] and pairs[i + 1][1]
               for i in range(len(pairs) - 1)), pairs            # a k-hit and a one-hit follower side by side, both keeping hits
    assert max(h for h, _ in pairs) >= k


def test_hit_counts(lib):
    """the nested patterns give the follower of the planted path exactly k final nodes"""
    for k in sm.HITS:
        c = sm.case("hits_%d" % k)
        a, o = c.compiled()
        p = max(c.patterns[:k], key=len)
        t = np.frombuffer(b"~~~~" + p + b"~~~~", dtype=np.uint8)
        assert o.scan(t)[0].size == k
        a.close()
        o.close()
