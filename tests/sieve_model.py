"""A Python model of the sparse pipeline's lookup tables (csrc/sieve_tables.h, csrc/sieve_image.cpp) and the
seeded searches that build pattern sets and texts which force the tables and the check kernel into chosen
states (a test helper, not a conftest).

The model is for CONSTRUCTING inputs and for counting what the filter flags.  It is never the expected
result of a scan: the oracle stays the only reference for planes.  test_host_sieve_tables.py pins the model to
the library through acm_sieve_selftest's stats on every set built here, and checks that every set and text
keeps the promise its GPU test relies on; a search that finds nothing raises AssertionError.
"""
import ctypes as C

import numpy as np

import variants

M32 = 0xFFFFFFFF
MUL_A, MUL_B, MUL_C, MUL_E, MUL_F = 0x9E3779, 0x85EBCA, 0xC2B2AF, 0xB5297B, 0x68E31D
MAX_PREFIX, MIN_LOG_WORDS, MAX_LOG_WORDS = 10, 8, 15
TILE = 1024          # bytes of a tile for texts up to 4 MiB (sparse.hip: kMinTile)

STATS = ("W", "D", "LG", "bloom_log_words", "bloom_popcount", "keys", "grams", "gram_log_buckets", "full_buckets",
         "gram_probes", "prefix_log_slots", "occupied_slots", "prefix_probes", "max_fanout", "longest_run", "edges",
         "fnv_bloom", "fnv_gram", "fnv_prefix", "fnv_rec", "fnv_edges")


def mul24(a, b):
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & M32


def sieve_bloom_block(gram, more, log_words):
    return ((mul24(gram, MUL_A) + mul24(more, MUL_E)) & M32) >> (33 - log_words)


def sieve_bloom_bits(gram, more):
    p = (mul24(gram, MUL_B) + mul24(more, MUL_F)) & M32
    lo = (1 << (p >> 27)) | (1 << ((p >> 22) & 31))
    hi = (1 << ((p >> 17) & 31)) | (1 << ((p >> 12) & 31))
    return lo | (hi << 32)


def sieve_gram_bucket(gram, log_buckets):
    return mul24(gram, MUL_C) >> (32 - log_buckets) if log_buckets else 0


def sieve_prefix_slot(k0, k1, k2, log_slots):
    h = (k0 * 0x9E3779B1) & M32
    h = ((h ^ (h >> 15) ^ k1) * 0x85EBCA6B) & M32
    h = ((h ^ (h >> 13) ^ k2) * 0xC2B2AE35) & M32
    return h >> (32 - log_slots) if log_slots else 0


def sieve_stride(m):
    return 8 if m >= 10 else 4 if m >= 6 else 2 if m >= 4 else 1


def gram_buckets_np(grams, log_buckets):
    """sieve_gram_bucket of a uint array of 3-grams"""
    g = np.asarray(grams, dtype=np.uint64)
    return (((g * np.uint64(MUL_C)) & np.uint64(M32)) >> np.uint64(32 - log_buckets)).astype(np.int64)


def gram_of(b):
    return b[0] | (b[1] << 8) | (b[2] << 16)


def key_words(key):
    """k0, k1, k2 of a prefix key of up to 10 bytes (the bytes beyond it zero)"""
    k = bytes(key) + bytes(12 - len(key))
    return int.from_bytes(k[0:4], "little"), int.from_bytes(k[4:8], "little"), int.from_bytes(k[8:12], "little")


def _linear_fill(homes, size, cap):
    """occupancy after inserting items with these home cells into `size` cells of `cap` places each, linear
    probing with wrap-around (the occupancy does not depend on the order of insertion)"""
    load = [0] * size
    for h in homes:
        while load[h] == cap:
            h = (h + 1) % size
        load[h] += 1
    return load


class Model:
    """What the host builder makes of a pattern list: W, D, LG, the gram set with its offset masks, the filter
    keys, the Bloom words, how full every gram bucket and every prefix slot is."""

    def __init__(self, patterns, nocase=False):
        pats = [variants.fold(p) if nocase else bytes(p) for p in patterns]
        self.patterns, self.nocase = pats, nocase
        shortest = min(len(p) for p in pats)
        assert shortest >= 3
        self.shortest = shortest
        self.W = W = sieve_stride(min(shortest, 64))
        self.D = D = min(shortest, MAX_PREFIX)
        self.LG = LG = 6 if (W + 5 <= shortest and W >= 4) else 3
        self.grams, self.keys = {}, set()
        for p in pats:
            for o in range(W):
                self.grams[gram_of(p[o:o + 3])] = self.grams.get(gram_of(p[o:o + 3]), 0) | (1 << o)
                self.keys.add((gram_of(p[o:o + 3]), gram_of(p[o + 3:o + 6]) if LG == 6 else 0))
        lw = MIN_LOG_WORDS
        while lw < MAX_LOG_WORDS and (1 << lw) < len(self.keys):
            lw += 1
        self.bloom_log_words = lw
        self.blocks = [0] * (1 << (lw - 1))
        for g, m in self.keys:
            self.blocks[sieve_bloom_block(g, m, lw)] |= sieve_bloom_bits(g, m)
        lb = 4
        while (1 << lb) < len(self.grams):
            lb += 1
        self.gram_log_buckets = lb
        self.bucket_load = _linear_fill([sieve_gram_bucket(g, lb) for g in self.grams], 1 << lb, 4)
        self.prefixes = sorted({p[:D] for p in pats})
        ls = 4
        while (1 << ls) < 8 * len(self.prefixes):
            ls += 1
        self.prefix_log_slots = ls
        self.slot_home = {k: sieve_prefix_slot(*key_words(k), ls) for k in self.prefixes}
        self.slot_load = _linear_fill(list(self.slot_home.values()), 1 << ls, 1)

    # -- what the library's stats must say of the same set
    def expected_stats(self):
        return dict(W=self.W, D=self.D, LG=self.LG, bloom_log_words=self.bloom_log_words,
                    bloom_popcount=sum(bin(b).count("1") for b in self.blocks), keys=len(self.keys),
                    grams=len(self.grams), gram_log_buckets=self.gram_log_buckets,
                    full_buckets=sum(1 for v in self.bucket_load if v == 4),
                    prefix_log_slots=self.prefix_log_slots, occupied_slots=sum(self.slot_load))

    def bloom_passes(self, gram, more=0):
        m = more if self.LG == 6 else 0
        bits = sieve_bloom_bits(gram, m)
        return self.blocks[sieve_bloom_block(gram, m, self.bloom_log_words)] & bits == bits

    def flagged_positions(self, text):
        """sample positions of `text` (uint8 array) the filter flags: p = 0 mod W with its key inside the text"""
        t = variants.fold(np.asarray(text, dtype=np.uint8)) if self.nocase else np.asarray(text, dtype=np.uint8)
        n = t.size
        out = []
        for p in range(0, n - 2, self.W):
            if self.LG == 6 and p + 6 > n:
                continue
            g = int(t[p]) | (int(t[p + 1]) << 8) | (int(t[p + 2]) << 16)
            m = (int(t[p + 3]) | (int(t[p + 4]) << 8) | (int(t[p + 5]) << 16)) if self.LG == 6 else 0
            if self.bloom_passes(g, m):
                out.append(p)
        return np.array(out, dtype=np.int64)

    def filler(self, seed=0):
        """two bytes (outside the set's alphabet where it leaves two) none of whose alternations' grams and keys the
        filter flags"""
        used = set(b"".join(self.patterns))
        if self.nocase:
            used |= {b + 0x20 for b in used if 0x41 <= b <= 0x5A}
        rng = np.random.default_rng(seed)
        free = [b for b in range(1, 255) if b not in used and not (0x41 <= b <= 0x5A) and not (0x61 <= b <= 0x7A)]
        if len(free) < 2:   # a set over all the bytes: any two whose alternation stays quiet
            free = [b for b in range(1, 255) if not (0x41 <= b <= 0x5A) and not (0x61 <= b <= 0x7A)]
        for _ in range(4096):
            x, y = (int(v) for v in rng.choice(free, size=2, replace=False))
            s = bytes([x, y] * 8)
            if not any(self.bloom_passes(gram_of(s[i:i + 3]), gram_of(s[i + 3:i + 6])) for i in (0, 1)):
                return x, y
        raise AssertionError("no quiet filler found")

    def filler_text(self, n, seed=0):
        x, y = self.filler(seed)
        t = np.empty(n, dtype=np.uint8)
        t[0::2], t[1::2] = x, y
        return t


def selftest(lib, automaton):
    """(return code, stats dict) of acm_sieve_selftest"""
    st = (C.c_uint32 * len(STATS))()
    rc = lib.acm_sieve_selftest(automaton.h, st)
    return rc, dict(zip(STATS, list(st)))


# ---------------------------------------------------------------- searches

def grams_in_bucket(bucket, log_buckets, count, rng, alphabet=None, exclude=()):
    """`count` distinct 3-grams whose home is `bucket`, drawn over `alphabet` (bytes; default all)"""
    sym = np.arange(256, dtype=np.uint64) if alphabet is None else np.frombuffer(bytes(alphabet), dtype=np.uint8).astype(np.uint64)
    out, seen = [], set(exclude)
    for _ in range(64):
        b = sym[rng.integers(0, sym.size, size=(1 << 16, 3))]
        g = b[:, 0] | (b[:, 1] << np.uint64(8)) | (b[:, 2] << np.uint64(16))
        for v in g[gram_buckets_np(g, log_buckets) == bucket].tolist():
            if v not in seen:
                seen.add(v)
                out.append(int(v))
                if len(out) == count:
                    return out
    raise AssertionError("found %d of %d grams for bucket %d of 2^%d" % (len(out), count, bucket, log_buckets))


def gram_bytes(g):
    return bytes([g & 0xFF, (g >> 8) & 0xFF, (g >> 16) & 0xFF])


def keys_in_slot(slot, log_slots, length, count, rng, alphabet, head=b"", exclude=()):
    """`count` distinct keys of `length` bytes over `alphabet` that begin with `head` and hash to `slot`"""
    sym = bytes(alphabet)
    out, seen = [], set(exclude)
    for _ in range(400000):
        k = head + bytes(sym[i] for i in rng.integers(0, len(sym), size=length - len(head)))
        if k not in seen and sieve_prefix_slot(*key_words(k), log_slots) == slot:
            seen.add(k)
            out.append(k)
            if len(out) == count:
                return out
    raise AssertionError("found %d of %d keys for slot %d of 2^%d" % (len(out), count, slot, log_slots))


class Case:
    """A constructed set, its texts, and what it promises (checked on the host against the library's stats)."""

    def __init__(self, name, patterns, texts, nocase=False, promise=None, notes=None):
        self.name, self.patterns, self.texts, self.nocase = name, patterns, texts, nocase
        self.promise = promise or {}       # stat name -> (lowest, highest or None)
        self.notes = notes or {}
        self.expect = {}                   # text index -> what the text promises (test_host_sieve_tables.py: check_expect)
        self.primed = ()                   # text indices that are ALSO scanned behind a priming batch

    def compiled(self):
        import orc
        from gpu_pattern_matching_amd import Automaton
        a, o = Automaton(nocase=self.nocase), orc.Oracle()
        for i, p in enumerate(self.patterns):
            a.add(p, i + 1)
            o.add(variants.fold(p) if self.nocase else p, i + 1)
        a.compile()
        o.compile()
        return a, o

    def oracle_text(self, t):
        return variants.fold(t) if self.nocase else t

    def model(self):
        if getattr(self, "_model", None) is None:
            self._model = Model(self.patterns, self.nocase)
        return self._model

    def quiet_text(self, n):
        """n bytes without a flagged sample: scanned first, it leaves the next launch without helper waves"""
        return self.model().filler_text(n, 1)

    def priming_text(self, n):
        """n bytes with a flagged sample per 128 bytes (more than one per 512): scanned first, it gives the next
        launch helper waves and sub-rows"""
        m = self.model()
        t = m.filler_text(n, 1)
        for i, at in enumerate(range(0, n - 64, 128)):
            plant(t, at, m.patterns[i % len(m.patterns)][:m.D])
        return t


def plant(text, at, piece):
    p = np.frombuffer(bytes(piece), dtype=np.uint8)
    assert 0 <= at and at + p.size <= text.size
    text[at:at + p.size] = p
    return at + p.size


def lay_out(model, pieces, n, gap=64, seed=0, start=None):
    """filler text of n bytes with the pieces planted `gap` bytes apart, each at a multiple of 8 plus its index mod 8
    (so that every alignment against the sample grid occurs), from `start` on (default: so that they straddle the
    first block border at 8 KiB)"""
    t = model.filler_text(n, seed)
    total = sum(len(p) + gap + 8 for p in pieces)
    assert total + 64 <= n, "text too small for its pieces: %d > %d" % (total, n)
    at = max(16, min(8192 - total // 2, n - total - 16)) if start is None else start
    for i, p in enumerate(pieces):
        at = (at + 7) // 8 * 8 + i % 8
        at = plant(t, at, p) + gap
    return t


# ---------------------------------------------------------------- the families

def gram_chain_case(shortest, seed=1):
    """Gram buckets: at least nine 3-grams with the LAST bucket as their home, so the chain runs through the last
    bucket, bucket 0 and bucket 1: lookups that end at probe 1, 2 and 3 and after the wrap.  Patterns beginning
    00 00 00 and FF FF FF (gram values 0 and 0xFFFFFF).  Text: every pattern, and absent 3-grams at sample
    positions that pass the filter and whose home is a bucket of the chain."""
    rng = np.random.default_rng(1000 * shortest + seed)
    W = sieve_stride(shortest)
    lb = 10
    last = (1 << lb) - 1
    npat = 900 // W
    chain = grams_in_bucket(last, lb, 12, rng)
    pats = []
    for i, g in enumerate(chain):   # the chained gram at offset i mod W, so every mask bit is looked at
        o = i % W
        body = bytearray(rng.integers(0, 256, size=shortest + int(rng.integers(0, 6)), dtype=np.uint8).tobytes())
        body[o:o + 3] = gram_bytes(g)
        pats.append(bytes(body))
    pats.append(bytes(shortest))
    pats.append(b"\xff" * shortest)
    while len(pats) < npat:
        pats.append(rng.integers(0, 256, size=shortest + int(rng.integers(0, 6)), dtype=np.uint8).tobytes())
    m = Model(pats)
    assert m.gram_log_buckets == lb, (m.gram_log_buckets, len(m.grams))
    assert m.LG == 3, "the absent grams below are searched as 3-byte filter keys"
    assert m.bucket_load[last] == 4 and m.bucket_load[0] == 4, "no chain through the last bucket"
    full = [b for b in (last, 0, 1, 2) if m.bucket_load[b] == 4]
    # absent grams the filter lets through, with their home in the chain
    absent = []
    cand = np.arange(1 << 24, dtype=np.uint64)
    for g in cand[np.isin(gram_buckets_np(cand, lb), full)].tolist():
        if g not in m.grams and m.bloom_passes(g):
            absent.append(int(g))
            if len(absent) == 12:
                break
    assert len(absent) >= 4, "only %d absent grams pass the filter" % len(absent)
    x, y = m.filler(seed)
    pieces = list(pats[:14]) + [pats[int(i)] for i in rng.integers(14, len(pats), size=10)]
    n = 64 * 1024
    t = lay_out(m, pieces, n, gap=40, seed=seed)
    at = 40 * 1024
    for g in absent:   # at a sample position, filler behind it
        plant(t, at, gram_bytes(g))
        at += 64
    flagged = set(m.flagged_positions(t[40 * 1024:at]).tolist())
    assert all(64 * i in flagged for i in range(len(absent))), "an absent gram is not flagged"
    return Case("gram_chain_s%d" % shortest, pats, [t],
                promise=dict(W=(W, W), gram_probes=(3, None), full_buckets=(2, None), gram_log_buckets=(lb, lb)),
                notes=dict(absent=len(absent)))


def prefix_chain_case(shortest, nocase=False, seed=1):
    """Prefix slots: keys that share their home slot, one chain through the LAST slot (wrap to slot 0) and one
    elsewhere, three keys or more each, so lookups end at probe 1, 2, 3.  Text: every chained key's pattern; absent
    keys that share a real pattern's first 3 bytes and hash to the head of a chain; for D = 10 keys that differ
    from a stored one in byte 8 or byte 9 only; for D < 10 a stored key followed by several different bytes."""
    rng = np.random.default_rng(2000 * shortest + seed + (7 if nocase else 0))
    D = min(shortest, MAX_PREFIX)
    sym = b"ABCDEFGH" if nocase else b"abcdefgh"
    wide = sym if D > 4 else bytes(range(1, 256))   # (8^3 keys are too few for 512 slots: all bytes then)
    npre = 40
    ls = 9                         # 33..64 prefixes: 512 slots
    last = (1 << ls) - 1
    other = 200
    keys = keys_in_slot(last, ls, D, 4, rng, wide)
    keys2 = keys_in_slot(other, ls, D, 3, rng, wide, exclude=keys)
    chained = keys + keys2

    def tail(extra):
        return bytes(sym[i] for i in rng.integers(0, len(sym), size=shortest - D + extra))

    pats = [k + tail(0 if i == 0 else int(rng.integers(0, 5))) for i, k in enumerate(chained)]
    while len({q[:D] for q in pats}) < npre:
        k = bytes(wide[i] for i in rng.integers(0, len(wide), size=D))
        pats.append(k + tail(int(rng.integers(0, 5))))
    assert min(len(q) for q in pats) == shortest
    m = Model(pats, nocase)
    assert m.prefix_log_slots == ls, (m.prefix_log_slots, len(m.prefixes))
    assert m.slot_load[last] and m.slot_load[0] and m.slot_load[1], "no chain through the last slot"
    # absent keys: a real pattern's first three bytes, the home of a chain
    absent = []
    if D > 3:   # (with D = 3 the 3-gram is the whole key: an absent key is an absent gram, gram_chain_case's business)
        for head, slot in ((chained[0][:3], last), (chained[4][:3], other), (chained[1][:3], last)):
            absent += keys_in_slot(slot, ls, D, 1, rng, bytes(range(1, 256)), head=head, exclude=set(m.prefixes) | set(absent))
    pieces = [p for p in pats[:len(chained)]] + [k + bytes([m.filler(seed)[0]]) * 3 for k in absent]
    if D == 10:                    # a stored key with byte 8 or byte 9 changed
        for k in chained[:3]:
            for at in (8, 9):
                other_byte = next(b for b in wide if b != k[at] and (k[:at] + bytes([b]) + k[at + 1:]) not in m.prefixes)
                pieces.append(k[:at] + bytes([other_byte]) + k[at + 1:] + b"abcd")
    else:                          # bytes behind a stored key do not matter to its lookup
        for k in chained[:3]:
            for b in (0x00, 0xFF, sym[0], sym[3], 0x80):
                pieces.append(k + bytes([b]) * 2)
    n = 32 * 1024
    t = lay_out(m, pieces, n, gap=24, seed=seed)
    if nocase:
        t = variants.scramble(t, seed)
        pats = [bytes(variants.scramble(np.frombuffer(p, dtype=np.uint8), seed + i)) for i, p in enumerate(pats)]
    return Case("prefix_chain_s%d%s" % (shortest, "_nocase" if nocase else ""), pats, [t], nocase=nocase,
                promise=dict(D=(D, D), prefix_probes=(3, None), prefix_log_slots=(ls, ls)))


def fanout_case(k, seed=1):
    """One node at depth 6 (D = 5) with k children: finals of prefix + byte, a longer pattern under every third child.
    Text: prefix + c for every child byte, one byte below the smallest child, one above the largest and one in every
    gap between children."""
    rng = np.random.default_rng(3000 + k + seed)
    prefix = b"node:="          # six bytes: the node lies behind depth D = 5 (the shortest pattern's length)
    if k >= 255:
        children = list(range(256))[:k] if k == 256 else list(range(1, 256))
    else:
        step = 254 // k
        children = sorted({3 + i * step + (i % 2) for i in range(k)})
    assert len(children) == k
    pats = []
    for i, c in enumerate(children):
        pats.append(prefix + bytes([c]))
        if i % 3 == 0:
            pats.append(prefix + bytes([c]) + b"tail" + bytes([65 + i % 26]))
    pats.append(b"short")
    m = Model(pats)
    probes = set(children)
    probes |= {children[0] - 1, children[-1] + 1} & set(range(256))
    for lo, hi in zip(children, children[1:]):
        if hi - lo > 1:
            probes.add(lo + 1 + (hi - lo - 2) // 2)
    pieces = []
    for c in sorted(probes):
        pieces.append(prefix + bytes([c]))
        if c in children and children.index(c) % 3 == 0:
            pieces.append(prefix + bytes([c]) + b"tail" + bytes([65 + children.index(c) % 26]))
            pieces.append(prefix + bytes([c]) + b"taim")
    n = 32 * 1024 if k < 255 else 64 * 1024
    t = lay_out(m, pieces, n, gap=16, seed=seed)
    return Case("fanout_%d" % k, pats, [t], promise=dict(D=(5, 5), max_fanout=(k, k)))


def run_path(n, x_d):
    """which compare a run level that starts behind text byte x_d takes (sparse.hip, follow): 64 bytes at once where
    the padded text has them ("roomy"), else byte by byte.  The code has a third branch between the two, x + 65 <=
    n_pad; with levels of 64 bytes that is the roomy condition itself, so no text reaches it."""
    n_pad = (n + 15) & ~15
    return "roomy" if x_d + 1 + 64 <= n_pad else "bytewise"


RUN_CUTS = (0, 1, 15, 16, 17, 63, 64, 65, 80)


def run_case(run, nocase=False, seed=1):
    """A pattern whose unary run behind depth D = 10 is `run` bytes long (a second pattern branches off at its
    end, so the run is exactly that).  Texts: one with a full match and with a mismatch at run byte 1, 63, 64, 65 and
    the last; and one per cut that ends 0, 1, 15, ... 80 bytes after the pattern's depth-D byte."""
    rng = np.random.default_rng(4000 + run + seed)
    sym = np.frombuffer(b"ABCDEFGH" if nocase else b"abcdefgh", dtype=np.uint8)
    body = sym[rng.integers(0, sym.size, size=10 + run + 1)].tobytes()
    other_last = bytes([b for b in sym.tobytes() if b != body[-1]][:1])
    # (no third pattern: the states of a path have consecutive ids, which is what makes a run, only while no other
    # path's states of the same depth are numbered between them)
    pats = [body, body[:-1] + other_last + (b"Z" if nocase else b"z")]
    m = Model(pats, nocase)
    pieces = [body]
    for at in sorted({1, 63, 64, 65, run}):
        if at <= run:
            wrong = bytearray(body)
            wrong[10 + at - 1] = 0x7E        # run byte `at` (1-based) is wrong
            pieces.append(bytes(wrong))
    texts = [lay_out(m, pieces, 16 * 1024, gap=32, seed=seed, start=8192 - 300)]
    paths = {}
    for cut in RUN_CUTS:
        n = 8192 + 3 + 10 + cut                # the pattern starts at 8195: its depth-D byte is byte n - cut - 1
        t = m.filler_text(n, seed)
        plant(t, 8195, body[:10 + cut])
        plant(t, 4096 + 5, body)               # and a whole one in the roomy middle
        texts.append(t)
        paths[cut] = run_path(n, n - cut - 1)
    if nocase:
        texts = [variants.scramble(t, seed + i) for i, t in enumerate(texts)]
        pats = [bytes(variants.scramble(np.frombuffer(p, dtype=np.uint8), seed + i)) for i, p in enumerate(pats)]
    return Case("run_%d%s" % (run, "_nocase" if nocase else ""), pats, texts, nocase=nocase,
                promise=dict(D=(10, 10), longest_run=(run, run)), notes=dict(paths=paths))


def hits_case(k, seed=1):
    """One trie path with exactly k final nodes (nested patterns p[:j]) behind depth D = 4.  Scanned alone, behind a
    longer overlapping follower that shadows some of its hits, behind one that shadows all of them, and with small-
    and big-hit followers at adjacent sample positions."""
    p = b"qrst" + b"uvwxyzUVWXYZ0123456789-+"[:2 * k]
    nested = [p[:4 + 2 * j] for j in range(1, k + 1)]         # k finals, at depths 6, 8, ...
    assert len(nested) == k
    # a longer path that overlaps p: it starts earlier and runs over part, or all, of p
    some = b"LONG-lead-" + p[:4 + k]                           # ends inside p: shadows the hits up to there
    whole = b"WHOLE-lead" + p + b"##"                          # runs past p: shadows every hit
    small = [b"qrsu", b"rstuvA"]                               # one hit each, starting next to p's start
    pats = nested + [some, whole] + small
    m = Model(pats)
    pieces = [p, some + p[4 + k:], whole, b"q" + p, p[:5] + p, small[0] + p, b"qrs" + small[1], p + p]
    t = lay_out(m, pieces, 16 * 1024, gap=24, seed=seed)
    return Case("hits_%d" % k, pats, [t], promise=dict(D=(4, 4)), notes=dict(finals=k))


# ---------------------------------------------------------------- what a text makes the check kernel do

BLOCK = 8 * TILE          # a row of the check kernel launched alone; twice that in a launch group of four or more


def followers(model, text):
    """The followers of a text, derived from the pattern list alone (plain Python over the trie as a set of
    prefixes): [(start, sample position, extent + 1, [positions of the final nodes on its path])] in start order.
    A follower is a start s whose D bytes are a trie path; its sample is the one position = 0 mod W in [s, s + W);
    a node is final when a pattern ends there (its own path's, or a suffix's: acsmx.c:417-429).  With 6-byte filter
    keys a path that leaves the trie inside its sample's key is never flagged and has no follower (it is shorter than
    the shortest pattern): those starts are left out."""
    t = variants.fold(np.asarray(text, dtype=np.uint8)) if model.nocase else np.asarray(text, dtype=np.uint8)
    tb, n, D, W = t.tobytes(), t.size, model.D, model.W
    pats = set(model.patterns)
    lens = sorted({len(p) for p in pats})
    prefixes = {p[:j] for p in pats for j in range(D, len(p) + 1)}
    heads = set(model.prefixes)
    seen = set(model.flagged_positions(text).tolist()) if model.LG == 6 else None
    out = []
    for s in range(0, n - D + 1):
        if tb[s:s + D] not in heads or (seen is not None and -(-s // W) * W not in seen):
            continue
        j, hits = D, []
        while True:
            path = tb[s:s + j]
            if any(j >= L and path[j - L:] in pats for L in lens):
                hits.append(s + j - 1)
            if s + j < n and tb[s:s + j + 1] in prefixes:
                j += 1
            else:
                break
        out.append((s, -(-s // W) * W, s + j, hits))
    return out


def surviving(fols):
    """per follower the hits the shadow leaves it: those at or behind the largest extent + 1 of the followers with
    a smaller start (sparse.hip, step 4)"""
    kept, reach = [], 0
    for s, p, ext1, hits in fols:
        kept.append([e for e in hits if e >= reach])
        reach = max(reach, ext1)
    return kept


def counts(model, text):
    """flagged samples per tile (the model's filter), followers and surviving hits per tile of their sample"""
    ntiles = (len(text) + TILE - 1) // TILE
    flagged = np.bincount(model.flagged_positions(text) // TILE, minlength=ntiles)
    fols = followers(model, text)
    kept = surviving(fols)
    fol = np.bincount(np.array([f[1] // TILE for f in fols], dtype=np.int64), minlength=ntiles)
    hit = np.bincount(np.array([f[1] // TILE for f in fols], dtype=np.int64), weights=[len(k) for k in kept],
                      minlength=ntiles).astype(np.int64)
    return flagged, fol, hit, fols, kept


# ---------------------------------------------------------------- the seams

SEAM_N = 40 * TILE
SEAM_AT = 2 * BLOCK       # the block the counts are put in: row 2 of 8 tiles, and the first half of row 1 of 16 tiles
                          # (whose second half stays quiet, so the row holds the same counts either way)


def seam_patterns(seed=5):
    """shortest 10 (W = 8, D = 10, 3-byte filter keys): 24 patterns of exactly 10 bytes, 24 longer ones, and the two
    of period 2 that make every position of "abab..." a follower"""
    rng = np.random.default_rng(seed)
    sym = np.frombuffer(b"abcdefghijklmnop", dtype=np.uint8)
    pats = [sym[rng.integers(0, sym.size, size=10)].tobytes() for _ in range(24)]
    pats += [sym[rng.integers(0, sym.size, size=int(rng.integers(14, 25)))].tobytes() for _ in range(24)]
    pats += [b"ab" * 5, b"ba" * 5]
    assert len({p[:10] for p in pats}) == len(pats)
    return pats


def seam_text(m, items, spacing, first=0):
    """SEAM_N bytes of quiet filler, two whole patterns in the first block and one at the very end, and the items
    `spacing` bytes apart (a multiple of 8: each at a sample position) from SEAM_AT + first on"""
    assert spacing % 8 == 0 and first % 8 == 0 and first + len(items) * spacing <= BLOCK - 64
    t = m.filler_text(SEAM_N, 1)
    plant(t, 1000, m.patterns[0])
    plant(t, 5003, m.patterns[30])
    plant(t, SEAM_N - len(m.patterns[31]), m.patterns[31])
    for i, it in enumerate(items):
        plant(t, SEAM_AT + first + i * spacing, it)
    return t


def seam_items(m, k, kinds):
    """k items, kinds in turn: "hit" a whole 10-byte pattern, "path" the first 10 bytes of a longer one (a follower
    that ends without a hit), "gram" the first 3 bytes of one (flagged, turned down by the prefix lookup)"""
    out = []
    for i in range(k):
        kind = kinds[i % len(kinds)]
        out.append(m.patterns[i % 24] if kind == "hit" else m.patterns[24 + i % 24][:10] if kind == "path"
                   else m.patterns[(5 * i) % 48][:3])
    return out


def seam_case(which):
    pats = seam_patterns()
    m = Model(pats)
    assert (m.W, m.D, m.LG) == (8, 10, 3)
    c = None
    if which == "tile":          # kSampleHead = 32 samples of a tile in the dense head
        ks = (30, 31, 32, 33, 34, 35)
        texts = [seam_text(m, seam_items(m, k, ("hit", "path", "gram")), 16, first=TILE) for k in ks]
        c = Case("seam_tile", pats, texts)
        c.expect = {i: dict(tile_flagged=(SEAM_AT // TILE + 1, k)) for i, k in enumerate(ks)}
    elif which == "hits":        # kHitHead = 8 hits of a row in the dense head
        ks = (6, 7, 8, 9, 10, 11)
        texts = [seam_text(m, seam_items(m, k, ("hit",)), 64, first=128) for k in ks]
        c = Case("seam_hits", pats, texts)
        c.expect = {i: dict(block_hits=k) for i, k in enumerate(ks)}
    elif which == "followers":   # 64 followers a stage-2 round
        ks = (62, 63, 64, 65, 66, 67, 126, 127, 128, 129, 130)
        texts = [seam_text(m, seam_items(m, k, ("path", "path", "hit")), 32, first=64) for k in ks]
        c = Case("seam_followers", pats, texts)
        c.expect = {i: dict(block_followers=k) for i, k in enumerate(ks)}
    elif which == "queue":       # kQ2Cap = 576 queued followers: a stage-1 round of 64 samples adds up to 64 x 8
        texts = []
        for first, length in ((5, 3000), (131, 2777), (8, 5120)):
            t = seam_text(m, [], 8)
            plant(t, SEAM_AT + first, (b"ab" * 4096)[:length])
            texts.append(t)
        c = Case("seam_queue", pats, texts)
        c.expect = {i: dict(block_followers_over=576, followers_per_sample=8) for i in range(len(texts))}
    elif which == "block":       # kSubRow = 256 samples of a block before it is cut into sub-rows
        ks = (254, 255, 256, 257, 258, 259)
        texts = [seam_text(m, seam_items(m, k, ("gram", "path", "hit", "gram")), 24, first=0) for k in ks]
        c = Case("seam_block", pats, texts)
        c.expect = {i: dict(block_flagged=k) for i, k in enumerate(ks)}
        c.primed = tuple(range(len(ks)))
    c._model = m
    return c


SEAMS = ("tile", "hits", "followers", "queue", "block")

GRAM_SHORTEST = (3, 4, 6, 10)
PREFIX_SHORTEST = (3, 5, 8, 9, 10, 13)
FANOUTS = (2, 3, 4, 5, 8, 9, 16, 255, 256)
RUNS = (63, 64, 65, 127, 128, 129, 200)
HITS = (3, 4, 5, 6, 12)

BUILDERS = {}
for _s in GRAM_SHORTEST:
    BUILDERS["gram_chain_s%d" % _s] = (gram_chain_case, (_s,))
for _s in PREFIX_SHORTEST:
    BUILDERS["prefix_chain_s%d" % _s] = (prefix_chain_case, (_s,))
BUILDERS["prefix_chain_s8_nocase"] = (prefix_chain_case, (8, True))
for _k in FANOUTS:
    BUILDERS["fanout_%d" % _k] = (fanout_case, (_k,))
for _r in RUNS:
    BUILDERS["run_%d" % _r] = (run_case, (_r,))
BUILDERS["run_129_nocase"] = (run_case, (129, True))
for _k in HITS:
    BUILDERS["hits_%d" % _k] = (hits_case, (_k,))

for _w in SEAMS:
    BUILDERS["seam_%s" % _w] = (seam_case, (_w,))

_cache = {}


def case(name):
    """the named case, built once per process"""
    if name not in _cache:
        fn, args = BUILDERS[name]
        _cache[name] = fn(*args)
    return _cache[name]
