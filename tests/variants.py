"""Seeded pattern sets and texts for the regimes that pick the scan kernels' template instantiations
(a test helper, not a conftest).

The host chooses a kernel per launch from properties of the set -- shortest pattern (the sieve's
stride W, its key length LG), longest pattern (halo or speculative walk, preload, wide pre), byte-class
count (class-compressed planes or the identity), state count (LDS-resident or not) -- and of the text.
Every generator here returns what it promises about those properties, and test_host_variants.py checks
the promises on the host, so a regime that drifts is caught without a GPU.
"""
import numpy as np

FOLD = np.arange(256, dtype=np.uint8)
FOLD[ord("a"):ord("z") + 1] -= 0x20

MIXED = (bytes(range(ord("A"), ord("Z") + 1)) + bytes(range(ord("a"), ord("z") + 1)) + b"@[`{"
         + bytes([0x80, 0xC1, 0xE1, 0xFF]))   # letters, the bytes next to the letter ranges, bytes >= 0x80


def fold(b):
    """C-locale toupper (what a nocase automaton does to its patterns and its text)"""
    if isinstance(b, np.ndarray):
        return FOLD[b]
    return bytes(FOLD[np.frombuffer(b, dtype=np.uint8)]) if b else b""


def sieve_stride(shortest):
    """W of the sparse pipeline's sample grid (sieve_tables.h: sieve_stride)"""
    return 8 if shortest >= 10 else 4 if shortest >= 6 else 2 if shortest >= 4 else 1


def sieve_key_len(shortest):
    """LG: 6-byte filter keys where every pattern has W + 5 bytes and W >= 4, else 3 (device_dfa.hip)"""
    w = sieve_stride(shortest)
    return 6 if w >= 4 and w + 5 <= shortest else 3


def log_stride(classes):
    """columns per state row of the chain pipeline's planes: 2^log_stride (automaton.cpp: byte_classes)"""
    if classes > 128:
        return 8
    ls = 1
    while (1 << ls) < classes:
        ls += 1
    return ls


def hot_max(classes):
    """rows the chain walk's LDS holds for this class count (automaton.cpp: number_for_device)"""
    return min((256 * 512) // (2 << log_stride(classes)), 0x8000)


class VariantSet:
    """A pattern set and what it promises: shortest/longest length, byte classes (256: identity),
    a state-count range, LDS residency, and the bytes its texts are drawn from."""

    def __init__(self, patterns, nocase, alphabet, classes, states, lds, run_byte=None):
        self.patterns = patterns
        self.nocase = nocase
        self.alphabet = np.frombuffer(bytes(alphabet), dtype=np.uint8).copy()
        self.shortest = min(len(p) for p in patterns)
        self.longest = max(len(p) for p in patterns)
        self.classes = classes
        self.states = states
        self.lds = lds
        self.run_byte = run_byte
        used = set(alphabet)
        fold_used = set(FOLD[list(used)].tolist())
        self.outside = next((b for b in range(256) if b not in used and FOLD[b] not in fold_used), None)

    @property
    def stride(self):
        return sieve_stride(self.shortest)

    @property
    def key_len(self):
        return sieve_key_len(self.shortest)

    def compiled(self):
        """(Automaton, Oracle): the oracle of the folded patterns for a nocase set; ids are index + 1"""
        import orc
        from gpu_pattern_matching_amd import Automaton
        a, o = Automaton(nocase=self.nocase), orc.Oracle()
        for i, p in enumerate(self.patterns):
            a.add(p, i + 1)
            o.add(fold(p) if self.nocase else p, i + 1)
        a.compile()
        o.compile()
        return a, o

    def text_of(self, t):
        """what the oracle scans for text t"""
        return fold(t) if self.nocase else t


def _symbols(rng, alphabet, classes):
    if classes is not None:
        k = classes - 1
        perm = rng.permutation(254)[:max(k - 2, 0)] + 1
        out = ([0x00, 0xFF] + perm.tolist())[:k] if k >= 2 else [0x61]
        return bytes(sorted(out))
    if alphabet == "letters":
        return b"abcde"[:int(rng.integers(3, 6))]
    if alphabet == "binary":
        return bytes(range(256))
    if alphabet == "mixed":
        return MIXED
    raise KeyError(alphabet)


def pattern_set(seed, shortest, longest, alphabet="letters", classes=None, count=24, nocase=False, big=False):
    """A seeded set with exactly this shortest and longest pattern.

    alphabet: "letters" (a few letters: prefixes, suffixes and whole patterns collide, duplicates kept),
    "binary" (all 256 bytes, 0x00 and 0xFF among them: the identity table), "mixed" (both cases, the
    bytes next to the letter ranges and bytes >= 0x80: for nocase).  classes: exactly classes - 1
    distinct bytes in the patterns (so that many byte classes; 129 and more: the identity).
    big: several thousand patterns, over 16384 states (not LDS-resident).
    """
    rng = np.random.default_rng(seed)
    sym = np.frombuffer(_symbols(rng, alphabet, classes), dtype=np.uint8)
    pats = []

    def rand(n):
        return bytes(sym[rng.integers(0, sym.size, size=n)])

    def length():
        r = rng.random()
        if r < 0.7:
            return int(rng.integers(shortest, min(longest, shortest + 8) + 1))
        return int(rng.integers(shortest, longest + 1))

    # every symbol in some pattern: a permutation of them cut into pattern-sized pieces
    perm = bytes(sym[rng.permutation(sym.size)])
    at = 0
    while at < len(perm):
        k = length()
        piece = perm[at:at + k]
        at += k
        pats.append(piece + rand(k - len(piece)))
    pats.append(rand(shortest))
    pats.append(rand(longest))
    run_byte = int(sym[0])
    pats.append(bytes([run_byte]) * min(longest, max(shortest, 12)))   # a run that can start a pattern (sv_run_ok)
    n_more = (6000 if big else count) - len(pats)
    for _ in range(max(n_more, 0)):
        k = length()
        r = rng.random()
        if r < 0.4:                      # an earlier pattern's prefix or suffix, extended
            base = pats[int(rng.integers(len(pats)))]
            cut = int(rng.integers(1, len(base) + 1))
            body = (base[:cut] + rand(k)) if rng.random() < 0.5 else (rand(k) + base[-cut:])
            pats.append(body[:k] if rng.random() < 0.5 else body[-k:])
        elif r < 0.45:                   # a duplicate
            pats.append(pats[int(rng.integers(len(pats)))])
        else:
            pats.append(rand(k))
    pats = [p for p in pats if shortest <= len(p) <= longest]
    used = set(b"".join(pats))
    if nocase:
        used = set(FOLD[list(used)].tolist())
    ncls = len(used) + (1 if len(used) < 256 else 0)
    ncls = 256 if ncls > 128 else ncls
    lds = longest <= 33 and not big and ncls <= 120
    states = (16385, 1 << 30) if big else (longest + 1, 1 + sum(len(p) for p in pats))
    if nocase:   # the patterns in mixed case: the automaton folds them
        pats = [bytes(scramble(np.frombuffer(p, dtype=np.uint8), seed + i)) for i, p in enumerate(pats)]
    return VariantSet(pats, nocase, bytes(sym), ncls, states, lds, run_byte)


def scramble(t, seed):
    """t with the case of its ASCII letters flipped at random"""
    t = np.array(t, dtype=np.uint8, copy=True)
    letter = ((t | 0x20) >= ord("a")) & ((t | 0x20) <= ord("z"))
    t[letter & (np.random.default_rng(seed).random(t.size) < 0.5)] ^= 0x20
    return t


BORDERS = (16, 64, 256, 1024, 4096, 16384, 65536)   # chain, tile and 4 KiB borders


def text(vs, n, seed, kind="planted"):
    """uint8[n] for a VariantSet.

    random:  over the set's bytes plus one byte outside them;
    planted: that, with patterns planted, a third across chain/tile/4 KiB borders, one at the text end;
    runs:    planted, with long runs of the set's run byte (mixed-case runs for nocase);
    dense:   patterns and pattern prefixes back to back: nearly every sample is a candidate.
    """
    rng = np.random.default_rng(seed)
    pool = vs.alphabet if vs.outside is None else np.concatenate([vs.alphabet, np.array([vs.outside], dtype=np.uint8)])
    t = pool[rng.integers(0, pool.size, size=n)]
    if kind == "dense":
        short = [p for p in vs.patterns if len(p) <= 2 * vs.shortest + 8] or vs.patterns
        parts, size = [], 0
        while size < n:
            p = short[int(rng.integers(len(short)))]
            if rng.random() < 0.3:
                p = p[:int(rng.integers(3, len(p) + 1))]
            parts.append(p)
            size += len(p)
        t = np.frombuffer(b"".join(parts)[:n], dtype=np.uint8).copy()
    elif kind in ("planted", "runs"):
        plants = max(8, n // 96)
        for k in range(plants):
            p = np.frombuffer(vs.patterns[int(rng.integers(len(vs.patterns)))], dtype=np.uint8)
            if p.size >= n:
                continue
            at = int(rng.integers(0, n - p.size + 1))
            if k % 3 == 0:
                b = BORDERS[(k // 3) % len(BORDERS)]
                if n > b + p.size:
                    at = max(0, min(n - p.size, (at // b) * b + b - int(rng.integers(1, p.size + 1))))
            t[at:at + p.size] = p
        p = np.frombuffer(vs.patterns[int(rng.integers(len(vs.patterns)))], dtype=np.uint8)
        if p.size <= n:
            t[n - p.size:] = p   # a match that ends with the text
        if kind == "runs":
            for _ in range(max(2, n // 8192)):
                k = int(rng.integers(64, 2049))
                at = int(rng.integers(0, max(1, n - k)))
                t[at:at + k] = vs.run_byte
    if vs.nocase:
        t = scramble(t, seed)
    return t


# The regimes of test_gpu_variants.py's rows and of test_host_variants.py, by name: pattern_set arguments.
REGIMES = {
    # sparse pipeline: every (W, D, LG) of the sieve, case-sensitive and nocase
    "s3_letters": dict(seed=1, shortest=3, longest=12),
    "s3_binary_l192": dict(seed=2, shortest=3, longest=192, alphabet="binary"),
    "s3_mixed": dict(seed=3, shortest=3, longest=16, alphabet="mixed", nocase=True),
    "s4_c9": dict(seed=4, shortest=4, longest=20, classes=9),
    "s4_letters": dict(seed=5, shortest=4, longest=24),
    "s5_binary": dict(seed=6, shortest=5, longest=64, alphabet="binary"),
    "s4_mixed": dict(seed=7, shortest=4, longest=24, alphabet="mixed", nocase=True),
    "s5_mixed": dict(seed=8, shortest=5, longest=40, alphabet="mixed", nocase=True),
    "s6_c33": dict(seed=9, shortest=6, longest=96, classes=33),
    "s8_binary": dict(seed=10, shortest=8, longest=24, alphabet="binary"),
    "s9_letters": dict(seed=11, shortest=9, longest=40),
    "s6_mixed": dict(seed=12, shortest=6, longest=48, alphabet="mixed", nocase=True),
    "s9_mixed": dict(seed=13, shortest=9, longest=20, alphabet="mixed", nocase=True),
    "s8_mixed": dict(seed=14, shortest=8, longest=32, alphabet="mixed", nocase=True),
    "s10_letters": dict(seed=15, shortest=10, longest=16),
    "s13_binary_l300": dict(seed=16, shortest=13, longest=300, alphabet="binary"),
    "s16_letters": dict(seed=17, shortest=16, longest=64),
    "s12_mixed": dict(seed=18, shortest=12, longest=32, alphabet="mixed", nocase=True),
    "s10_mixed": dict(seed=19, shortest=10, longest=100, alphabet="mixed", nocase=True),
    "s13_mixed": dict(seed=20, shortest=13, longest=40, alphabet="mixed", nocase=True),
    "s12_c65": dict(seed=21, shortest=12, longest=30, classes=65),
    # chain pipeline: halo vs speculative, preload, wide pre, class-compressed vs identity planes
    "l16_letters": dict(seed=30, shortest=3, longest=16),
    "l16_binary": dict(seed=31, shortest=4, longest=16, alphabet="binary"),
    "l32_binary": dict(seed=32, shortest=4, longest=32, alphabet="binary"),
    "l40_c33": dict(seed=33, shortest=5, longest=40, classes=33),
    "l80_c17": dict(seed=34, shortest=4, longest=80, classes=17),
    "l150_letters": dict(seed=35, shortest=3, longest=150),
    "l64_binary": dict(seed=36, shortest=6, longest=64, alphabet="binary"),
    "l60_mixed": dict(seed=37, shortest=4, longest=60, alphabet="mixed", nocase=True),
    "l40_c65": dict(seed=38, shortest=4, longest=40, classes=65),
    "l150_c9": dict(seed=39, shortest=4, longest=150, classes=9),
    "l120_binary": dict(seed=40, shortest=5, longest=120, alphabet="binary"),
    "l300_c5": dict(seed=41, shortest=3, longest=300, classes=5),
    # LDS-resident (k_lds_walk: halo <= 16 B or longer), and too big for it
    "lds16_letters": dict(seed=50, shortest=3, longest=16),
    "lds12_mixed": dict(seed=51, shortest=3, longest=12, alphabet="mixed", nocase=True),
    "lds33_c33": dict(seed=52, shortest=4, longest=33, classes=33),
    "big_c17": dict(seed=53, shortest=10, longest=20, classes=17, big=True),
    # byte-class counts either side of every log_stride step (host checks only)
    "c2": dict(seed=60, shortest=4, longest=8, classes=2),
    "c3": dict(seed=61, shortest=4, longest=8, classes=3),
    "c4": dict(seed=62, shortest=4, longest=8, classes=4),
    "c5": dict(seed=63, shortest=4, longest=8, classes=5),
    "c8": dict(seed=64, shortest=4, longest=8, classes=8),
    "c16": dict(seed=65, shortest=4, longest=8, classes=16),
    "c17": dict(seed=66, shortest=4, longest=8, classes=17),
    "c32": dict(seed=67, shortest=4, longest=8, classes=32),
    "c64": dict(seed=68, shortest=4, longest=8, classes=64),
    "c128": dict(seed=69, shortest=4, longest=8, classes=128, count=200),
    "c129": dict(seed=70, shortest=4, longest=8, classes=129, count=200),
}


def regime(name):
    return pattern_set(**REGIMES[name])
