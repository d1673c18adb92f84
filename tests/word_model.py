"""Whole-word matching in Python (test infrastructure only): the rule of acm_word_matches_async on top of
the oracle's all-patterns scan, and a brute-force restatement to check it against.

A word byte is a byte of W (default [0-9A-Za-z_]).  Pattern P of length L >= 1 ending at offset o is
word-bounded when the byte at o - L is not in W or o - L + 1 is a text start, and the byte at o + 1 is
not in W or o + 1 is a text end.  Text starts: the first byte of the stream (in front of `before`)
and every segment start; text ends: the end of the stream when next_byte is -1, and every segment
start.
"""
import numpy as np

import fixtures
import orc

DEFAULT = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")
EMPTY = frozenset()
FULL = frozenset(range(256))
CUSTOM = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz'")   # letters and the apostrophe

FOLD = np.arange(256, dtype=np.uint8)
FOLD[ord("a"):ord("z") + 1] -= 0x20


def fold(b):
    return bytes(FOLD[np.frombuffer(bytes(b), dtype=np.uint8)]) if b else b""


class WordModel:
    """The oracle of a fixture set (of its folded patterns when nocase) and the pattern lengths."""

    def __init__(self, name, nocase=False):
        base = fixtures.oracle_for(name)
        self.pats = [p for p, _ in base.patterns()]
        if nocase:
            o = orc.Oracle()
            for p, iid in base.patterns():
                o.add(fold(p), iid)
            self.o = o.compile()
        else:
            self.o = base
        self.nocase = nocase
        self.lengths = np.array([len(p) for p in self.pats], dtype=np.int64)
        self.max_len = int(self.lengths.max()) if self.lengths.size else 0

    def scan_all(self, text, init_state=0, starts=None):
        """(offsets, patterns, final state) in list order; with starts every segment from state 0"""
        t = np.ascontiguousarray(text, dtype=np.uint8)
        if self.nocase:
            t = FOLD[t]
        if starts is None or len(starts) == 0:
            return self.o.scan_all(t, init_state)
        bounds = [0] + [int(min(max(s, 0), t.size)) for s in starts] + [t.size]
        offs, pats, state = [], [], init_state
        for k in range(-1, len(starts)):
            lo, hi = bounds[k + 1], max(bounds[k + 2], bounds[k + 1])
            if k >= 0:
                state = 0
            p, q, state = self.o.scan_all(t[lo:hi], state)
            offs.append(p.astype(np.int64) + lo)
            pats.append(q)
        return np.concatenate(offs).astype(np.uint32), np.concatenate(pats).astype(np.int32), state

    def words(self, text, word_set=DEFAULT, all_patterns=False, init_state=0, before=b"", next_byte=-1,
              starts=None):
        """(offsets, patterns, final state) of the word pass: head form (first bounded pattern per offset)
        or all form (every bounded pattern, list order)"""
        t = np.ascontiguousarray(text, dtype=np.uint8)
        offs, pats, last = self.scan_all(t, init_state, starts)
        ok = bounded_mask(t, offs, self.lengths[pats] if pats.size else np.zeros(0, np.int64), word_set, before,
                          next_byte, starts)
        if all_patterns:
            return offs[ok], pats[ok], last
        o_out, p_out, prev = [], [], None
        for o, p, k in zip(offs.tolist(), pats.tolist(), ok.tolist()):
            if k and o != prev:
                o_out.append(o)
                p_out.append(p)
                prev = o
        return np.array(o_out, dtype=np.uint32), np.array(p_out, dtype=np.int32), last


def bounded_mask(text, offs, lens, word_set, before=b"", next_byte=-1, starts=None):
    """bool per (offset, length): the entry is word-bounded"""
    t = bytes(np.ascontiguousarray(text, dtype=np.uint8))
    n, nb = len(t), len(before)
    st = set(int(s) for s in starts) if starts is not None else set()

    def byte(p):
        if 0 <= p < n:
            return t[p]
        if p == n:
            return next_byte
        if -nb <= p < 0:
            return before[nb + p]
        return -1

    out = np.zeros(len(offs), dtype=bool)
    for i, (o, L) in enumerate(zip(np.asarray(offs).tolist(), np.asarray(lens).tolist())):
        if L <= 0:
            continue
        a = o - L + 1
        left = a in st or byte(a - 1) not in word_set
        right = (o + 1) in st or byte(o + 1) not in word_set
        out[i] = left and right
    return out


def brute_force(pats, text, word_set=DEFAULT, nocase=False):
    """every word-bounded (end offset, pattern index) pair, found with bytes.find for every pattern"""
    t = bytes(np.ascontiguousarray(text, dtype=np.uint8))
    hay = fold(t) if nocase else t
    out = set()
    for i, p in enumerate(pats):
        if not p:
            continue
        needle = fold(p) if nocase else p
        k = hay.find(needle)
        while k >= 0:
            o = k + len(p) - 1
            if (k == 0 or t[k - 1] not in word_set) and (o + 1 == len(t) or t[o + 1] not in word_set):
                out.add((o, i))
            k = hay.find(needle, k + 1)
    return out


def planted_text(pats, n, seed, max_len=None):
    """n bytes: patterns planted next to letters, digits, '_', punctuation, spaces, bytes >= 0x80, at the
    start and at the end"""
    rng = np.random.default_rng(seed)
    neighbours = [b"a", b"Z", b"7", b"_", b".", b",", b" ", b"\n", b"\x80", b"\xe9", b"'", b"-", b""]
    short = [p for p in pats if p and (max_len is None or len(p) <= max_len)] or [p for p in pats if p]
    out = bytearray(short[int(rng.integers(len(short)))])
    while len(out) < n:
        p = short[int(rng.integers(len(short)))]
        out += neighbours[int(rng.integers(len(neighbours)))] + p + neighbours[int(rng.integers(len(neighbours)))]
        if rng.random() < 0.3:
            out += bytes(rng.integers(32, 127, size=int(rng.integers(1, 6)), dtype=np.uint8))
    out = out[:n] + short[int(rng.integers(len(short)))]   # (about n bytes; one pattern at the very end)
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def mask32(word_set):
    """the 32-byte bit mask acm_word_matches_async takes"""
    m = np.zeros(256, dtype=np.uint8)
    if word_set:
        m[np.array(sorted(word_set), dtype=np.int64)] = 1
    return np.packbits(m, bitorder="little").tobytes()
