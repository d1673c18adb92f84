"""The model of the normalise pass (acm_normalize_async, include/acmatch.h): a serial walk over the units of every
text.  It knows nothing of the locality the kernels rest on (bytes i - 3 .. i + 2): it walks from the first unit of a
text to its last and remembers one thing, whether the unit in front was blank.

  normalize(...)  -> Norm: out (bytes), first[], last[] (per output byte, in the caller's coordinates), keep (bool per
                     input byte), keep_words (uint64), block (int32 cells), seg_out, info (list of 8)
  remap(...)      -> what acm_normalize_remap_async leaves for planes of offsets (and patterns)
"""
import numpy as np

PERCENT, SQUEEZE, STRIP = 1, 2, 4
BLOCK = 1024
DEFAULT_BLANKS = frozenset(b"\t\n\v\f\r ")
HEX = frozenset(b"0123456789abcdefABCDEF")


def blank_mask(blanks):
    """the 32-byte mask acm_normalize_async takes: bit b % 8 of byte b // 8"""
    m = bytearray(32)
    for b in blanks:
        m[b >> 3] |= 1 << (b & 7)
    return bytes(m)


class Norm:
    pass


def text_cuts(n, origin, seg_start):
    """the texts of a call as [a, b) pairs in call offsets: the starts clamped into the text, the bytes in front of
    the first start a text of their own, empty texts left out"""
    cuts = {0, n}
    for s in (seg_start if seg_start is not None else ()):
        cuts.add(min(max(int(s), origin), origin + n) - origin)
    cuts = sorted(cuts)
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def normalize(text, flags=0, blanks=None, blank_byte=0x20, origin=0, seg_start=None, out_capacity=None, with_out=True):
    t = bytes(text)
    n = len(t)
    assert not (flags & SQUEEZE and flags & STRIP) and not flags & ~7
    blanks = DEFAULT_BLANKS if blanks is None else frozenset(blanks)
    if not flags & (SQUEEZE | STRIP):
        blanks = frozenset()
    out, first, last = bytearray(), [], []
    keep = np.zeros(n, dtype=bool)
    dropped = triples = blank_emitted = 0
    for a, b in text_cuts(n, origin, seg_start):
        i = a
        prev_blank = False                     # (the first unit of a text has no unit in front)
        while i < b:
            if flags & PERCENT and t[i] == 0x25 and i + 2 < b and t[i + 1] in HEX and t[i + 2] in HEX:
                length, value = 3, int(t[i + 1:i + 3], 16)
                triples += 1
            else:
                length, value = 1, t[i]
            is_blank = value in blanks
            emit = True
            if is_blank:
                emit = bool(flags & SQUEEZE) and not prev_blank
                value = blank_byte
            if emit:
                out.append(value)
                first.append(origin + i)
                last.append(origin + i + length - 1)
                keep[i] = True
                blank_emitted += int(is_blank)
            else:
                dropped += 1
            prev_blank = is_blank
            i += length
    r = Norm()
    r.out, r.m = bytes(out), len(out)
    r.first, r.last = np.array(first, dtype=np.int64), np.array(last, dtype=np.int64)
    r.keep = keep
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = keep
    r.keep_words = np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8") if n else \
        np.zeros(0, dtype=np.uint64)
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)      # before[i]: emitted in front of byte i
    cells = (n + BLOCK - 1) // BLOCK + 1
    r.block = np.array([before[min(j * BLOCK, n)] for j in range(cells)], dtype=np.int32)
    r.block[-1] = r.m
    r.seg_out = None
    if seg_start is not None:
        r.seg_out = np.array([before[min(max(int(s), origin), origin + n) - origin] for s in seg_start], dtype=np.int32)
    cut = int(with_out and out_capacity is not None and r.m > out_capacity)
    r.info = [r.m, dropped, triples, blank_emitted, cut, 0, 0, 0]
    return r


def remap(norm, offs, pats=None, pat_len=None):
    """(off_out, start_out, bad): per record last(off), first(off - len + 1), -1 where unmapped; bad: records with an
    unmapped cell"""
    off_out, start_out, bad = [], [], 0
    for k, o in enumerate(offs):
        o = int(o)
        ok = 0 <= o < norm.m
        off_out.append(int(norm.last[o]) if ok else -1)
        if pats is not None:
            p = int(pats[k])
            s = o - pat_len[p] + 1 if 0 <= p < len(pat_len) and pat_len[p] >= 1 else -1
            good = 0 <= s < norm.m
            start_out.append(int(norm.first[s]) if good else -1)
            ok = ok and good
        bad += int(not ok)
    return (np.array(off_out, dtype=np.int64), np.array(start_out, dtype=np.int64) if pats is not None else None, bad)
