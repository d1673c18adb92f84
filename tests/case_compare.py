"""The byte compare of the case pass, swept (test infrastructure only, not a conftest): the patterns, the
hand-built planes and the expected records of tests/test_gpu_case_compare.py, and of the host test in
tests/test_host_case.py that pins them to case_model.CaseModel without a GPU.

The set is the suffixes of two master strings.  M (33 bytes, all distinct, mixed case): the exact suffixes
of every length 1..20, of 24 and of 33, and the suffix of length 2 once more, ignoring case.  M13 (13 bytes
over other letters): the exact suffixes of every length 1..13 and the one of length 2 ignoring case.  The
24-byte suffix of M is added last: it is the last exact pattern in the device's pool and a multiple of 4
long, so the compare's look-ahead load behind it is the pool's spare word.  The state at the end of a
master lists every suffix of that master, so one STATE record at a planted copy's last byte asks for every
length at once, and an entry of length L is kept iff no altered byte lies in the copy's last L bytes.

Expected records are direct slice compares (hay[a:o + 1] == pattern), list order from the model's lists.
"""
import numpy as np

M = b"aBcDeFgHiJkLmNoPqRAbCdEfGhIjKlMnO"
M13 = b"sTuVwXyZStUvW"
FILL = b".,;:-_+=0123456789"                  # none of the masters' letters, in either case
assert len(M) == 33 and len(set(M)) == 33 and len(M13) == 13 and len(set(M13)) == 13
assert not set(bytes(M + M13).lower()) & set(FILL) and not set(M.lower()) & set(M13.lower())

M_LENGTHS = list(range(1, 21)) + [33]
PATS = [(M[-L:], False) for L in M_LENGTHS] + [(M[-2:], True)] + \
       [(M13[-L:], False) for L in range(1, 14)] + [(M13[-2:], True)] + [(M[-24:], False)]
OF_M = set(range(len(M_LENGTHS) + 1)) | {len(PATS) - 1}        # the patterns that are suffixes of M
OF_M13 = set(range(len(PATS))) - OF_M
assert len(PATS[-1][0]) % 4 == 0 and not PATS[-1][1]

BIT_CASE, BIT_OTHER = 0x20, 0x01


def altered(master, j, bit=BIT_CASE):
    """master with one bit of byte j flipped (j None: as it is)"""
    b = bytearray(master)
    if j is not None:
        b[j] ^= bit
    return bytes(b)


def filler(rng, n):
    return bytes(rng.choice(np.frombuffer(FILL, dtype=np.uint8), size=n))


def expect(pats, lists, records, hay, lo, text_end, all_patterns):
    """(patterns, offsets) of the records [(state, offset)], by slice compare: hay holds the bytes at stream
    offsets [lo, lo + len(hay)) (before ++ text), lists: state -> its match list.  An exact entry is kept iff
    its bytes lie in hay, end in front of text_end and equal the pattern; one that ignores case always."""
    ep, eo = [], []
    for s, o in records:
        for p in lists[s]:
            pat, nocase = pats[p]
            a = o - len(pat) + 1
            if nocase or (a >= lo and o < text_end and hay[a - lo:o + 1 - lo] == pat):
                ep.append(p)
                eo.append(o)
                if not all_patterns:
                    break
    return np.array(ep, dtype=np.int32), np.array(eo, dtype=np.int64)


def text_only(seed=1):
    """(text, [(index of the copy's last byte, altered position or None, bit)]): one copy of M per altered
    position (none, 0..32), per kind of alteration (a case flip, bit 0) and per residue 0..3 of the copy's
    start, filler in between"""
    rng = np.random.default_rng(seed)
    out, copies = bytearray(), []
    for res in range(4):
        for bit in (BIT_CASE, BIT_OTHER):
            for j in [None] + list(range(len(M))):
                out += filler(rng, 1 + (res - len(out) - 1) % 4)
                assert len(out) % 4 == res
                out += altered(M, j, bit)
                copies.append((len(out) - 1, j, bit))
    out += filler(rng, 5)
    return bytes(out), copies


REST = b".7" + M + b";" + M13 + b"--=" + M + b"9."      # plain matches behind every seam
REST_ENDS = [(1 + 33, "M"), (1 + 33 + 1 + 13, "M13"), (1 + 33 + 1 + 13 + 3 + 33, "M")]   # index in REST, master


class Seam:
    """one planted copy of a master, its first k bytes in `before` and the rest at the start of the text,
    REST behind it.  mode: "exact" (before is those k bytes), "fewer" (the last k - 1 of them: the longest
    entry reaches outside), "spare" (five filler bytes in front of them)."""
    SPARE = 5

    def __init__(self, master, k, j, mode="exact", bit=BIT_CASE):
        self.master, self.k, self.j, self.mode = master, k, j, mode
        alt = altered(master, j, bit)
        self.in_before = alt[:k]
        self.text = alt[k:] + REST
        self.before = {"exact": alt[:k], "fewer": alt[1:k], "spare": FILL[:self.SPARE] + alt[:k]}[mode]
        self.name = "M13" if master == M13 else "M"

    def records(self, state_of, origin):
        """[(state, stream offset)]: the seam copy's last byte, then REST's copies"""
        n = len(self.master) - self.k
        return [(state_of[self.name], origin + n - 1)] + [(state_of[w], origin + n + e) for e, w in REST_ENDS]

    def expect(self, lists, state_of, origin, all_patterns):
        return expect(PATS, lists, self.records(state_of, origin), self.before + self.text, origin - len(self.before),
                      origin + len(self.text), all_patterns)


def seams_13():
    """every split, every altered position, every before form (k = 0 has no byte to leave out)"""
    return [Seam(M13, k, j, mode) for k in range(14) for j in [None] + list(range(13))
            for mode in ("exact", "fewer", "spare") if not (mode == "fewer" and k == 0)]


def seams_33():
    """every split of M: unaltered, the last byte in before altered, the first byte in the text altered"""
    out = []
    for k in range(34):
        for j in {None, k - 1 if k >= 1 else None, k if k <= 32 else None}:
            out.append(Seam(M, k, j))
    return sorted(out, key=lambda s: (s.k, -1 if s.j is None else s.j))
