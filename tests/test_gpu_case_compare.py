"""The byte compare of the case pass (same_bytes in csrc/case.hip) swept over every path it takes: the byte
loop over `before` and up to the text's first aligned word, the word loop at every shift of the pattern
against the text, the byte tail.  tests/case_compare.py holds the set (the suffixes of two master strings, so
one record asks for every length at once), the planted copies and the expected records, which are slice
compares; tests/test_host_case.py pins them to the model without a GPU.

  text only   a copy of the 33-byte master per altered byte (none, 0..32), per kind of alteration (a case
              flip; bit 0, which is none) and per residue of its start, the whole batch at every residue of
              the text pointer and two text origins
  the seam    a 13-byte master cut at every byte between `before` and the text, every byte altered, every
              residue of the text pointer, `before` as long as the match needs, a byte shorter, and longer;
              the 33-byte master cut at every byte with the bytes next to the seam altered, one residue each

Planes are hand-built (one STATE record at a copy's last byte), every call runs in both forms with poisoned
output planes and a poisoned workspace of its own, and the output planes are compared whole: count, records,
trailer, the poison behind the trailer and behind the capacity.  The bytes in front of the text pointer and
behind `before` are those that would mend an altered copy: a read on the wrong side of the seam keeps an
entry.  The calls of a sweep are enqueued back to back and read back once (Batch): a call costs its two
launches."""
import numpy as np
import pytest

import case_compare as cc
import case_model as cm
import poison
from gpu_pattern_matching_amd import DeviceArray, Matcher

pytestmark = pytest.mark.gpu

P = poison.PLANE_POISON
PV = poison.cell(P)
SLACK = 16                                   # guard cells behind every output plane
TRAILER = 77
ORIGIN = 1001


class Env:
    def __init__(self):
        a = cm.build(cc.PATS)
        assert a.mixed_case
        self.model = cm.CaseModel(cc.PATS)
        self.state_of = {"M": self.model.walk(cc.M)[2], "M13": self.model.walk(cc.M13)[2]}
        self.lists = {s: self.model.list_of(s) for s in self.state_of.values()}
        # the state at the end of a master lists every suffix of it
        assert sorted(self.lists[self.state_of["M"]]) == sorted(cc.OF_M)
        assert sorted(self.lists[self.state_of["M13"]]) == sorted(cc.OF_M13)
        self.m = Matcher(a, 0, max_text=4096)
        self.bufs = []

    def buf(self, nbytes):
        b = DeviceArray(max(nbytes, 16))
        assert b.ptr % 4 == 0
        self.bufs.append(b)
        return b

    def upload(self, host, pad_to=16):
        b = DeviceArray.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8), pad_to=pad_to)
        assert b.ptr % 4 == 0
        self.bufs.append(b)
        return b

    def planes(self, records):
        """device state and offset planes of [(state, offset)]"""
        cells = [[len(records)] + [r[k] for r in records] + [TRAILER] for k in (0, 1)]
        return [DeviceArray.from_numpy(np.array(c, dtype=np.int64).astype(np.int32), pad_to=0) for c in cells]

    def close(self):
        for b in self.bufs:
            b.free()
        self.m.close()


@pytest.fixture(scope="module")
def env(gpu):
    e = Env()
    yield e
    e.close()


class Batch:
    """calls of one shape -- at most max_records records into cap cells -- each with output planes and a
    workspace of its own in two buffers that are poisoned once, up front: add() only enqueues, so the calls
    run back to back on the stream; finish() reads everything back once and compares every call's planes whole"""

    def __init__(self, env, max_records, cap, calls):
        self.env, self.max_records, self.cap, self.calls = env, max_records, cap, calls
        self.cells = cap + SLACK
        self.out = env.buf(calls * 2 * self.cells * 4)
        self.out.fill(P)
        self.wsb = env.m.lib.acm_case_workspace_bytes(max_records)
        self.ws = env.buf(calls * self.wsb)
        self.ws.fill(0xA5)
        self.exp = np.full((calls, 2, self.cells), PV, dtype=np.int32)
        self.what = []

    def expected(self, exp):
        """the two planes a call must leave for the records exp = (patterns, offsets)"""
        assert exp[0].size + 2 <= self.cap
        return np.stack(cm.planes(exp[0], exp[1], self.cap, PV, TRAILER))

    def add(self, planes, text, origin, end, all_patterns, exp, what, before=None, before_len=0):
        """exp: what expected() made of the call's records"""
        i = len(self.what)
        self.what.append(what)
        self.exp[i, :, :self.cap] = exp
        at = self.out.ptr + i * 2 * self.cells * 4
        self.env.m.case_async(planes[0], planes[1], self.max_records, text, origin, end, at, at + self.cells * 4, self.cap,
                              before=before, before_len=before_len, all_patterns=all_patterns,
                              workspace=(self.ws.ptr + i * self.wsb, self.wsb))

    def finish(self):
        assert len(self.what) == self.calls
        got = self.out.to_numpy(np.int32, self.exp.size).reshape(self.exp.shape)
        for i in np.flatnonzero((got != self.exp).any(axis=(1, 2))).tolist():
            for g, e, name in zip(got[i], self.exp[i], ("pattern", "offset")):
                assert int(g[0]) == int(e[0]), "%s: count %d, expected %d" % (self.what[i], g[0], e[0])
                bad = np.flatnonzero(g[:self.cap] != e[:self.cap])
                assert bad.size == 0, "%s: %s plane differs at %s: %s, expected %s" % (self.what[i], name, bad[:5],
                                                                                       g[bad[:5]], e[bad[:5]])
                assert (g[self.cap:] == PV).all(), "%s: %s plane written behind the capacity" % (self.what[i], name)
        return self.calls


def test_text_only(env):
    text, copies = cc.text_only()
    sM = env.state_of["M"]
    front = 64
    call = Batch(env, len(copies), len(copies) * len(cc.OF_M) + 2 + 7, 2 * 4 * 2)
    kept, keep = set(), []
    for origin in (0, ORIGIN):
        records = [(sM, origin + o) for o, _, _ in copies]
        planes = env.planes(records)
        exps = {ap: cc.expect(cc.PATS, env.lists, records, text, origin, origin + len(text), ap) for ap in (False, True)}
        kept |= set(exps[True][0].tolist())
        assert exps[False][0].size == len(copies) < exps[True][0].size < len(copies) * len(cc.OF_M)
        exps = {ap: call.expected(e) for ap, e in exps.items()}
        for r in range(4):
            d = env.upload((cc.FILL * 8)[:front + r] + text + cc.FILL * 4)
            ptr = d.ptr + front + r
            assert ptr % 4 == r
            for ap in (False, True):
                call.add(planes, ptr, origin, origin + len(text), ap, exps[ap],
                         "text only: origin %d pointer residue %d all %d" % (origin, r, ap))
        keep += planes
    call.finish()
    for x in keep:
        x.free()
    assert kept == cc.OF_M


class Image:
    """one device buffer with a slot per (seam, residue) for the text and one per seam for `before`; residues(seam):
    the residues of the text pointer that seam runs at.  In front
    of a text lie the unaltered bytes the copy has in `before`; behind `before` the unaltered bytes it has in
    the text; in front of a `before` that is a byte short, the byte left out."""
    FRONT, TEXT_SLOT, BEFORE_SLOT = 40, 192, 96

    def __init__(self, env, seams, residues):
        rng = np.random.default_rng(len(seams))
        texts = 4 * len(seams) * self.TEXT_SLOT
        host = bytearray(cc.filler(rng, texts + len(seams) * self.BEFORE_SLOT))
        self.text_at, self.before_at = {}, {}
        for i, s in enumerate(seams):
            for r in residues(s):
                at = (4 * i + r) * self.TEXT_SLOT + self.FRONT + r
                assert len(s.text) < self.TEXT_SLOT - self.FRONT - 3 and s.k <= self.FRONT
                host[at - s.k:at] = s.master[:s.k]
                host[at:at + len(s.text)] = s.text
                self.text_at[i, r] = at
            lead = {"exact": b"", "fewer": s.master[:1], "spare": b""}[s.mode]
            body = lead + s.before + s.master[s.k:]
            at = texts + i * self.BEFORE_SLOT + 8
            assert 8 + len(body) < self.BEFORE_SLOT
            host[at:at + len(body)] = body
            self.before_at[i] = at + len(lead)
        self.host = bytes(host)
        self.d = env.upload(self.host)

    def check(self, i, r, s):
        """the slots hold what the seam says (the test's own layout, on the host)"""
        t, b = self.text_at[i, r], self.before_at[i]
        assert self.host[t:t + len(s.text)] == s.text and self.host[b:b + len(s.before)] == s.before and t % 4 == r


def sweep(env, seams, residues, what):
    img = Image(env, seams, residues)
    call = Batch(env, 4, 96, sum(len(residues(s)) for s in seams) * 2)
    plane_of = {}
    dropped = 0
    for i, s in enumerate(seams):
        key = (s.name, s.k)
        if key not in plane_of:
            plane_of[key] = env.planes(s.records(env.state_of, ORIGIN))
        exps = {ap: s.expect(env.lists, env.state_of, ORIGIN, ap) for ap in (False, True)}
        dropped += exps[True][0].size < 2 * len(cc.OF_M) + len(cc.OF_M13) + len(cc.OF_M if s.name == "M" else cc.OF_M13)
        exps = {ap: call.expected(e) for ap, e in exps.items()}
        nb = len(s.before)
        for r in residues(s):
            img.check(i, r, s)
            for ap in (False, True):
                call.add(plane_of[key], img.d.ptr + img.text_at[i, r], ORIGIN, ORIGIN + len(s.text), ap, exps[ap],
                         "%s: %s split %d altered %s before %s residue %d all %d" % (what, s.name, s.k, s.j, s.mode, r, ap),
                         before=img.d.ptr + img.before_at[i] if nb else None, before_len=nb)
    calls = call.finish()
    for pl in plane_of.values():
        for x in pl:
            x.free()
    assert 0 < dropped < len(seams)
    return calls


def test_seam_13(env):
    """head bytes 0..3, shift 0..3, at least one whole word, tail bytes 0..3: every split k, altered byte j and
    pointer residue r of the 13-byte master, in every form of `before`"""
    seams = cc.seams_13()
    assert sweep(env, seams, lambda s: range(4), "seam 13") == len(seams) * 4 * 2 == (14 * 14 * 3 - 14) * 8


def test_seam_33(env):
    """every split of the 33-byte master, each at one residue of the text pointer: the residue turns with the
    split, so the four of them meet every length of the part in the text modulo 4 within 16 splits (the 13-byte
    grid is the one that crosses everything with everything)"""
    seams = cc.seams_33()
    assert sweep(env, seams, lambda s: [s.k // 4 % 4], "seam 33") == len(seams) * 2 == (34 * 3 - 2) * 2
