"""Scans the way callers run them: on created (non-blocking) streams, several in flight, chained through
the event fields of acm_scan_batch, replayed as HIP graphs, timed in line, enqueued from several host
threads -- every plane compared whole with the CPU oracle (count cell, records, trailer, poison behind
the trailer: poison.check_planes), never one GPU path with another.

The other GPU tests enqueue on the NULL stream from one thread, one pipeline at a time.  Here nothing
orders a scan against its neighbours but what the test enqueues (tests/streams.py makes the streams, the
events and the per-batch text/workspace/planes triples).  Output planes are filled with the poison byte
on the scan's own stream before every scan: a scan that silently did not run cannot pass on left-overs.

  1. every pipeline on a created stream: plain, shard, REPORT_STATE + expand/segment/word passes with no
     host sync, a three-piece d_init_plane chain, a plane overflow
  2. four streams in flight with one acm_dfa of each kind, a different issue form per stream; buffer reuse
     protected by stream order alone; scan -> segment -> case -> position passes chained on two streams
  3. the event fields: recorded on every path (the empty text too), the wait honoured, events and groups
  4. graph replay, counted through acm_scan_graph_stats (Matcher.graph_stats)
  5. in-line profiling: results unchanged, launches as the header says
  6. four host threads against one acm_dfa
"""
import math
import threading

import numpy as np
import pytest

import fixtures
import poison
import position_model as pm
import streams
import variants
from gpu_pattern_matching_amd import Automaton, Matcher, _lib
from test_gpu_position import COMP_W, WITH1, comp_texts
from test_host_segments import oracle_segments

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
N = 192 * KiB + 37          # ragged: not a multiple of 16, of a chain or of a tile
EE = poison.PLANE_POISON
HEAD, STATE = _lib.REPORT_HEAD, _lib.REPORT_STATE
ACM_ERR_ARG = -1          # acmatch.h


class Pipe:
    """one launch shape: the regime of its set (variants.REGIMES), the mode and knobs that select it"""

    def __init__(self, name, regime, mode, S=0, env=None, n=N, lds=False, check=None):
        self.name, self.regime, self.mode, self.S, self.env, self.n, self.lds = name, regime, mode, S, env or {}, n, lds
        self.check = check or (lambda vs: True)

    @property
    def path(self):
        return "sparse" if self.mode == "sparse" else "chain"


PIPES = [
    Pipe("sparse-W1", "s3_letters", "sparse", check=lambda vs: vs.stride == 1),
    Pipe("sparse-W2", "s4_letters", "sparse", check=lambda vs: vs.stride == 2),
    Pipe("sparse-W4", "s6_c33", "sparse", check=lambda vs: vs.stride == 4 and vs.key_len == 3),
    Pipe("sparse-W8", "s10_letters", "sparse", check=lambda vs: vs.stride == 8 and vs.key_len == 3),
    Pipe("sparse-6-byte-keys", "s16_letters", "sparse", check=lambda vs: vs.key_len == 6),
    Pipe("speculative", "l150_letters", "chain", S=32, check=lambda vs: vs.longest - 1 > 32),
    Pipe("halo-preload", "l32_binary", "chain", S=32, check=lambda vs: vs.longest - 1 <= 32),
    Pipe("halo-no-preload", "l16_binary", "chain", S=32, env={"ACM_SCAN_NO_PRELOAD": "1"}),
    Pipe("wide-pre", "l150_c9", "chain", n=16 * MiB + 5, check=lambda vs: vs.longest > 64),
    Pipe("lds-walk", "lds33_c33", "chain", lds=True),
    Pipe("big-not-lds", "big_c17", "chain", S=32, check=lambda vs: vs.states[0] > 16384),
    Pipe("nocase", "s8_mixed", "sparse", check=lambda vs: vs.nocase),
]
BY_NAME = {p.name: p for p in PIPES}
FOUR = [BY_NAME[k] for k in ("sparse-W4", "speculative", "halo-preload", "lds-walk")]   # sparse, speculative, halo, LDS walk


def ids(pipes):
    return [p.name for p in pipes]


def setup(pipe, monkeypatch):
    """(VariantSet, oracle, Matcher) configured for the pipe"""
    for k, v in pipe.env.items():
        monkeypatch.setenv(k, v)
    vs = variants.regime(pipe.regime)
    assert pipe.check(vs), "regime %s no longer selects %s" % (pipe.regime, pipe.name)
    a, o = vs.compiled()
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    a.close()
    assert m.set_mode(pipe.mode) == pipe.mode
    if pipe.S:
        assert m.set_chain_bytes(pipe.S) == pipe.S
    if pipe.mode == "chain":   # the LDS walk, or the cold-plane walk kernels
        assert m.lds_resident() == pipe.lds
    if pipe.mode == "sparse":
        assert m.sparse_eligible()
    return vs, o, m


def named(name):
    """a Matcher of a fixture set (fixtures.oracle_for(name) is its oracle)"""
    path, hx, ml = fixtures.set_source(name)
    a = Automaton()
    a.load_file(path, hx, ml)
    a.compile()
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    a.close()
    return m


def named_text(name, n, seed):
    if name == "sentiment":
        return fixtures.text_for({"kind": "words", "n": n, "seed": seed}, None)
    return fixtures.text_for({"kind": "clamav", "n": n, "seed": seed, "n_plant": max(4, n // 2048)},
                             fixtures.patterns_of(name))


def scan_on(m, tr, s, **kw):
    """poison the triple's planes and enqueue its scan, both on stream s"""
    tr.poison(s)
    m.enqueue(tr.batch(s, **kw))


def sharded(o, vs, piece, h, shift):
    """what a shard scan of piece (h bytes of halo in front) reports: the oracle's records of piece that end
    behind the halo, offsets shifted"""
    e = o.scan(vs.text_of(piece))
    keep = e[0] >= h
    return e[0][keep].astype(np.int64) + shift, e[1][keep], e[2]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("pipe", PIPES, ids=ids(PIPES))
def test_pipeline_on_a_created_stream(gpu, monkeypatch, pipe):
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    n = pipe.n
    rng = np.random.default_rng(n + len(pipe.name))
    try:
        s = rig.stream()
        t = variants.text(vs, n, 21, "planted")
        ft = vs.text_of(t)
        init = int(rng.integers(1, o.num_states))
        # a plain scan, a state carried in
        tr = rig.triple(m, t)
        scan_on(m, tr, s, init_state=init)
        exp = o.scan(ft, init)
        assert exp[0].size > 8
        tr.check(exp, s, pipe.name + " plain")
        assert tr.path(s) == pipe.path
        # a shard: the longest pattern's halo in front, offsets in the whole text's coordinates
        lo, h = n // 2 + 5, vs.longest - 1
        piece = t[lo - h:]
        sh = rig.triple(m, piece, room=n)
        scan_on(m, sh, s, halo=h, offset_shift=lo - h)
        sh.check(sharded(o, vs, piece, h, lo - h), s, pipe.name + " shard")
        assert sh.path(s) == pipe.path
        # REPORT_STATE, then the expand, segment and word passes behind it on the stream: no host sync between
        full = streams.oracle_all(o, ft, init)
        mr = tr.cap - 2
        starts = np.sort(rng.choice(np.arange(1, n), 300, replace=False)).astype(np.int64)
        starts = np.concatenate([starts[:150], starts[150:151], starts[150:]])   # one empty segment
        nseg = int(starts.size)
        d_st = rig.upload(starts.astype(np.int32), pad_to=0)
        wexp = streams.words(o, vs, t, init)
        ocap = max(full[0].size, wexp[0].size) + 2 + 64
        xws, sws, wws = (rig.buf(f(mr), 0xA5) for f in (m.lib.acm_expand_workspace_bytes,
                                                       m.lib.acm_segment_workspace_bytes,
                                                       m.lib.acm_word_workspace_bytes))
        xp, xq = rig.planes(ocap)
        sp, sq = rig.planes(tr.cap)
        sg, cnt = rig.buf(tr.cap * 4, EE), rig.buf(nseg * 4, EE)
        wp, wq = rig.planes(ocap)
        scan_on(m, tr, s, init_state=init, report=STATE)
        _lib.check(m.lib.acm_expand_matches_async(m.dfa, tr.pat.ptr, tr.off.ptr, mr, xp.ptr, xq.ptr, ocap, xws.ptr,
                                                  m.lib.acm_expand_workspace_bytes(mr), s), "acm_expand_matches_async")
        m.segment_async(tr.pat, tr.off, mr, d_st, nseg, n, sp, sq, tr.cap, seg_out=sg, seg_counts=cnt, report=HEAD,
                        workspace=(sws.ptr, m.lib.acm_segment_workspace_bytes(mr)), stream=s)
        m.word_async(tr.pat, tr.off, mr, tr.text, 0, n, wp, wq, ocap, word_mask=Matcher.word_mask(sorted(streams.HALF)),
                     all_patterns=True, workspace=(wws.ptr, m.lib.acm_word_workspace_bytes(mr)), stream=s)
        tr.check(exp, s, pipe.name + " states", pat_cells=False)
        poison.check_planes(xp, xq, ocap, full, what=pipe.name + " expansion", stream=s)
        eo, ep, es, ec, ef = oracle_segments(o, ft, starts, init)
        poison.check_planes(sp, sq, tr.cap, (eo, ep, ef), what=pipe.name + " segment pass", stream=s)
        assert np.array_equal(sg.to_numpy(np.int32, eo.size + 1, stream=s)[1:], es), "segment ids differ"
        assert np.array_equal(cnt.to_numpy(np.int32, nseg, stream=s), ec), "per-segment counts differ"
        assert 0 < wexp[0].size < full[0].size
        poison.check_planes(wp, wq, ocap, wexp, what=pipe.name + " word pass", stream=s)
        # three pieces, cut inside matches, each starting in the state the piece in front left on the device
        k1, k2 = exp[0].size // 3, 2 * exp[0].size // 3
        cuts = [0, int(exp[0][k1]), int(exp[0][k2]) - 1, n]
        pieces = [rig.triple(m, t[cuts[i]:cuts[i + 1]]) for i in range(3)]
        for i, p in enumerate(pieces):
            p.poison(s)
            m.enqueue(p.batch(s, init_state=init if i == 0 else 0, init_plane=pieces[i - 1].pat if i else None,
                              init_plane_capacity=pieces[i - 1].cap if i else 0))
        state = init
        for i, p in enumerate(pieces):
            e = o.scan(ft[cuts[i]:cuts[i + 1]], state)
            p.check(e, s, "%s piece %d of a d_init_plane chain" % (pipe.name, i))
            state = e[2]
        assert state == exp[2]
        # more records than the planes hold
        small = rig.triple(m, t, cap=10)
        scan_on(m, small, s, init_state=init)
        small.check(exp, s, pipe.name + " overflow")
        assert small.path(s) == pipe.path
    finally:
        rig.close()
        m.close()
        o.close()


# ------------------------------------------------------------------------------------------------ 2
SIZES = (256 * KiB, 64 * KiB, 100003)
FORMS = ("singles", "groups", "chain", "head-state")


def flight(rig, ms, seed0):
    """per stream and per set six batches of their own, and what the oracle says about them.  The group
    stream gets five batches of one size and a ragged one (a launch group needs equal sizes)."""
    plan = []
    for si, form in enumerate(FORMS):
        s = rig.stream()
        for name, m in ms.items():
            o = fixtures.oracle_for(name)
            sizes = [SIZES[0]] * 5 + [SIZES[2]] if form == "groups" else [SIZES[k % 3] for k in range(6)]
            trs = []
            for k, n in enumerate(sizes):
                t = named_text(name, n, seed0 + 100 * si + 10 * len(name) + k)
                tr = rig.triple(m, t, room=SIZES[0])
                tr.report = STATE if form == "head-state" and k % 2 else HEAD
                tr.exp = o.scan(t)
                trs.append(tr)
            plan.append((form, s, name, m, trs))
    return plan


def issue_round_robin(plan):
    """Enqueue everything, a unit per stream in turn, nothing synchronised.  acm_scan_set_mode and
    acm_scan_set_max_group are read when a batch is enqueued, so one acm_dfa serves mixed modes as long as
    the (single) issuing thread switches between its calls -- which this does."""
    units = []
    for form, s, name, m, trs in plan:
        mode = "chain" if form == "chain" or not m.sparse_eligible() else "sparse"
        if form == "groups":
            units.append([(m, mode, s, trs)])
        else:
            units.append([(m, mode, s, [tr]) for tr in trs])
    for k in range(max(len(u) for u in units)):
        for u in units:
            if k >= len(u):
                continue
            m, mode, s, trs = u[k]
            assert m.set_mode(mode) == mode
            for tr in trs:
                tr.poison(s)
            batches = [tr.batch(s, report=tr.report) for tr in trs]
            if len(batches) > 1:
                assert m.group_capable()
                m.enqueue_many(batches)
            else:
                m.enqueue(batches[0])


def check_flight(rig, plan, what):
    for form, s, name, m, trs in plan:
        rig.sync(s)
    for form, s, name, m, trs in plan:
        path = "chain" if form == "chain" or not m.sparse_eligible() else "sparse"
        for k, tr in enumerate(trs):
            w = "%s: %s stream, %s batch %d" % (what, form, name, k)
            tr.check(tr.exp, s, w, pat_cells=tr.report == HEAD)
            assert tr.path(s) == path, w


def two_sets():
    ms = {"clamav2000": named("clamav2000"), "sentiment": named("sentiment")}
    assert ms["clamav2000"].sparse_eligible() and ms["sentiment"].lds_resident()
    assert ms["clamav2000"].set_max_group(4) == 4 and ms["sentiment"].set_max_group(16) == 16
    return ms


def test_streams_in_flight_together(gpu):
    """four streams x two sets x six batches, each with its own text, workspace and planes, enqueued round
    robin with no synchronisation: singles, launch groups (of at most 4 for the signature set's sparse
    kernels, of at most 16 for the LDS walk), forced chain mode, HEAD and STATE reports in alternation"""
    ms = two_sets()
    rig = streams.Rig()
    try:
        plan = flight(rig, ms, 1000)
        issue_round_robin(plan)
        check_flight(rig, plan, "in flight")
    finally:
        rig.close()
        for m in ms.values():
            m.close()


def test_streams_reuse_their_buffers(gpu):
    """three rounds through the same buffers; within a round every buffer is scanned twice, a decoy text
    and then the round's text copied in on the stream in front of each scan with no synchronisation:
    stream order alone keeps the second copy behind the first scan and the second scan behind its copy"""
    ms = two_sets()
    rig = streams.Rig()
    try:
        plan = flight(rig, ms, 2000)
        for r in range(3):
            keep = []
            for form, s, name, m, trs in plan:
                for k, tr in enumerate(trs):
                    decoy = named_text(name, tr.n, 3000 + 7 * r + k)
                    keep.append(decoy)
                    tr.set_text(decoy, s)
            issue_round_robin(plan)
            for form, s, name, m, trs in plan:
                o = fixtures.oracle_for(name)
                for k, tr in enumerate(trs):
                    t = np.roll(tr.t, 4099 * (r + 1) + k)
                    t[:64] = tr.t[:64][::-1]
                    tr.set_text(t, s)
                    tr.exp = o.scan(t)
            issue_round_robin(plan)
            check_flight(rig, plan, "round %d" % r)
            del keep
    finally:
        rig.close()
        for m in ms.values():
            m.close()


class PassSet:
    """the buffers of one scan -> segment -> case -> position chain: a triple for the scan, the segment table,
    the planes and the workspace of every pass, the position pass's info cells"""
    INFO = 4 + 16

    def __init__(self, rig, m, room, max_segments):
        self.rig, self.m = rig, m
        self.tr = rig.triple(m, np.zeros(room, dtype=np.uint8))
        cap = self.tr.cap
        self.mr, self.icap = cap - 2, 8 * cap
        self.d_st = rig.buf(max_segments * 4, EE)
        self.seg, self.case, self.pos = rig.planes(cap), rig.planes(self.icap), rig.planes(self.icap)
        self.info = rig.buf(self.INFO * 4, EE)
        self.wsb = (m.lib.acm_segment_workspace_bytes(self.mr), m.lib.acm_case_workspace_bytes(self.mr),
                    m.lib.acm_position_workspace_bytes(self.icap - 2))
        self.ws = [rig.buf(b) for b in self.wsb]

    def steps(self, s, job):
        """what one stream enqueues, a step per entry: the text and its table copied in, every output and
        workspace poisoned, then the four launches -- all on s, nothing synchronised"""
        tr, m, n, nseg = self.tr, self.m, job.t.size, job.starts.size

        def load():
            tr.set_text(job.t, s)
            self.rig.h2d(self.d_st, job.starts, s)

        def spoil():
            tr.poison(s)
            for b in self.seg + self.case + self.pos + (self.info,):
                b.fill(EE, s)
            for k, b in enumerate(self.ws):
                b.fill((0xA5, 0xFF)[k % 2], s)
        return [load, spoil,
                lambda: m.enqueue(tr.batch(s, report=STATE)),
                lambda: m.segment_async(tr.pat, tr.off, self.mr, self.d_st, nseg, n, self.seg[0], self.seg[1], tr.cap,
                                        report=STATE, workspace=(self.ws[0].ptr, self.wsb[0]), stream=s),
                lambda: m.case_async(self.seg[0], self.seg[1], self.mr, tr.text, 0, n, self.case[0], self.case[1],
                                     self.icap, all_patterns=True, workspace=(self.ws[1].ptr, self.wsb[1]), stream=s),
                lambda: m.position_async(self.case[0], self.case[1], self.icap - 2, self.pos[0], self.pos[1], self.icap,
                                         self.info, report=HEAD, seg_start=self.d_st, segments=nseg, lead_begin=0,
                                         text_end=n, open_end=n if job.closed else -1, all_patterns=job.all_patterns,
                                         workspace=(self.ws[2].ptr, self.wsb[2]), stream=s)]

    def check(self, s, job, what):
        tr = self.tr
        poison.check_planes(tr.pat, tr.off, tr.cap, job.scan, what=what + " scan", stream=s)
        poison.check_planes(self.seg[0], self.seg[1], tr.cap, job.seg, what=what + " segment pass", stream=s)
        poison.check_planes(self.case[0], self.case[1], self.icap, job.case, what=what + " case pass", stream=s)
        poison.check_planes(self.pos[0], self.pos[1], self.icap, job.pos[:3], what=what + " position pass", stream=s)
        info = self.info.to_numpy(np.int32, self.INFO, stream=s)
        assert info[:4].tolist() == [job.pos[3], 0, 0, 0] and (info[4:] == poison.cell(EE)).all(), what + " info"


class PassJob:
    """texts, packed, and what the model says every pass of the chain leaves: (offsets, cells, trailer)"""

    def __init__(self, model, texts, all_patterns, closed):
        self.t, self.starts = Matcher.pack_segments(texts)
        self.all_patterns, self.closed = all_patterns, closed
        states, offs, last = model.walk(self.t)
        self.scan = (offs, states, last)
        so, ss, co, cp, base = [], [], [], [], 0
        for t in texts:
            states, offs, last = model.walk(t)
            so.append(offs + base)
            ss.append(states)
            for st, o in zip(states.tolist(), offs.tolist()):
                for p in model.list[st, :model.list_len[st]].tolist():
                    if model.then_keeps("case", p, o, t):
                        co.append(o + base)
                        cp.append(p)
            base += len(t)
        self.seg = (np.concatenate(so), np.concatenate(ss), last)
        self.case = (np.array(co, dtype=np.int64), np.array(cp, dtype=np.int64), last)
        self.pos = model.records(texts, all_patterns, then="case", open_end="end" if closed else None)
        assert self.pos[2] == last and (self.pos[3] > 0) == (not closed) and self.scan[0].size > self.seg[0].size > 0      # texts cut matches
        assert self.case[0].size > self.pos[0].size > 15 and self.case[0].size != self.seg[0].size


def test_case_and_position_passes_chained_on_two_streams(gpu):
    """scan(STATE) -> segment pass (STATE form) -> case pass (all patterns) -> position pass (pattern-form
    input) on two created streams, a text and a segment table of its own on each, issued step by step in
    turn with no host sync; then again with the two streams' buffers swapped, the other stream's records
    still in them: every plane of every pass whole against the models, and the undecided count"""
    a = pm.build(WITH1, COMP_W)
    assert a.mixed_case and a.positioned
    model = pm.PositionModel(WITH1, COMP_W)
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    a.close()
    rig = streams.Rig()
    try:
        texts = comp_texts()
        jobs = [PassJob(model, texts, True, True),           # the second: the last text's end is not known
                PassJob(model, texts[::-1][5:] + [b"aBcd.abc", b"", b"Abcd d"], False, False)]
        assert jobs[0].t.size != jobs[1].t.size and jobs[0].starts.size != jobs[1].starts.size
        room = max(j.t.size for j in jobs)
        sets = [PassSet(rig, m, room, max(j.starts.size for j in jobs)) for _ in jobs]
        ss = [rig.stream(), rig.stream()]
        for turn, order in enumerate(((0, 1), (1, 0))):
            plan = [sets[order[k]].steps(ss[k], jobs[k]) for k in range(2)]
            for step in zip(*plan):
                for enqueue in step:
                    enqueue()
            for k in range(2):
                sets[order[k]].check(ss[k], jobs[k], "turn %d stream %d" % (turn, k))
    finally:
        rig.close()
        m.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("pipe", FOUR, ids=ids(FOUR))
def test_event_chain_over_three_streams(gpu, monkeypatch, pipe):
    """batch k records E[k] behind its first kernel, batch k + 1 on the next stream waits for it.  Every E[k]
    must have been recorded -- between two events the test records on batch k's stream around the enqueue:
    acm_rt_event_elapsed_ms fails on an event that never was -- and every plane must be the oracle's."""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        ss = [rig.stream() for _ in range(3)]
        trs = [rig.triple(m, variants.text(vs, N - 16 * (k % 2), 30 + k, "planted")) for k in range(7)]
        E = [rig.event() for _ in trs]
        around = [(rig.event(), rig.event()) for _ in trs]
        for k, tr in enumerate(trs):
            s = ss[k % 3]
            tr.poison(s)
            rig.record(around[k][0], s)
            m.enqueue(tr.batch(s, wait=E[k - 1] if k else None, record=E[k], init_state=k))
            rig.record(around[k][1], s)
        for s in ss:
            rig.sync(s)
        for k, tr in enumerate(trs):
            tr.check(o.scan(vs.text_of(tr.t), k), ss[k % 3], "%s batch %d" % (pipe.name, k))
            assert tr.path(ss[k % 3]) == pipe.path
            for a, b in ((around[k][0], E[k]), (E[k], around[k][1])):
                rc, ms = rig.elapsed(a, b)
                assert rc == _lib.ACM_OK and ms >= 0, "batch %d: record_after_walk not recorded (%d, %r)" % (k, rc, ms)
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("pipe", FOUR, ids=ids(FOUR))
def test_empty_text_records_its_event(gpu, monkeypatch, pipe):
    """The header: batch k + 1's first kernel waits for the event batch k records.  A batch of no bytes has
    no walk, but the batch behind it still waits on its event -- left unrecorded that is a wait on whatever
    the event recorded last, or on nothing.  So an empty batch records it too (behind the kernel that writes
    its header and trailer), with d_init_plane or without."""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        a, b = rig.stream(), rig.stream()
        first = rig.triple(m, variants.text(vs, N, 41, "planted"))
        empty = rig.triple(m, np.zeros(0, dtype=np.uint8), room=64)
        carried = rig.triple(m, np.zeros(0, dtype=np.uint8), room=64)
        after = rig.triple(m, variants.text(vs, N, 42, "planted"))
        e1, e2, start, end = (rig.event() for _ in range(4))
        exp = o.scan(vs.text_of(first.t))
        scan_on(m, first, a)
        rig.record(start, a)
        scan_on(m, empty, a, record=e1, init_state=7)
        scan_on(m, carried, a, record=e2, init_plane=first.pat, init_plane_capacity=first.cap)
        rig.record(end, a)
        scan_on(m, after, b, wait=e2, init_plane=carried.pat, init_plane_capacity=carried.cap)
        rig.sync(a)
        rig.sync(b)
        none = np.zeros(0, dtype=np.uint32)
        empty.check((none, none, 7), a, pipe.name + " empty")
        carried.check((none, none, exp[2]), a, pipe.name + " empty, state carried")
        after.check(o.scan(vs.text_of(after.t), exp[2]), b, pipe.name + " behind the empty batches")
        for ev in (e1, e2):
            for x, y in ((start, ev), (ev, end)):
                rc, ms = rig.elapsed(x, y)
                assert rc == _lib.ACM_OK and ms >= 0, "an empty batch did not record its event (%d, %r)" % (rc, ms)
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("pipe", FOUR, ids=ids(FOUR))
def test_wait_before_walk_is_honoured(gpu, monkeypatch, pipe):
    """Stream A: some milliseconds of copies, then the text copied into X, then batch k (another text)
    recording E.  Stream B, nothing in front: batch k + 1 scans X and waits for E.  X held other bytes
    before, so only a scan that waited sees the text.  (Seen red once with the hipStreamWaitEvent call
    taken out of a scratch copy of the dispatcher (dispatch.cpp, then part of scan.hip): wrong records, as expected.)"""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        a, b = rig.stream(), rig.stream()
        real = variants.text(vs, N, 51, "planted")
        before = variants.text(vs, N, 52, "dense" if pipe.mode != "sparse" else "random")
        assert o.scan(vs.text_of(before))[0].size != o.scan(vs.text_of(real))[0].size
        src = rig.upload(real)
        other = rig.triple(m, variants.text(vs, N, 53, "planted"))
        x = rig.triple(m, before)
        x.t = real
        big = [rig.buf(256 * MiB, 0x11), rig.buf(256 * MiB, 0x22)]
        e = rig.event()
        for k in range(12):
            rig.d2d(big[k % 2], big[1 - k % 2], 256 * MiB, a)
        rig.d2d(x.text, src, real.size, a)
        scan_on(m, other, a, record=e)
        scan_on(m, x, b, wait=e)
        rig.sync(b)
        x.check(o.scan(vs.text_of(real)), b, pipe.name + " the batch that waited")
        other.check(o.scan(vs.text_of(other.t)), a, pipe.name + " the batch that recorded")
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("pipe", [BY_NAME["sparse-W4"], BY_NAME["lds-walk"]], ids=["sparse-W4", "lds-walk"])
def test_events_inside_enqueue_many(gpu, monkeypatch, pipe):
    """a batch with event fields between groupable batches has its launches to itself (groupable, dispatch.cpp):
    its event is recorded, its waiter on another stream waits, and every batch is right"""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        a, b = rig.stream(), rig.stream()
        assert m.group_capable()
        trs = [rig.triple(m, variants.text(vs, N, 60 + k, "planted")) for k in range(7)]
        waiter = rig.triple(m, variants.text(vs, N, 70, "planted"))
        e, start, end = rig.event(), rig.event(), rig.event()
        for tr in trs:
            tr.poison(a)
        rig.record(start, a)
        m.enqueue_many([tr.batch(a, record=e if k == 3 else None, init_state=k) for k, tr in enumerate(trs)])
        rig.record(end, a)
        scan_on(m, waiter, b, wait=e)
        rig.sync(a)
        rig.sync(b)
        for k, tr in enumerate(trs):
            tr.check(o.scan(vs.text_of(tr.t), k), a, "%s batch %d of enqueue_many" % (pipe.name, k))
            assert tr.path(a) == pipe.path
        waiter.check(o.scan(vs.text_of(waiter.t)), b, pipe.name + " waiter")
        for x, y in ((start, e), (e, end)):
            rc, ms = rig.elapsed(x, y)
            assert rc == _lib.ACM_OK and ms >= 0
    finally:
        rig.close()
        m.close()
        o.close()


# ------------------------------------------------------------------------------------------------ 4
GRAPH_PIPES = FOUR + [BY_NAME["nocase"]]


class Counted:
    """graph_stats() as deltas: expect(captured, launched) since the last call"""

    def __init__(self, m):
        self.m = m
        self.last = m.graph_stats()

    def expect(self, captured, launched, what=""):
        now = self.m.graph_stats()
        got = (now[0] - self.last[0], now[1] - self.last[1])
        self.last = now
        assert got == (captured, launched), "%s: captured/launched %r, expected %r" % (what, got, (captured, launched))
        assert self.m.set_graphs(-1) is True, what + ": the graph path fell back to plain launches"


def replay(m, o, vs, tr, s, seeds, what, init=0, shard=None, **kw):
    """the same batch enqueued once per seed, another text of the same size copied in and the planes
    poisoned in front of each: every result is the oracle's for the text then in the buffer"""
    for seed in seeds:
        t = variants.text(vs, tr.n, seed, "planted")
        tr.set_text(t, s)
        scan_on(m, tr, s, init_state=init, **kw)
        exp = sharded(o, vs, t, *shard) if shard else o.scan(vs.text_of(t), init)
        tr.check(exp, s, "%s seed %d" % (what, seed), pat_cells=kw.get("report", HEAD) == HEAD)


@pytest.mark.parametrize("pipe", GRAPH_PIPES, ids=ids(GRAPH_PIPES))
def test_graph_replay_per_pipeline(gpu, monkeypatch, pipe):
    """R enqueues of one key: the first plain, the second captures and launches, the rest replay --
    captured 1, launched R - 1 -- for head records, REPORT_STATE, shard arguments and an overflowing
    plane; the text changes and the planes are poisoned between replays"""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.set_graphs(True) is True and not m.group_capable()
        c = Counted(m)
        n = N
        tr = rig.triple(m, variants.text(vs, n, 80, "planted"))
        replay(m, o, vs, tr, s, range(81, 85), pipe.name + " head", init=5)
        assert tr.path(s) == pipe.path
        c.expect(1, 3, "head")
        replay(m, o, vs, tr, s, range(85, 89), pipe.name + " state", init=5, report=STATE)
        c.expect(1, 3, "state")
        h = vs.longest - 1
        replay(m, o, vs, tr, s, range(89, 93), pipe.name + " shard", shard=(h, 1000 - h), halo=h, offset_shift=1000 - h)
        c.expect(1, 3, "shard")
        small = rig.triple(m, tr.t, cap=10)
        replay(m, o, vs, small, s, range(93, 96), pipe.name + " overflow")
        c.expect(1, 2, "overflow")
        assert small.path(s) == pipe.path
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("pipe", FOUR, ids=ids(FOUR))
def test_graph_replay_reads_the_carried_state_on_the_device(gpu, monkeypatch, pipe):
    """a d_init_plane chain of two pieces replayed with other texts each round: the second piece's start
    state is read from the first piece's planes when the graph runs, not baked in at capture"""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.set_graphs(True) is True
        c = Counted(m)
        p0 = rig.triple(m, variants.text(vs, N, 100, "planted"))
        p1 = rig.triple(m, variants.text(vs, 64 * KiB + 3, 101, "planted"))
        finals = set()
        for r in range(4):
            t0 = variants.text(vs, p0.n, 110 + r, "planted")
            long_one = max(vs.patterns, key=len)
            t0[t0.size - len(long_one) + 1:] = np.frombuffer(long_one[:-1], dtype=np.uint8)   # ends inside a pattern
            t0[t0.size - 1 - r] ^= 1 if r else 0
            t1 = variants.text(vs, p1.n, 120 + r, "planted")
            p0.set_text(t0, s)
            p1.set_text(t1, s)
            scan_on(m, p0, s)
            scan_on(m, p1, s, init_plane=p0.pat, init_plane_capacity=p0.cap)
            e0 = o.scan(vs.text_of(t0))
            finals.add(e0[2])
            p0.check(e0, s, "%s round %d piece 0" % (pipe.name, r))
            p1.check(o.scan(vs.text_of(t1), e0[2]), s, "%s round %d piece 1" % (pipe.name, r))
        assert len(finals) > 1, "the carried state must differ between the rounds"
        c.expect(2, 6, "d_init_plane chain")
    finally:
        rig.close()
        m.close()
        o.close()


def test_graph_key_follows_the_knobs(gpu, monkeypatch):
    """acm_scan_set_chain_bytes between enqueues gives another key: one more capture, no stale geometry"""
    pipe = BY_NAME["speculative"]
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.set_graphs(True) is True
        c = Counted(m)
        tr = rig.triple(m, variants.text(vs, N, 130, "planted"))
        replay(m, o, vs, tr, s, (131, 132), "chains of 32")
        c.expect(1, 1, "chains of 32")
        assert m.set_chain_bytes(64) == 64
        replay(m, o, vs, tr, s, (133, 134), "chains of 64")
        c.expect(1, 1, "chains of 64")
        assert m.set_chain_bytes(32) == 32
        replay(m, o, vs, tr, s, (135,), "chains of 32 again")
        c.expect(0, 1, "chains of 32 again")
    finally:
        rig.close()
        m.close()
        o.close()


def test_graph_cache_evicts_and_recaptures(gpu, monkeypatch):
    """40 keys (the cache holds 32), each enqueued twice per cycle, two cycles: the oldest keys are evicted,
    come back as first sightings and are captured again; every result is right"""
    pipe = BY_NAME["sparse-W4"]
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.set_graphs(True) is True
        c = Counted(m)
        n = 64 * KiB + 5
        trs = [rig.triple(m, variants.text(vs, n, 200 + k, "planted")) for k in range(40)]
        for cycle in range(2):
            for k, tr in enumerate(trs):
                replay(m, o, vs, tr, s, (300 + 100 * cycle + 2 * k, 301 + 100 * cycle + 2 * k), "key %d cycle %d" % (k, cycle))
        captured, launched = m.graph_stats()
        assert captured - c.last[0] > 32 and launched - c.last[1] >= captured - c.last[0]
        assert m.set_graphs(-1) is True
    finally:
        rig.close()
        m.close()
        o.close()


def test_graph_of_one_key_on_two_streams(gpu, monkeypatch):
    """the key leaves the stream out: captured on stream A, replayed on stream B"""
    pipe = BY_NAME["lds-walk"]
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        a, b = rig.stream(), rig.stream()
        assert m.set_graphs(True) is True
        c = Counted(m)
        tr = rig.triple(m, variants.text(vs, N, 400, "planted"))
        replay(m, o, vs, tr, a, (401, 402), "stream A")
        c.expect(1, 1, "stream A")
        replay(m, o, vs, tr, b, (403, 404), "stream B")
        c.expect(0, 2, "stream B")
        replay(m, o, vs, tr, a, (405,), "stream A again")
        c.expect(0, 1, "stream A again")
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("pipe", [BY_NAME["sparse-W4"], BY_NAME["lds-walk"]], ids=["sparse-W4", "lds-walk"])
def test_graphs_and_enqueue_many(gpu, monkeypatch, pipe):
    """with graphs on acm_scan_batches_async goes batch by batch (no launch groups): the second round of the
    same four batches captures each, the third replays"""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.group_capable()
        assert m.set_graphs(True) is True
        assert not m.group_capable()
        c = Counted(m)
        trs = [rig.triple(m, variants.text(vs, N, 500 + k, "planted")) for k in range(4)]
        for r in range(3):
            for k, tr in enumerate(trs):
                tr.set_text(variants.text(vs, N, 510 + 10 * r + k, "planted"), s)
                tr.poison(s)
            m.enqueue_many([tr.batch(s, init_state=k) for k, tr in enumerate(trs)])
            for k, tr in enumerate(trs):
                tr.check(o.scan(vs.text_of(tr.t), k), s, "%s round %d batch %d" % (pipe.name, r, k))
        c.expect(4, 8, "enqueue_many")
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("pipe", [BY_NAME["sparse-W4"], BY_NAME["lds-walk"]], ids=["sparse-W4", "lds-walk"])
def test_what_the_graph_path_leaves_out(gpu, monkeypatch, pipe):
    """graphs on, and the NULL stream, an event field, profiling or an empty text: plain launches (launched
    does not move), right results"""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.set_graphs(True) is True
        c = Counted(m)
        tr = rig.triple(m, variants.text(vs, N, 600, "planted"))
        e = rig.event()
        replay(m, o, vs, tr, None, (601, 602, 603), "NULL stream")
        c.expect(0, 0, "NULL stream")
        replay(m, o, vs, tr, s, (604, 605, 606), "record_after_walk", record=e)
        c.expect(0, 0, "record_after_walk")
        replay(m, o, vs, tr, s, (607, 608, 609), "wait_before_walk", wait=e)
        c.expect(0, 0, "wait_before_walk")
        replay(m, o, vs, tr, s, (610, 611, 612), "batch profile", profile=True)
        c.expect(0, 0, "batch profile")
        assert m.profile_read()[3] == 3
        m.profile(True)
        replay(m, o, vs, tr, s, (613, 614, 615), "profiling on")
        m.profile(False)
        c.expect(0, 0, "profiling on")
        assert m.profile_read()[3] == 3
        empty = rig.triple(m, np.zeros(0, dtype=np.uint8), room=64)
        none = np.zeros(0, dtype=np.uint32)
        for _ in range(3):
            scan_on(m, empty, s, init_state=3)
            empty.check((none, none, 3), s, "empty text")
        c.expect(0, 0, "empty text")
    finally:
        rig.close()
        m.close()
        o.close()


# ------------------------------------------------------------------------------------------------ 5
def read_profile(m, launches, what):
    first, second, whole, count = m.profile_read()
    assert count == launches, "%s: %d timed launches, expected %d" % (what, count, launches)
    for v in (first, second, whole):
        assert math.isfinite(v) and v >= 0, "%s: %r" % (what, (first, second, whole))
    assert m.profile_read() == (0.0, 0.0, 0.0, 0), what + ": a second read must find nothing"


@pytest.mark.parametrize("pipe", FOUR, ids=ids(FOUR))
def test_profiled_scans(gpu, monkeypatch, pipe):
    """The header: with profiling on every scan records an event before its first kernel, after it and
    after its last, and acm_scan_profile_read sums them over 'launches' calls and resets.  So three scans
    give launches == 3, for acm_scan_profile_enable and for acm_scan_batch.profile alike (an empty text is
    a call too), and the planes are what they are without the events."""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        trs = [rig.triple(m, variants.text(vs, N - 5 * k, 700 + k, "planted")) for k in range(3)]
        exps = [o.scan(vs.text_of(tr.t), k) for k, tr in enumerate(trs)]
        read_profile(m, 0, "nothing timed yet")
        for how in ("enable", "batch"):
            if how == "enable":
                m.profile(True)
            for k, tr in enumerate(trs):
                scan_on(m, tr, s, init_state=k, profile=how == "batch")
            m.profile(False)
            for k, tr in enumerate(trs):
                tr.check(exps[k], s, "%s profiled (%s) batch %d" % (pipe.name, how, k))
                assert tr.path(s) == pipe.path
            read_profile(m, 3, "%s profiled (%s)" % (pipe.name, how))
        empty = rig.triple(m, np.zeros(0, dtype=np.uint8), room=64)
        scan_on(m, empty, s, init_state=2, profile=True)
        none = np.zeros(0, dtype=np.uint32)
        empty.check((none, none, 2), s, "empty profiled")
        read_profile(m, 1, "empty text")
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("pipe", [BY_NAME["sparse-W4"], BY_NAME["lds-walk"]], ids=["sparse-W4", "lds-walk"])
def test_profiled_launch_groups(gpu, monkeypatch, pipe):
    """acm_scan_batches_async over batches of one size.  A group is timed as a whole or not at all:
      profile = 1 in all four batches          one group, launches == 1
      acm_scan_profile_enable(1)               no groups (timed batches are taken out of them): launches == 4
      profiled, profiled, plain, plain, profiled   groups split where the flag changes: launches == 2
    The planes are the same every time."""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.group_capable()
        trs = [rig.triple(m, variants.text(vs, N, 800 + k, "planted")) for k in range(5)]
        exps = [o.scan(vs.text_of(tr.t), k) for k, tr in enumerate(trs)]

        def run(flags, what, launches):
            for tr in trs[:len(flags)]:
                tr.poison(s)
            m.enqueue_many([tr.batch(s, init_state=k, profile=flags[k]) for k, tr in enumerate(trs[:len(flags)])])
            for k in range(len(flags)):
                trs[k].check(exps[k], s, "%s %s batch %d" % (pipe.name, what, k))
                assert trs[k].path(s) == pipe.path
            read_profile(m, launches, pipe.name + " " + what)

        run([True] * 4, "a profiled group", 1)
        m.profile(True)
        run([False] * 4, "profiling on", 4)
        m.profile(False)
        run([True, True, False, False, True], "profiled and plain batches mixed", 2)
        run([False] * 4, "no profiling", 0)
    finally:
        rig.close()
        m.close()
        o.close()


@pytest.mark.parametrize("bad", (0, 1, 2))
@pytest.mark.parametrize("pipe", [BY_NAME["sparse-W4"], BY_NAME["lds-walk"]], ids=["sparse-W4", "lds-walk"])
def test_group_stops_at_its_failing_member(gpu, monkeypatch, pipe, bad):
    """acm_scan_batches_async "stops at the first batch that fails; the batches before it stay enqueued" --
    inside a launch group too.  Four profiled batches of one size that would form one group; batch 'bad'
    carries an init_state that is no state, which the host rejects before it enqueues anything of that
    batch.  The batches in front of it run as a shorter group (timed as one launch), the planes of the rest
    keep their poison, the call returns ACM_ERR_ARG.  The same four with valid states then form a group
    that is timed as one launch: the events the failed call took went back to the pool."""
    vs, o, m = setup(pipe, monkeypatch)
    rig = streams.Rig()
    try:
        s = rig.stream()
        assert m.group_capable()
        trs = [rig.triple(m, variants.text(vs, N, 900 + k, "planted")) for k in range(4)]
        exps = [o.scan(vs.text_of(tr.t), k) for k, tr in enumerate(trs)]

        def poisoned():
            for tr in trs:
                tr.ws.fill(0xA5, s)
                tr.poison(s)

        poisoned()
        with pytest.raises(_lib.AcmError) as err:
            m.enqueue_many([tr.batch(s, init_state=o.num_states if k == bad else k, profile=True)
                            for k, tr in enumerate(trs)])
        assert err.value.code == ACM_ERR_ARG
        rig.sync(s)
        for k, tr in enumerate(trs):
            what = "%s batch %d, batch %d invalid" % (pipe.name, k, bad)
            if k < bad:
                tr.check(exps[k], s, what)
                assert tr.path(s) == pipe.path, what
            else:
                for plane in (tr.pat, tr.off):
                    cells = plane.to_numpy(np.int32, tr.cap, stream=s)
                    assert np.all(cells == poison.cell(EE)), what + ": written, but nothing of it was to be enqueued"
        read_profile(m, 1 if bad else 0, "%s the group in front of batch %d" % (pipe.name, bad))
        poisoned()
        m.enqueue_many([tr.batch(s, init_state=k, profile=True) for k, tr in enumerate(trs)])
        for k, tr in enumerate(trs):
            tr.check(exps[k], s, "%s batch %d after the failed call" % (pipe.name, k))
            assert tr.path(s) == pipe.path
        read_profile(m, 1, pipe.name + " the whole group after the failed call")
    finally:
        rig.close()
        m.close()
        o.close()


# ------------------------------------------------------------------------------------------------ 6
THREADS = 4


def run_threads(work):
    """work(i, barrier, stop) in THREADS threads behind a barrier; the first exception of a worker is raised
    here, the other workers see stop set (and a broken barrier) and return without enqueueing more"""
    barrier, stop, errors = threading.Barrier(THREADS), threading.Event(), []

    def body(i):
        try:
            work(i, barrier, stop)
        except BaseException as e:   # noqa: B902 -- handed to the main thread
            errors.append((i, e))
            stop.set()
            barrier.abort()

    ts = [threading.Thread(target=body, args=(i,), name="scan-worker-%d" % i) for i in range(THREADS)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    alive = [t.name for t in ts if t.is_alive()]
    stop.set()
    real = [e for e in errors if not isinstance(e[1], threading.BrokenBarrierError)] or errors
    if real:
        raise real[0][1]
    assert not alive, "workers still running: %s" % alive


def threaded(m, rig, jobs, rounds, repeat=lambda i: 1, paths=("chain", "sparse"), graphs=False):
    """jobs[i]: thread i's triples (with .texts: a text per round, .exps: the oracle's records of each).
    Every thread enqueues its triples on its own stream round by round (ctypes drops the GIL in the call),
    then synchronises its stream and compares."""
    ss = [rig.stream() for _ in range(THREADS)]

    def work(i, barrier, stop):
        s = ss[i]
        barrier.wait(60)
        for r in range(rounds):
            for tr in jobs[i]:
                if stop.is_set():
                    return
                tr.set_text(tr.texts[r], s)
                for _ in range(repeat(i)):
                    scan_on(m, tr, s)
            rig.sync(s)
            for k, tr in enumerate(jobs[i]):
                if stop.is_set():
                    return
                tr.check(tr.exps[r], s, "thread %d round %d batch %d" % (i, r, k))
                assert tr.path(s) in paths

    run_threads(work)


def thread_jobs(rig, m, texts_of, scan, per_thread, rounds, size):
    jobs = []
    for i in range(THREADS):
        trs = []
        for k in range(per_thread):
            n = size(k)
            texts = [texts_of(i, k, r, n) for r in range(rounds)]
            tr = rig.triple(m, texts[0])
            tr.texts, tr.exps = texts, [scan(t) for t in texts]
            trs.append(tr)
        jobs.append(trs)
    return jobs


def test_threads_auto_mode(gpu):
    """four threads, AUTO mode: pick_sparse's counters are fed by all of them; either pipeline may run"""
    name = "clamav2000"
    m, o = named(name), fixtures.oracle_for(name)
    rig = streams.Rig()
    try:
        assert m.set_mode("auto") == "auto"
        jobs = thread_jobs(rig, m, lambda i, k, r, n: named_text(name, n, 5000 + 100 * i + 10 * k + r), o.scan, 6, 3,
                           lambda k: SIZES[k % 3])
        threaded(m, rig, jobs, 3)
    finally:
        rig.close()
        m.close()


def test_threads_auto_mode_one_dense_thread(gpu, monkeypatch):
    """one thread's texts are dense in matches (and it enqueues each of them four times), so AUTO moves
    everybody's batches to the chain pipeline for a while, mid-run"""
    vs, o, m = setup(BY_NAME["sparse-W4"], monkeypatch)
    rig = streams.Rig()
    try:
        assert m.set_mode("auto") == "auto"
        jobs = thread_jobs(rig, m, lambda i, k, r, n: variants.text(vs, n, 6000 + 100 * i + 10 * k + r,
                                                                    "dense" if i == 0 else "planted"),
                           lambda t: o.scan(vs.text_of(t)), 6, 4, lambda k: SIZES[k % 3])
        threaded(m, rig, jobs, 4, repeat=lambda i: 4 if i == 0 else 1)
    finally:
        rig.close()
        m.close()
        o.close()


def test_threads_with_graphs(gpu):
    """graphs on, four threads capturing and replaying at once, 40 keys against a cache of 32: lookups,
    evictions and captures of different threads interleave (hipStreamCaptureModeThreadLocal).  Every thread
    has its own buffers: two threads on the very same key would be two scans writing one workspace at once."""
    name = "clamav2000"
    m, o = named(name), fixtures.oracle_for(name)
    rig = streams.Rig()
    try:
        assert m.set_mode("sparse") == "sparse"
        assert m.set_graphs(True) is True
        before = m.graph_stats()
        jobs = thread_jobs(rig, m, lambda i, k, r, n: named_text(name, n, 7000 + 100 * i + 10 * k + r), o.scan, 10, 4,
                           lambda k: SIZES[1])
        threaded(m, rig, jobs, 4, repeat=lambda i: 2, paths=("sparse",))
        captured, launched = m.graph_stats()
        assert launched - before[1] > 0 and captured - before[0] > 0
        assert m.set_graphs(-1) is True
    finally:
        rig.close()
        m.close()
