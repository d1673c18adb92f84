"""Every scan path on recycled memory: poisoned text tails, workspaces, planes and pass inputs.

The other GPU tests upload through DeviceArray.from_numpy (zeros after n) into fresh allocations.  Real
callers do not: acm_grep -t scans packed chunks whose buffer still holds an earlier round's stream,
bench.py takes its workspaces from a caching allocator, output planes are reused across scans whose
record counts differ.  Here (tests/poison.py builds the memory):

A. every row of test_gpu_variants.ROWS scans text views -- inside a match of the longest pattern, at
   n % 16 = 0, 1, 15, either side of tile and chain borders, 1..17 bytes -- with a carried-in state, a
   caller-owned workspace poisoned before every launch and planes filled with 0xEE; head records,
   REPORT_STATE and the expansion, and an overflow into 10 cells;
B. launch groups over adjacent views of one allocation (batch k's bytes past n are batch k + 1's text),
   chained through d_init_plane, with init planes that hold poison in every cell but count and trailer;
C. the segment, word, case and position passes with stale records behind the input trailer, poisoned
   scratch and outputs, starts and d_before with poison behind them, word bytes around the text;
D. acm_grep -t whose packed buffer holds a longer earlier round's bytes behind a shorter stream.

Every cell behind a trailer must still hold the poison, and no byte past n may change a record."""
import os

import numpy as np
import pytest

import fixtures
import orc
import poison
import position_model as pm
import variants
import word_model as wm
from gpu_pattern_matching_amd import DeviceArray, Matcher, _lib
from test_gpu_acm_grep import CLI, run
from test_gpu_variants import ROWS, oracle_all
from test_host_segments import oracle_segments
import test_gpu_words

pytestmark = pytest.mark.gpu

KiB = 1 << 10
DENSE_N = 64 * KiB + 5     # the denser scan whose leftovers are the "stale" fill
EE = poison.PLANE_POISON


def planes(cap, byte=EE):
    p, q = DeviceArray(cap * 4), DeviceArray(cap * 4)
    p.fill(byte)
    q.fill(byte)
    return p, q


def configure(m, row, vs):
    assert m.set_mode(row.mode) == row.mode
    if row.S:
        assert m.set_chain_bytes(row.S) == row.S
    assert m.set_chains_per_lane(row.C) == row.C
    assert m.lds_resident() == (vs.lds and "ACM_SCAN_NO_LDSWALK" not in row.env)


def expanded(o, vs, text, init, head, cap):
    """oracle all-patterns records of the first min(m, cap - 2) head records"""
    pos, pat, last = oracle_all(o, vs.text_of(text), init)
    stored = min(head[0].size, cap - 2)
    if stored < head[0].size:
        keep = pos <= (head[0][stored - 1] if stored else -1)
        pos, pat = pos[keep], pat[keep]
    return pos, pat, last


def expand_check(m, o, vs, P, Q, cap, text, init, head, how, what):
    """acm_expand_matches_async over the STATE planes in P, Q: workspace and output poisoned"""
    exp = expanded(o, vs, text, init, head, cap)
    ocap = exp[0].size + 2 + 64
    ewb = m.lib.acm_expand_workspace_bytes(cap - 2)
    ews = DeviceArray(max(ewb, 16))
    ews.fill(0xA5 if how == "stale" else how)
    xp, xq = planes(ocap)
    try:
        _lib.check(m.lib.acm_expand_matches_async(m.dfa, P.ptr, Q.ptr, cap - 2, xp.ptr, xq.ptr, ocap, ews.ptr, ewb,
                                                  m.stream), "acm_expand_matches_async")
        poison.check_planes(xp, xq, ocap, exp, what=what + " expansion")
    finally:
        for b in (ews, xp, xq):
            b.free()


# ---------------------------------------------------------------------------------------------- A
VIEW_CASES = [(r, f) for r in ROWS for f in (poison.FILLS if r.n <= poison.SMALL else (0xA5,))]


def fill_id(f):
    return f if isinstance(f, str) else "0x%02X" % f


def prime_text(vs, row):
    """what the launch before each scan of a row sees: a dense text for a helped row (more than a flagged
    sample per 512 bytes: the check kernel gets helper waves), else a quiet one"""
    if row.dense:
        return variants.text(vs, poison.SMALL, 7, "dense")
    if vs.outside is not None:
        return np.full(DENSE_N, vs.outside, dtype=np.uint8)
    return variants.text(vs, DENSE_N, 8, "random")


def group_texts(t, count):
    """the texts of a launch group: the row's text first, then rotations of it"""
    return [t] + [np.roll(t, 4099 * k) for k in range(1, count)]


def group_view(texts, n, tail, vs, fold, seed):
    """texts[k][:n] at k * round16(n) of one allocation: the bytes behind a batch are the completion of its
    last pattern prefix and then the next batch's text, behind the last one a tail of kind `tail`"""
    stride = poison.round16(n)
    last = poison.view_host(texts[-1], n, tail, vs.patterns, fold, seed)
    h = np.empty(stride * (len(texts) - 1) + last.size, dtype=np.uint8)
    for k, t in enumerate(texts[:-1]):
        h[k * stride:k * stride + n] = t[:n]
        h[k * stride + n:(k + 1) * stride] = poison.tail_bytes("complete", t, n, stride - n, vs.patterns, fold,
                                                               seed + k)
    h[stride * (len(texts) - 1):] = last
    return DeviceArray.from_numpy(h), stride


@pytest.mark.parametrize("row,how", VIEW_CASES, ids=["%s fill=%s" % (r.kernel, fill_id(f)) for r, f in VIEW_CASES])
def test_view(gpu, monkeypatch, row, how):
    """each cut of the row's text as a view (a launch group of row.group adjacent views), every workspace
    filled with `how` before every launch, planes with 0xEE; the launch before it dense for a helped row
    and quiet otherwise, complete before the scan is enqueued (the host reads its sample count)"""
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    vs = variants.regime(row.regime)
    a, o = vs.compiled()
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    fold = variants.fold if vs.nocase else None
    seed = poison.row_seed(row.regime)
    t, match_cut = poison.row_text(vs, row.n, seed, row.kind)
    cut_list = poison.cuts(row.n, row.S, match_cut)
    inits = poison.init_states(seed, len(cut_list), o.num_states)   # the row's text: as test_host_poison
    more = poison.init_states(seed + 1, len(cut_list) * row.group, o.num_states)
    cap = row.cap or row.n + 2
    count = row.group
    texts = group_texts(t, count)
    prime = prime_text(vs, row)
    wsb = m.lib.acm_scan_workspace_bytes(m.dfa, max(row.n, DENSE_N, prime.size))
    wss = [DeviceArray(wsb) for _ in range(count)]
    ws_prime = DeviceArray(wsb)
    pl = {c: [planes(c) for _ in range(count)] for c in (cap, 10)}
    prime_pl = planes(10)
    d_dense = DeviceArray.from_numpy(variants.text(vs, DENSE_N, 7, "dense"))
    d_prime = DeviceArray.from_numpy(prime)
    keep = wss + [ws_prime, d_dense, d_prime] + list(prime_pl) + [x for c in pl for pr in pl[c] for x in pr]
    try:
        configure(m, row, vs)
        for i, n in enumerate(cut_list):
            s = [inits[i]] + more[i * count + 1:(i + 1) * count]
            tail = poison.TAIL_KINDS[i % 3]
            what = "%s n=%d tail=%s fill=%s" % (row.kernel, n, tail, fill_id(how))
            d, stride = group_view(texts, n, tail, vs, fold, seed + n)
            keep.append(d)
            exps = [o.scan(vs.text_of(x[:n]), s[k], cap=row.cap) for k, x in enumerate(texts)]
            for c in [cap] + ([10] if i == 0 else []):
                def stale():   # a denser scan through the same workspaces and planes
                    for k in range(count):
                        m.scan_async(d_dense, DENSE_N, 0, pat_plane=pl[c][k][0], off_plane=pl[c][k][1],
                                     plane_capacity=c, workspace=(wss[k].ptr, wsb))
                for report in (_lib.REPORT_HEAD, _lib.REPORT_STATE):
                    poison.fill(wss, how, stale)
                    for pp, qq in pl[c]:
                        pp.fill(EE)
                        qq.fill(EE)
                    m.scan_async(d_prime, prime.size, 0, pat_plane=prime_pl[0], off_plane=prime_pl[1],
                                 plane_capacity=10, workspace=(ws_prime.ptr, wsb))
                    _lib.check(m.lib.acm_rt_stream_sync(m.stream), "acm_rt_stream_sync")
                    if count == 1:
                        m.scan_async(d, n, s[0], pat_plane=pl[c][0][0], off_plane=pl[c][0][1], plane_capacity=c,
                                     workspace=(wss[0].ptr, wsb), report=report)
                    else:
                        m.enqueue_many([m.make_batch(d.ptr + k * stride, n, m.stream, pl[c][k][0], pl[c][k][1], c,
                                                     (wss[k].ptr, wsb), init_state=s[k], report=report)
                                        for k in range(count)])
                    for k in range(count):
                        w = "%s batch %d cap=%d %s" % (what, k, c, "state" if report else "head")
                        pp, qq = pl[c][k]
                        poison.check_planes(pp, qq, c, exps[k], what=w, pat_cells=report == _lib.REPORT_HEAD)
                        if report == _lib.REPORT_STATE and k == 0:
                            expand_check(m, o, vs, pp, qq, c, texts[k][:n], s[k], exps[k], how, w)
                if n >= 64 * KiB:
                    for k in range(count):
                        assert m.path_taken(n, workspace=(wss[k].ptr, wsb)) == row.path, what
            d.free()
            keep.remove(d)
    finally:
        for b in keep:
            b.free()
        m.close()
        a.close()
        o.close()


# ---------------------------------------------------------------------------------------------- B
GROUPS = {   # regime, mode, batches, a dense batch first (the check kernel's helper waves)
    "sparse-4": ("s9_letters", "sparse", 4, False),
    "sparse-16-helped": ("s8_binary", "sparse", 16, True),
    "lds-walk-4": ("lds33_c33", "chain", 4, False),
}
GROUP_N = 128 * KiB + 9     # 7 pad bytes behind every batch, then the next batch's text


def adjacent(texts, n, vs, fold, seed):
    """one allocation: batch k at k * round16(n), the bytes between it and batch k + 1 the completion of its
    last pattern prefix, PAST_PAD bytes of completion behind the last"""
    stride = poison.round16(n)
    h = np.empty(stride * len(texts) + poison.PAST_PAD, dtype=np.uint8)
    for k, t in enumerate(texts):
        h[k * stride:k * stride + n] = t
        end = (k + 1) * stride if k + 1 < len(texts) else h.size
        h[k * stride + n:end] = poison.tail_bytes("complete", t, n, end - k * stride - n, vs.patterns, fold, seed + k)
    return DeviceArray.from_numpy(h), stride


def init_plane(cap, count, state):
    """an init plane of cap cells: poison everywhere but the count cell and the trailer cell"""
    c = np.full(cap, poison.cell(0xA5), dtype=np.int32)
    c[0] = count
    c[min(count + 1, cap - 1)] = state
    return DeviceArray.from_numpy(c, pad_to=0)


@pytest.mark.parametrize("group", list(GROUPS))
def test_group_views(gpu, group):
    reg, mode, count, dense = GROUPS[group]
    vs = variants.regime(reg)
    a, o = vs.compiled()
    m = Matcher(a, 0, max_text=GROUP_N)
    fold = variants.fold if vs.nocase else None
    n, cap = GROUP_N, GROUP_N + 2
    rng = np.random.default_rng(count)
    wsb = m.lib.acm_scan_workspace_bytes(m.dfa, n)
    keep = []
    try:
        assert m.set_mode(mode) == mode
        assert m.lds_resident() == (mode == "chain")
        rounds = []
        for r in range(2):
            texts = [variants.text(vs, n, 40 * r + k, ("planted", "runs", "random")[k % 3]) for k in range(count)]
            d, stride = adjacent(texts, n, vs, fold, 40 * r)
            wss = [DeviceArray(wsb) for _ in texts]
            for k, w in enumerate(wss):
                w.fill((0xFF, 0xA5)[k % 2])
            pl = [planes(cap) for _ in texts]
            keep += [d] + wss + [x for p in pl for x in p]
            rounds.append((texts, d, stride, wss, pl))
        # round 0: one launch group, carried-in states
        texts, d, stride, wss, pl = rounds[0]
        inits = [int(rng.integers(0, o.num_states)) for _ in texts]
        if dense:
            m.scan(variants.text(vs, n, 7, "dense"))
        m.enqueue_many([m.make_batch(d.ptr + k * stride, n, m.stream, pl[k][0], pl[k][1], cap, (wss[k].ptr, wsb),
                                     init_state=inits[k]) for k in range(count)])
        finals = []
        for k, t in enumerate(texts):
            exp = o.scan(vs.text_of(t), inits[k])
            poison.check_planes(pl[k][0], pl[k][1], cap, exp, what="%s batch %d" % (group, k))
            assert m.path_taken(n, workspace=(wss[k].ptr, wsb)) == ("chain" if mode == "chain" else "sparse")
            finals.append(exp[2])
        # round 1: every batch goes on from round 0's planes on the device; batches 0 and 1 from init planes
        # with poison in every cell but count and trailer (batch 1: a count beyond the plane, the state in
        # its last cell)
        texts1, d1, stride1, wss1, pl1 = rounds[1]
        ipcap = 64
        crafted = [init_plane(ipcap, 5, finals[0]), init_plane(ipcap, ipcap + 100, finals[1])]
        keep += crafted
        batches = []
        for k in range(count):
            src, scap = (crafted[k], ipcap) if k < 2 else (pl[k][0], cap)
            batches.append(m.make_batch(d1.ptr + k * stride1, n, m.stream, pl1[k][0], pl1[k][1], cap,
                                        (wss1[k].ptr, wsb), init_plane=src, init_plane_capacity=scap))
        m.enqueue_many(batches)
        for k, t in enumerate(texts1):
            poison.check_planes(pl1[k][0], pl1[k][1], cap, o.scan(vs.text_of(t), finals[k]),
                                what="%s chained batch %d" % (group, k))
    finally:
        for b in keep:
            b.free()
        m.close()
        a.close()
        o.close()


# ---------------------------------------------------------------------------------------------- C
PASS_N = 96 * KiB + 3
ORIGIN = 1000                 # text_origin: the scan's offset_shift
FRONT = 64                    # word bytes in front of d_text and of d_before
WORD = ord("q")


def framed(data, front=FRONT, back=poison.PAST_PAD):
    """a device buffer of word bytes with data at byte `front`: (buffer, pointer to data)"""
    h = np.full(front + poison.round16(len(data)) + back, WORD, dtype=np.uint8)
    h[front:front + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    d = DeviceArray.from_numpy(h)
    return d, d.ptr + front


def read_cells(buf, count):
    return buf.to_numpy(np.int32, count)


@pytest.mark.parametrize("nocase", [False, True], ids=["case", "nocase"])
@pytest.mark.parametrize("row", list(test_gpu_words.ROWS))
def test_passes(gpu, monkeypatch, row, nocase):
    name, mode, env, lds = test_gpu_words.ROWS[row]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, a = test_gpu_words.matcher(name, 16, nocase)
    model = wm.WordModel(name, nocase)
    text = wm.planted_text(model.pats, PASS_N, 7, max_len=24)
    last = min((p for p in model.pats if p), key=len)
    # whole words at the very start and the very end
    text = np.concatenate([np.frombuffer(last + b" ", dtype=np.uint8), text, np.frombuffer(b" " + last, np.uint8)])
    short = [p for p in model.pats if 0 < len(p) <= 8] or [last]
    rng = np.random.default_rng(11)
    dense = np.frombuffer(b"".join(short[int(rng.integers(len(short)))] for _ in range(text.size // 2))[:text.size],
                          dtype=np.uint8)   # patterns back to back: many more records than text
    if nocase:
        text = test_gpu_words.scramble(text, 3)
    n = text.size
    fold_t = wm.FOLD[text] if nocase else text
    before = b"q7_ " + bytes(text[:40]) + b" "     # a previous piece that ends in a non-word byte
    init = model.o.scan(wm.FOLD[np.frombuffer(before, np.uint8)] if nocase else before)[2]
    dense_exp = model.o.scan(wm.FOLD[dense] if nocase else dense)
    cap = dense_exp[0].size + 2   # the pass reads records up to max_records = cap - 2: stale ones only
    wsb = m.lib.acm_scan_workspace_bytes(m.dfa, n)
    keep = []

    def buf(nbytes, byte):
        b = DeviceArray(max(nbytes, 16))
        b.fill(byte)
        keep.append(b)
        return b

    try:
        assert m.set_mode(mode) == mode
        assert m.lds_resident() == lds
        ws = buf(wsb, 0xA5)
        P, Q = buf(cap * 4, 0), buf(cap * 4, 0)   # behind the stale records: state 0, a valid record too
        d_dense = DeviceArray.from_numpy(dense)
        d_text, p_text = framed(text)
        d_before, p_before = framed(before)
        keep += [d_dense, d_text, d_before]
        # stale input records: a denser scan's records, in range and valid states, stay behind this scan's trailer
        m.scan_async(d_dense, dense.size, 0, pat_plane=P, off_plane=Q, plane_capacity=cap, workspace=(ws.ptr, wsb),
                     offset_shift=ORIGIN, report=_lib.REPORT_STATE)
        ws.fill(0xFF)
        m.scan_async(p_text, n, init, pat_plane=P, off_plane=Q, plane_capacity=cap, workspace=(ws.ptr, wsb),
                     offset_shift=ORIGIN, report=_lib.REPORT_STATE)
        stale = read_cells(P, cap)
        stale_off = read_cells(Q, cap)
        full = model.o.scan(fold_t, init)
        k = full[0].size
        assert int(stale[0]) == k and int(stale[k + 1]) == full[2]
        assert dense_exp[0].size > k + 100
        behind = stale_off[k + 2:cap - 1].astype(np.int64)
        assert np.array_equal(behind, dense_exp[0][k + 1:].astype(np.int64) + ORIGIN), \
            "the dense scan's records must lie behind the trailer"
        mr = cap - 2

        # the segment pass: starts with poison behind them (a start that would split the text again)
        rng = np.random.default_rng(13)
        starts = np.sort(rng.choice(n, 300, replace=False)).astype(np.int64)
        starts = np.concatenate([starts[:150], starts[150:151], starts[150:]])   # one empty segment
        nseg = starts.size
        st_cells = np.full(nseg + 64, ORIGIN + n // 3, dtype=np.int32)
        st_cells[:nseg] = starts + ORIGIN
        d_st = DeviceArray.from_numpy(st_cells, pad_to=0)
        keep.append(d_st)
        for report in (_lib.REPORT_HEAD, _lib.REPORT_STATE):
            sws_b = m.lib.acm_segment_workspace_bytes(mr)
            sws = buf(sws_b, 0xFF if report else 0xA5)
            sp, so, sg = buf(cap * 4, EE), buf(cap * 4, EE), buf(cap * 4, EE)
            cnt = buf((nseg + 64) * 4, EE)
            m.segment_async(P, Q, mr, d_st, nseg, ORIGIN + n, sp, so, cap, seg_out=sg, seg_counts=cnt,
                            report=report, workspace=(sws.ptr, sws_b))
            eo, ep, es, ec, ef = oracle_segments(model.o, fold_t, starts, init)
            w = "%s %s segment pass %s" % (row, "nocase" if nocase else "case", "state" if report else "head")
            poison.check_planes(sp, so, cap, (eo.astype(np.int64) + ORIGIN, ep, ef), what=w, pat_cells=not report)
            k = eo.size
            g = read_cells(sg, cap)
            assert np.array_equal(g[1:1 + k], es), w + ": segment ids differ"
            assert np.all(g[k + 2:] == poison.cell(EE)), w + ": segment plane written behind the trailer"
            c = read_cells(cnt, nseg + 64)
            assert np.array_equal(c[:nseg], ec), w + ": per-segment counts differ"
            assert np.all(c[nseg:] == poison.cell(EE)), w + ": counts written past segments"
        seg_state = (sp, so)

        # the word pass: word bytes in front of d_text and d_before and past text_end (next_byte = -1)
        L = a.max_pattern_len
        wwb = m.lib.acm_word_workspace_bytes(mr)
        cases = [   # (d_before, before bytes, all patterns, with the segment pass's STATE output)
            (None, b"", False, False),
            (p_before, before, True, False),
            (p_before, before, False, True),
        ]
        for bptr, bb, ap, seg in cases:
            wws = buf(wwb, 0xA5 if ap else 0xFF)
            ocap = 8 * cap if ap else cap
            wp, wo = buf(ocap * 4, EE), buf(ocap * 4, EE)
            tail = buf(L + 16 + poison.PAST_PAD, EE)
            sp_, so_ = seg_state if seg else (P, Q)
            m.word_async(sp_, so_, mr, p_text, ORIGIN, ORIGIN + n, wp, wo, ocap, before=bptr, before_len=len(bb),
                         next_byte=-1, seg_start=d_st if seg else None, segments=nseg if seg else 0,
                         all_patterns=ap, tail_out=tail, workspace=(wws.ptr, wwb))
            eo, ep, ef = model.words(text, wm.DEFAULT, ap, init_state=init, before=bb, next_byte=-1,
                                     starts=starts if seg else None)
            if seg:
                ef = oracle_segments(model.o, fold_t, starts, init)[4]
            w = "%s %s word pass before=%d all=%s segments=%s" % (row, "nocase" if nocase else "case", len(bb), ap,
                                                                 seg)
            assert eo.size > 50 and eo[-1] == n - 1, w + ": the text must end with a word-bounded match"
            if not seg:
                assert np.any(eo.astype(np.int64) == model.lengths[ep] - 1), \
                    w + ": a word-bounded match must start at the text's first byte"
            poison.check_planes(wp, wo, ocap, (eo.astype(np.int64) + ORIGIN, ep, ef), what=w)
            tl = min(L, len(bb) + n)
            got = tail.to_numpy(np.uint8, L + 16 + poison.PAST_PAD)
            assert bytes(got[:tl]) == (bb + bytes(text))[-tl:], w + ": tail"
            assert np.all(got[tl:] == EE), w + ": tail written past its bytes"
    finally:
        for b in keep:
            b.free()
        m.close()


def case_kept(pats, hay, lo, end, offs, ids):
    """bool per (offset, pattern) entry: the pattern ignores case, or the bytes under it -- hay holds the stream
    offsets [lo, lo + len(hay)), the text ends at end -- equal it as added"""
    out = np.zeros(len(offs), dtype=bool)
    for i, (o, p) in enumerate(zip(np.asarray(offs).tolist(), np.asarray(ids).tolist())):
        pat, nocase = pats[p]
        a = o - len(pat) + 1
        out[i] = len(pat) > 0 and (nocase or (a >= lo and o < end and hay[a - lo:o + 1 - lo] == pat))
    return out


def first_per_offset(offs, ids):
    first = np.concatenate([[True], offs[1:] != offs[:-1]]) if offs.size else np.zeros(0, dtype=bool)
    return offs[first], ids[first]


def mixed_inputs(name):
    """(nocase model, (pattern, ignores case) pairs, windows, text, denser text, before) of a set with every third
    pattern ignoring case and windows on three quarters of them.  The text's letters change case now and
    then; an exact pattern lies across the seam of before and text."""
    model = wm.WordModel(name, True)          # the candidates are the nocase automaton's
    pats = [(p, i % 3 == 0) for i, p in enumerate(model.pats)]
    windows = {i: ((0, 150, False), (8, 200, True), (5, 2, False))[i % 4 - 1] for i in range(len(pats)) if i % 4}
    text = wm.planted_text(model.pats, PASS_N, 7, max_len=24)
    letter = ((text | 0x20) >= ord("a")) & ((text | 0x20) <= ord("z"))
    text[letter & (np.random.default_rng(3).random(text.size) < 0.15)] ^= 0x20
    across = next(p for p, nocase in pats if not nocase and 4 <= len(p) <= 24)
    text = np.concatenate([np.frombuffer(across[2:] + b" ", dtype=np.uint8), text])
    before = b"q7_ " + bytes(text[40:80]) + b" " + across[:2]
    short = [p for p in model.pats if 0 < len(p) <= 8] or [min((p for p in model.pats if p), key=len)]
    rng = np.random.default_rng(11)
    dense = np.frombuffer(b"".join(short[int(rng.integers(len(short)))] for _ in range(text.size // 2))[:text.size],
                          dtype=np.uint8)   # patterns back to back, as added: many more records and entries
    return model, pats, windows, text, dense, before


@pytest.mark.parametrize("row", list(test_gpu_words.ROWS))
def test_case_and_position_passes(gpu, monkeypatch, row):
    """the row's set made mixed and positioned (mixed_inputs), so that the case and position passes have
    work: both over the STATE planes of a scan that a denser scan used before it, and the position pass also
    over case-pass output that a denser call left its entries in"""
    name, mode, env, lds = test_gpu_words.ROWS[row]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, pats, windows, text, dense, before = mixed_inputs(name)
    rule = pm.Windows(pats, windows)
    a = pm.build(pats, windows)
    assert a.mixed_case and a.positioned
    m = Matcher(a, 0, max_text=16)
    n = text.size
    init = model.o.scan(wm.FOLD[np.frombuffer(before, np.uint8)])[2]
    dense_head = model.o.scan(wm.FOLD[dense])
    cap = dense_head[0].size + 2
    mr, icap = cap - 2, 8 * cap
    wsb = m.lib.acm_scan_workspace_bytes(m.dfa, n)
    cwb, pwb = m.lib.acm_case_workspace_bytes(mr), m.lib.acm_position_workspace_bytes(icap - 2)
    keep = []

    def buf(nbytes, byte):
        b = DeviceArray(max(nbytes, 16))
        b.fill(byte)
        keep.append(b)
        return b

    def cells(o, p, shift=ORIGIN):
        return o.astype(np.int64) + shift, p

    try:
        assert m.set_mode(mode) == mode
        assert m.lds_resident() == lds
        ws = buf(wsb, 0xA5)
        P, Q = buf(cap * 4, 0), buf(cap * 4, 0)
        hp, hq = buf(icap * 4, 0), buf(icap * 4, 0)
        d_dense = DeviceArray.from_numpy(dense)
        d_text, p_text = framed(text)
        d_before, p_before = framed(before)
        keep += [d_dense, d_text, d_before]
        # the denser scan and its case pass leave their records in P, Q and their entries in hp, hq
        m.scan_async(d_dense, dense.size, 0, pat_plane=P, off_plane=Q, plane_capacity=cap, workspace=(ws.ptr, wsb),
                     offset_shift=ORIGIN, report=_lib.REPORT_STATE)
        m.case_async(P, Q, mr, d_dense, ORIGIN, ORIGIN + dense.size, hp, hq, icap, all_patterns=True,
                     workspace=(buf(cwb, 0xFF).ptr, cwb))
        do, dp, _ = model.o.scan_all(wm.FOLD[dense])
        dk = case_kept(pats, bytes(dense), 0, dense.size, do, dp)
        dense_entries = int(dk.sum())
        assert int(read_cells(hp, 1)[0]) == dense_entries <= icap - 2
        ws.fill(0xFF)
        m.scan_async(p_text, n, init, pat_plane=P, off_plane=Q, plane_capacity=cap, workspace=(ws.ptr, wsb),
                     offset_shift=ORIGIN, report=_lib.REPORT_STATE)
        head = model.o.scan(wm.FOLD[text], init)
        k = head[0].size
        stale = read_cells(Q, cap)
        assert int(stale[0]) == k and dense_head[0].size > k + 100
        assert np.array_equal(stale[k + 2:cap - 1].astype(np.int64), dense_head[0][k + 1:].astype(np.int64) + ORIGIN), \
            "the dense scan's records must lie behind the trailer"
        last = head[2]
        eo, ep, _ = model.o.scan_all(wm.FOLD[text], init)
        eo = eo.astype(np.int64)
        hay = before + bytes(text)
        tag = row + " "

        # the case pass, all patterns, with before; then the first kept entry per record, without
        kept = case_kept(pats, hay, -len(before), n, eo, ep)
        assert 50 < int(kept.sum()) < eo.size and kept[eo < 20].any()
        cp, cq = buf(icap * 4, EE), buf(icap * 4, EE)
        m.case_async(P, Q, mr, p_text, ORIGIN, ORIGIN + n, cp, cq, icap, before=p_before, before_len=len(before),
                     all_patterns=True, workspace=(buf(cwb, 0xA5).ptr, cwb))
        poison.check_planes(cp, cq, icap, cells(eo[kept], ep[kept]) + (last,), what=tag + "case pass, all, before")
        alone = case_kept(pats, bytes(text), 0, n, eo, ep)
        assert int(alone.sum()) < int(kept.sum())          # an entry reached into before
        fp, fq = buf(cap * 4, EE), buf(cap * 4, EE)
        m.case_async(P, Q, mr, p_text, ORIGIN, ORIGIN + n, fp, fq, cap, all_patterns=False,
                     workspace=(buf(cwb, 0xFF).ptr, cwb))
        poison.check_planes(fp, fq, cap, cells(*first_per_offset(eo[alone], ep[alone])) + (last,),
                            what=tag + "case pass, first, no before")

        # the position pass over the STATE planes: texts from the starts, the last one's end unknown
        rng = np.random.default_rng(13)
        starts = np.sort(rng.choice(n, 300, replace=False)).astype(np.int64)
        starts = np.concatenate([starts[:150], starts[150:151], starts[150:]])   # one empty text
        nseg = starts.size
        st_cells = np.full(nseg + 64, ORIGIN + n // 3, dtype=np.int32)
        st_cells[:nseg] = starts + ORIGIN
        d_st = DeviceArray.from_numpy(st_cells, pad_to=0)
        keep.append(d_st)
        lead = ORIGIN - len(before)
        xp, xo, und = rule.entries(ep, eo + ORIGIN, True, starts + ORIGIN, lead, ORIGIN + n, None)
        assert 50 < xp.size < eo.size and und > 0
        pp, pq, info = buf(icap * 4, EE), buf(icap * 4, EE), buf(64, EE)
        m.position_async(P, Q, mr, pp, pq, icap, info, report=_lib.REPORT_STATE, seg_start=d_st, segments=nseg,
                         lead_begin=lead, text_end=ORIGIN + n, open_end=-1, all_patterns=True,
                         workspace=(buf(pwb, 0xA5).ptr, pwb))
        poison.check_planes(pp, pq, icap, (xo, xp, last), what=tag + "position pass over states")
        assert read_cells(info, 16).tolist() == [und, 0, 0, 0] + [poison.cell(EE)] * 12, tag + "info"

        # the position pass over case-pass output with the denser call's entries behind the trailer
        m.case_async(P, Q, mr, p_text, ORIGIN, ORIGIN + n, hp, hq, icap, before=p_before, before_len=len(before),
                     all_patterns=True, workspace=(buf(cwb, 0xA5).ptr, cwb))
        e = int(kept.sum())
        assert dense_entries > e + 100
        got_p, got_q = read_cells(hp, icap), read_cells(hq, icap)
        assert got_p[0] == e and np.array_equal(got_p[1:1 + e], ep[kept]) and got_p[e + 1] == last
        assert np.array_equal(got_q[1:1 + e], eo[kept] + ORIGIN)
        assert np.array_equal(got_q[e + 2:dense_entries + 1], do[dk][e + 1:].astype(np.int64) + ORIGIN), \
            "the dense call's entries must lie behind the trailer"
        xp, xo, und = rule.entries(ep[kept], eo[kept] + ORIGIN, False, (), lead, ORIGIN + n, ORIGIN + n)
        assert 50 < xp.size < e and und == 0
        pp, pq, info = buf(icap * 4, EE), buf(icap * 4, EE), buf(64, EE)
        m.position_async(hp, hq, icap - 2, pp, pq, icap, info, report=_lib.REPORT_HEAD, lead_begin=lead,
                         text_end=ORIGIN + n, open_end=ORIGIN + n, all_patterns=False,
                         workspace=(buf(pwb, 0xFF).ptr, pwb))
        poison.check_planes(pp, pq, icap, (xo, xp, last), what=tag + "position pass over case output")
        assert read_cells(info, 16).tolist() == [0, 0, 0, 0] + [poison.cell(EE)] * 12, tag + "info"
    finally:
        for b in keep:
            b.free()
        m.close()
        a.close()


# ---------------------------------------------------------------------------------------------- D
GREP_B, GREP_G = 256, 64


def replay_text_mode(data, B, G):
    """acm_grep's fill_text for one file and one worker: per round the list of chunks (the lines as fgets
    returns them) and whether they lie packed (each chunk at a 16-byte multiple of the sum before it)"""
    size = B * G
    rounds, at = [], 0
    chunks, used = [], 0
    while at < len(data):
        room = min(size - used, B)
        if room < 2 or len(chunks) >= G:
            rounds.append(chunks)
            chunks, used = [], 0
            continue
        nl = data.find(b"\n", at, at + room - 1)
        end = nl + 1 if nl >= 0 else min(len(data), at + room - 1)
        chunks.append(data[at:end])
        used += min((end - at + 15) & ~15, size - used)
        at = end
        if len(chunks) >= G or used + 2 > size:
            rounds.append(chunks)
            chunks, used = [], 0
    if chunks:
        rounds.append(chunks)
    return rounds


def stale_layout_file(tmp_path):
    """two full rounds of long lines and a short third round on the first buffer again: its stream ends
    with ' attack', and round 1's bytes at that place go on with 's' ('attacks' is a pattern too)"""
    words = open(os.path.join(orc.DATA, "sentiment", "top5000_words.txt")).read().split()
    rng = np.random.default_rng(5)

    def line(k):
        out = b""
        while len(out) < k:
            out += words[int(rng.integers(len(words)))].encode() + b" "
        return out[:k].replace(b"\n", b" ") + b"\n"

    third = [line(int(rng.integers(20, 60))) for _ in range(6)] + [b"the end of an attack"]
    len3 = sum(len(x) for x in third)
    first = [line(int(rng.integers(150, 200))) for _ in range(GREP_G)]
    s1 = bytearray(b"".join(first))
    assert b"\n" not in s1[len3 - 7:len3 + 2]
    s1[len3 - 6:len3 + 1] = b"attacks"
    second = [line(int(rng.integers(150, 200))) for _ in range(GREP_G)]
    data = bytes(s1) + b"".join(second) + b"".join(third)
    p = tmp_path / "stale.txt"
    p.write_bytes(data)
    return str(p), data, len3


@pytest.mark.parametrize("flags", [[], ["-W"], ["-S"]], ids=["plain", "W", "S"])
def test_grep_stale_packed(gpu, tmp_path, flags):
    path, data, len3 = stale_layout_file(tmp_path)
    rounds = replay_text_mode(data, GREP_B, GREP_G)
    streams = [b"".join(r) for r in rounds]
    assert len(rounds) == 3 and len(rounds[0]) == len(rounds[1]) == GREP_G
    assert len(streams[2]) == len3 < len(streams[0])            # round 3 fills buffer A again, shorter
    assert any(len(c) % 16 for c in rounds[2])                  # not packed: the scan reads d_packed
    assert streams[2].endswith(b" attack") and streams[0][len3 - 6:len3 + 1] == b"attacks"
    o = fixtures.oracle_for("sentiment")
    s3 = np.frombuffer(streams[2], dtype=np.uint8)
    over = np.frombuffer(streams[2] + streams[0][len3:len3 + 16], dtype=np.uint8)
    assert o.scan(over)[0].size > o.scan(s3)[0].size            # reading round 1's bytes adds a match
    assert o.scan(np.frombuffer(streams[0], np.uint8))[0].size > 3 * o.scan(s3)[0].size   # round 1 denser
    stream = np.frombuffer(data, dtype=np.uint8)
    if "-W" in flags:
        exp = wm.WordModel("sentiment").words(stream)[0].size
    elif "-S" in flags:
        starts = np.concatenate([[0], np.flatnonzero(stream == ord("\n")) + 1])
        exp = oracle_segments(o, stream, starts[starts < stream.size])[0].size
    else:
        exp = o.scan(stream)[0].size
    pat_path = os.path.join(orc.DATA, "sentiment", "patterns_categorical.txt")
    hits, stats, _ = run(CLI, ["-f", path, "-p", pat_path, "-t", "-B", str(GREP_B), "-D", "0", "-G", str(GREP_G),
                               "-L", "1024", "-w", "1", "-R", "64", "-v"] + flags)
    assert int(stats["Kernel launches"]) == 3
    assert int(stats["Matches"]) == exp
    last = [h[1] for h in hits if h[1] in ("attack", "attacks")]
    assert last and last[-1] == "attack"     # the stream's last match, not round 1's 'attacks'
