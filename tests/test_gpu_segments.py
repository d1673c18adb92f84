"""Segmented scans on the device (acm_segment_matches_async, Matcher.scan_segments): bit for bit the
concatenation of the oracle's scans of every segment alone from state 0 -- offsets, patterns, segment
ids, per-segment counts and the final state -- behind every pipeline."""
import numpy as np
import pytest

import fixtures
from gpu_pattern_matching_amd import AcmError, Automaton, DeviceArray, Matcher, _lib
from test_host_segments import oracle_segments, random_starts

pytestmark = pytest.mark.gpu

MiB = 1 << 20


def matcher(name, max_text, nocase=False, patterns=None):
    a = Automaton(nocase=nocase)
    if patterns is not None:
        for p in patterns:
            a.add(p)
    else:
        path, hx, max_len = fixtures.set_source(name)
        a.load_file(path, hx, max_len)
    a.compile()
    m = Matcher(a, 0, max_text=max_text)
    return m, a


def words_text(n, seed):
    return fixtures.text_for({"kind": "words", "n": n, "seed": seed}, [])


def clamav_text(n, seed):
    pats = fixtures.patterns_of("clamav2000")
    return fixtures.text_for({"kind": "clamav", "n": n, "seed": seed, "n_plant": max(4, n // 2048)}, pats)


def planted(name, n, seed, seg_mean):
    """n bytes cut into segments of about seg_mean bytes, with a pattern of the set planted across every
    boundary (its first part ends one segment, the rest begins the next)"""
    pats = [p for p in fixtures.patterns_of(name) if len(p) >= 2]
    rng = np.random.default_rng(seed)
    base = clamav_text(n, seed) if name.startswith("clamav") else words_text(n, seed)
    out, x = [], 0
    while x < n:
        size = int(rng.integers(1, 2 * seg_mean))
        piece = base[x:x + size]
        x += size
        p = pats[int(rng.integers(0, len(pats)))]
        cut = int(rng.integers(1, len(p)))
        out.append(bytes(piece) + p[:cut])
        out.append(p[cut:])
    # a segment is the tail of one planted pattern, a piece of text and the head of the next
    starts, pos = [0], 0
    for i, q in enumerate(out):
        if i % 2 == 1:
            starts.append(pos)
        pos += len(q)
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy(), np.array(starts, dtype=np.int32)


def assert_same(got, exp, counts=True):
    assert got[0].size == exp[0].size, "record count %d != %d" % (got[0].size, exp[0].size)
    assert np.array_equal(got[0], exp[0]), "offsets differ"
    assert np.array_equal(got[1], exp[1]), "pattern indices differ"
    assert np.array_equal(got[2], exp[2]), "segment ids differ"
    assert got[3] == exp[4], "final state %d != %d" % (got[3], exp[4])
    if counts:
        assert np.array_equal(got[4], exp[3]), "per-segment counts differ"


@pytest.mark.parametrize("name,mode", [("clamav2000", "sparse"), ("clamav2000", "chain"), ("clamav2000", "auto"),
                                       ("sentiment", "chain"), ("sentiment", "auto"), ("tests", "auto")])
def test_pipelines(gpu, name, mode):
    m, a = matcher(name, 4 * MiB)
    assert m.set_mode(mode) == mode
    if name == "sentiment":
        assert m.lds_resident()
    o = fixtures.oracle_for(name)
    text, starts = planted(name, 3 * MiB // 2, 11, 300)
    got = m.scan_segments((text, starts), counts=True)
    exp = oracle_segments(o, text, starts)
    assert exp[0].size > 300
    assert_same(got, exp)
    assert m.scan(text)[0].size > exp[0].size   # the planted patterns straddle the boundaries
    if mode == "sparse":
        assert m.path_taken(text.size) == "sparse"
    # the same with random segment shapes: empty ones, one byte, shorter than the longest pattern
    starts = random_starts(text.size, np.random.default_rng(5), a.max_pattern_len)
    assert_same(m.scan_segments((text, starts), counts=True), oracle_segments(o, text, starts))
    m.close()


def test_list_of_texts(gpu):
    m, _ = matcher("sentiment", MiB)
    o = fixtures.oracle_for("sentiment")
    text = words_text(20000, 3)
    texts = [bytes(text[i:i + 140]) for i in range(0, text.size, 140)] + [b"", b"x"]
    got = m.scan_segments(texts, counts=True)
    t, starts = Matcher.pack_segments(texts)
    assert_same(got, oracle_segments(o, t, starts))
    m.close()


@pytest.mark.parametrize("patterns,head", [((b"abcd", b"cd"), 1), ((b"abcd", b"bcd", b"cd"), 2)])
def test_clamping_changes_the_head(gpu, patterns, head):
    m, _ = matcher(None, 4096, patterns=patterns)
    texts = [b"xxab", b"cdxx"]
    got = m.scan_segments(texts, counts=True)
    assert got[0].tolist() == [5] and got[1].tolist() == [head] and got[2].tolist() == [1]
    assert got[4].tolist() == [0, 1]
    plain = m.scan(b"xxabcdxx")
    assert plain[0].tolist() == [5]
    m.close()


@pytest.mark.parametrize("name", ["sentiment", "clamav2000"])
def test_all_patterns(gpu, name):
    m, _ = matcher(name, 2 * MiB)
    o = fixtures.oracle_for(name)
    text, starts = planted(name, MiB, 21, 200)
    got = m.scan_segments((text, starts), all_patterns=True, counts=True)
    assert_same(got, oracle_segments(o, text, starts, all_patterns=True))
    m.close()


def test_nocase(gpu):
    from test_host_nocase import fold, folded_oracle, scramble
    m, _ = matcher("sentiment", 2 * MiB, nocase=True)
    o = folded_oracle("sentiment")
    text, starts = planted("sentiment", MiB, 31, 140)
    text = scramble(text, 4)
    got = m.scan_segments((text, starts), counts=True)
    assert_same(got, oracle_segments(o, fold(text), starts))
    m.close()


def segment_planes(m, max_records, starts, text_end, cap, report=_lib.REPORT_HEAD, planes=None):
    """segment pass over the matcher's planes into fresh ones -> (count, pat cells, off cells, seg cells,
    counts, the output planes)"""
    nseg = len(starts)
    d_st = DeviceArray.from_numpy(np.asarray(starts, dtype=np.int32), pad_to=0) if nseg else None
    pat, off, seg, cnt = DeviceArray(cap * 4), DeviceArray(cap * 4), DeviceArray(cap * 4), DeviceArray(max(nseg, 1) * 4)
    src = planes if planes is not None else (m.pat_plane, m.off_plane)
    m.segment_async(src[0], src[1], max_records, d_st, nseg, text_end, pat, off, cap, seg_out=seg,
                    seg_counts=cnt if nseg else None, report=report)
    full = int(pat.to_numpy(np.int32, 1)[0])
    cells = min(full + 2, cap)
    res = (full, pat.to_numpy(np.int32, cells), off.to_numpy(np.int32, cells), seg.to_numpy(np.int32, cells),
           cnt.to_numpy(np.int32, nseg))
    return res, (pat, off, seg, cnt, d_st)


def test_carry_through_the_init_plane(gpu):
    """two scans with a segment spanning the cut, the second starting from the segment output's trailer
    (acm_scan_batch.d_init_plane): the records equal those of one scan"""
    name = "clamav2000"
    m, _ = matcher(name, 2 * MiB)
    o = fixtures.oracle_for(name)
    text, starts = planted(name, MiB, 41, 500)
    exp = oracle_segments(o, text, starts)
    # cut one byte before the end of a match that lies inside its segment, past the middle of the text
    r = int(np.flatnonzero((exp[0] > 600000) & (exp[0].astype(np.int64) >= starts[exp[2]].astype(np.int64) + 2))[0])
    k = int(exp[2][r]) + 1
    cut = int(exp[0][r])   # the match's last byte is the first byte of the second scan
    cap = m.plane_capacity
    d1 = DeviceArray.from_numpy(text[:cut])
    m.scan_async(d1, cut, report=_lib.REPORT_STATE)
    r1, keep1 = segment_planes(m, cap - 2, starts[:k], cut, cap, report=_lib.REPORT_HEAD)
    d2 = DeviceArray.from_numpy(text[cut:])
    st2 = starts[k:] - cut
    ws = (m.ws.ptr, m.ws_bytes)
    b = m.make_batch(d2, text.size - cut, m.stream, m.pat_plane, m.off_plane, cap, ws, report=_lib.REPORT_STATE,
                     init_plane=keep1[0], init_plane_capacity=cap)
    m.enqueue(b)
    r2, keep2 = segment_planes(m, cap - 2, st2, text.size - cut, cap)
    n1, n2 = r1[0], r2[0]
    offs = np.concatenate([r1[2][1:1 + n1], r2[2][1:1 + n2] + cut]).astype(np.uint32)
    pats = np.concatenate([r1[1][1:1 + n1], r2[1][1:1 + n2]])
    seg2 = r2[3][1:1 + n2]
    segs = np.concatenate([r1[3][1:1 + n1], np.where(seg2 < 0, k - 1, seg2 + k)]).astype(np.int32)
    assert np.any(seg2 < 0), "no record continues the segment across the cut"
    assert np.array_equal(offs, exp[0]) and np.array_equal(pats, exp[1]) and np.array_equal(segs, exp[2])
    assert int(r2[1][n2 + 1]) == exp[4]
    m.close()


def test_shard_with_offset_shift(gpu):
    name = "clamav2000"
    m, a = matcher(name, 2 * MiB)
    o = fixtures.oracle_for(name)
    text, starts = planted(name, MiB, 51, 700)
    exp = oracle_segments(o, text, starts)
    halo = a.max_pattern_len - 1
    load_begin = 262144
    begin, end = load_begin + halo, 700001
    d = DeviceArray.from_numpy(text)
    cap = m.plane_capacity
    m.scan_async(d.ptr + load_begin, end - load_begin, halo=halo, offset_shift=load_begin, report=_lib.REPORT_STATE)
    r, _ = segment_planes(m, cap - 2, starts, end, cap)
    n = r[0]
    sel = (exp[0] >= begin) & (exp[0] < end)
    assert n == int(sel.sum()) > 0
    assert np.array_equal(r[2][1:1 + n].astype(np.uint32), exp[0][sel])
    assert np.array_equal(r[1][1:1 + n], exp[1][sel])
    assert np.array_equal(r[3][1:1 + n], exp[2][sel])
    # the trailer: the per-segment state at the shard's end
    last = oracle_segments(o, text[:end], starts[starts <= end])[4]
    assert int(r[1][n + 1]) == last
    m.close()


def test_zero_segments_is_the_plain_scan(gpu):
    m, _ = matcher("clamav2000", 2 * MiB)
    text = clamav_text(MiB + 3, 61)
    plain = m.scan(text)
    got = m.scan_segments((text, np.zeros(0, dtype=np.int32)))
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and got[3] == plain[2]
    assert np.all(got[2] == -1)
    m.close()


def test_overflow_follows_the_scan_contract(gpu):
    name = "sentiment"
    m, _ = matcher(name, MiB)
    o = fixtures.oracle_for(name)
    text, starts = planted(name, 200000, 71, 140)
    exp = oracle_segments(o, text, starts)
    d = DeviceArray.from_numpy(text)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    cap = 10
    r, _ = segment_planes(m, m.plane_capacity - 2, starts, text.size, cap)
    assert r[0] == exp[0].size > cap
    assert np.array_equal(r[2][1:cap - 1].astype(np.uint32), exp[0][:cap - 2])
    assert np.array_equal(r[1][1:cap - 1], exp[1][:cap - 2])
    assert int(r[1][cap - 1]) == exp[4] and int(r[2][cap - 1]) == exp[4]
    assert np.array_equal(r[4], exp[3])
    m.close()


def test_argument_errors(gpu):
    m, _ = matcher("tests", 4096)
    buf = DeviceArray(4096)
    ws = m.lib.acm_segment_workspace_bytes(100)
    for args in [dict(out_capacity=1), dict(segments=3, seg_start=None), dict(report=7), dict(ws_bytes=ws - 1)]:
        a = dict(out_capacity=100, segments=0, seg_start=None, report=0, ws_bytes=ws)
        a.update(args)
        rc = m.lib.acm_segment_matches_async(m.dfa, buf.ptr, buf.ptr, 100, a["seg_start"], a["segments"], 100,
                                             a["report"], buf.ptr, buf.ptr, None, a["out_capacity"], None, buf.ptr,
                                             a["ws_bytes"], None)
        assert rc == -1, args
    with pytest.raises(AcmError):
        m.segment_async(buf, buf, 100, None, 2, 100, buf, buf, 100)
    m.close()


@pytest.mark.parametrize("name,seg", [("sentiment", 140), ("clamav2000", 4096)])
def test_full_size(gpu, name, seg):
    n = 32 * MiB
    m, _ = matcher(name, n)
    o = fixtures.oracle_for(name)
    text = words_text(n, 81) if name == "sentiment" else clamav_text(n, 81)
    starts = np.arange(0, n, seg, dtype=np.int32)
    got = m.scan_segments((text, starts), counts=True)
    exp = oracle_segments(o, text, starts)
    assert_same(got, exp)
    m.close()
