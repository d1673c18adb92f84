"""What line extraction costs: acm_line_context_async and acm_extract_async per 32 MiB batch of line-structured text
(sentiment words, a newline for every 20th space: lines of about 114 bytes), one JSON line per case:

  every_line        every line its own range: acm_line_select_async's planes, unmerged; the output equals the text
  one_in_100_C0     1 line in 100 holds a record; the context pass with no context, then the extract
  one_in_100_C2     the same records with two lines of context either side (glue "--\\n")
  only_matching     a 6-byte match in each of those lines: (start, offset) planes, ACM_EXTRACT_END_INCLUSIVE

Beside each case, in the same run and alternating with it: a device-to-device copy of the m output bytes, for
every_line acm_rewrite_async over the same text with zero records (the same output), and the host path -- the text
and the planes copied back (timed alone: what the device path saves before any slicing) and the slices joined with
numpy.  Device events around each run, median, minimum and maximum over the repeats.

python tools/extract_bench.py [--seconds 0.5] >> profiles/extract_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import extract_model as xm
import line_model as lm
import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib

N = 32 << 20


def lined_text(seed):
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    t = synth.word_corpus(N, seed, words).copy()
    sp = np.flatnonzero(t == 0x20)
    rng = np.random.default_rng(seed)
    t[sp[rng.random(sp.size) < 0.05]] = 0x0A
    t[-1] = 0x0A
    return t


def stats(ms):
    a = np.asarray(ms) * 1e3
    return {"median_us": round(float(np.median(a)), 1), "min_us": round(float(a.min()), 1), "max_us": round(float(a.max()), 1),
            "runs": int(a.size)}


def timed(runs, seconds):
    """every callable of runs in turn, alternating, until each has had `seconds` of device time and 20 runs"""
    for f in runs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or min(len(v) for v in t.values()) < 20:
        for key, f in runs.items():
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    return {k: stats(v) for k, v in t.items()}


def host_path(d_text, n, planes, k, incl, seconds_out):
    """the text and the planes copied back, then the ranges sliced and joined on the host; (copy us, slice us, bytes)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    text = d_text.to_numpy(np.uint8, n)
    b = planes[0].to_numpy(np.int32, k + 1)[1:]
    e = planes[1].to_numpy(np.int32, k + 1)[1:]
    t1 = time.perf_counter()
    e = e + 1 if incl else e
    out = np.concatenate([text[x:y] for x, y in zip(b.tolist(), e.tolist())]) if k else np.zeros(0, dtype=np.uint8)
    t2 = time.perf_counter()
    return round((t1 - t0) * 1e6, 1), round((t2 - t1) * 1e6, 1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    a = Automaton()
    a.add(b"\x00never\x00", 0)
    a.compile()
    m = Matcher(a, 0, max_text=N)
    a.close()
    lib = m.lib
    t = lined_text(21)
    _, e_info, e_st = lm.index(t)
    lines = int(e_st.size)
    lcap = lines + 1
    d = DeviceArray.from_numpy(t)
    copy_dst = DeviceArray(N + 4096)
    starts, linfo = DeviceArray(lcap * 4), DeviceArray(32)
    nb_ix = lib.acm_line_index_workspace_bytes(N)
    ws_ix = DeviceArray(nb_ix)
    m.line_index_async(d, N, starts, lcap, linfo, workspace=(ws_ix.ptr, nb_ix))
    rel, beg, nxt, cnt = (DeviceArray((lcap + 2) * 4) for _ in range(4))
    cinfo, xinfo = DeviceArray(16), DeviceArray(32)
    nb_ctx = lib.acm_line_context_workspace_bytes(lcap, 0)
    nb_sel = lib.acm_line_select_workspace_bytes(lcap)
    ws_ctx = DeviceArray(max(nb_ctx, nb_sel))
    out = DeviceArray(N + 4096)
    common = {"tool": "extract_bench", "batch_bytes": N, "lines": lines, "tile_bytes": 16384}

    def d2d(nbytes):
        return lambda: _lib.check(lib.acm_rt_memcpy_d2d(copy_dst.ptr, d.ptr, nbytes, m.stream), "acm_rt_memcpy_d2d")

    def figures():
        r = xinfo.to_numpy(np.int32, 8)
        return r, (int(np.uint32(r[3])) << 32) | int(np.uint32(r[2]))

    def check_against_host(planes, k, incl, mlen, glue, case):
        copy_us, slice_us, host_out = host_path(d, N, planes, k, incl, None)
        if not glue:            # (the host slices carry no glue and no terminators: compared where there are none)
            assert mlen == host_out.size and np.array_equal(out.to_numpy(np.uint8, mlen), host_out), case
        return {"host_copy_back_us": copy_us, "host_slice_us": slice_us}

    # ---- (a) every line its own range
    none = DeviceArray.from_numpy(np.zeros(2, dtype=np.int32), pad_to=0)
    m.line_select_async(starts, lcap, linfo, 0, N, none, 0, rel, beg, nxt, lcap + 2, invert=True, workspace=(ws_ctx.ptr, nb_sel))
    k = int(beg.to_numpy(np.int32, 1)[0])
    assert k == lines
    nb_ex = lib.acm_extract_workspace_bytes(k, 0)
    ws_ex = DeviceArray(nb_ex)

    def extract_lines():
        m.extract_async(d, N, beg, nxt, k, out, N + 4096, xinfo, terminator=0x0A, workspace=(ws_ex.ptr, nb_ex))

    nb_rw = lib.acm_rewrite_workspace_bytes(4096, 0)
    ws_rw, rw_info = DeviceArray(nb_rw), DeviceArray(32)

    def rewrite_nothing():
        m.rewrite_async(d, N, none, none, 4096, out, N + 4096, rw_info, workspace=(ws_rw.ptr, nb_rw))

    extract_lines()
    info, mlen = figures()
    assert mlen == N and np.array_equal(out.to_numpy(np.uint8, N), t)
    row = dict(common, case="every_line", ranges=k, output_bytes=mlen)
    row.update(timed({"extract": extract_lines, "rewrite_zero_records": rewrite_nothing, "d2d_copy": d2d(mlen)}, args.seconds))
    row.update(check_against_host((beg, nxt), k, False, mlen, b"", "every_line"))
    rw = row["rewrite_zero_records"]
    row["extract_over_rewrite"] = round(row["extract"]["median_us"] / rw["median_us"], 2)
    row["extract_minus_rewrite_us"] = round(row["extract"]["median_us"] - rw["median_us"], 1)
    row["rewrite_spread_us"] = round(rw["max_us"] - rw["min_us"], 1)
    row["extract_GBps_in_plus_out"] = round(2 * mlen / row["extract"]["median_us"] / 1e3, 1)
    print(json.dumps(row), flush=True)

    # ---- (b) 1 line in 100, without and with context
    picked = e_st[::100]
    picked = picked[picked + 9 < N]
    offs = DeviceArray.from_numpy(xm.plane_of(picked + 3), pad_to=0)
    for before, after, glue, case in ((0, 0, b"", "one_in_100_C0"), (2, 2, b"--\n", "one_in_100_C2")):
        def context():
            m.line_context_async(starts, lcap, linfo, 0, N, offs, picked.size, rel, beg, nxt, lcap + 2, cinfo, before=before,
                                 after=after, lines_out=cnt, workspace=(ws_ctx.ptr, nb_ctx))

        def extract():
            m.extract_async(d, N, beg, nxt, lcap, out, N + 4096, xinfo, glue=glue, terminator=0x0A, workspace=(ws_big.ptr, nb_big))

        nb_big = lib.acm_extract_workspace_bytes(lcap, 0)
        ws_big = DeviceArray(nb_big)
        context()
        extract()
        info, mlen = figures()
        groups = int(beg.to_numpy(np.int32, 1)[0])
        exp_groups, exp_ctx = xm.context(e_st, e_info, 0, N, picked + 3, False, before, after)
        assert groups == len(exp_groups[0]) and cinfo.to_numpy(np.int32, 4).tolist() == exp_ctx.tolist()
        row = dict(common, case=case, ranges=groups, output_bytes=mlen, kept_lines=int(exp_ctx[1]))
        row.update(timed({"context": context, "extract": extract, "context_and_extract": lambda: (context(), extract()),
                          "d2d_copy": d2d(mlen)}, args.seconds))
        # the host path reads the text and the records: the copy-back alone is what the device path is held against
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.to_numpy(np.uint8, N)
        offs.to_numpy(np.int32, picked.size + 1)
        row["host_copy_back_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        row.update({"host_slice_us": check_against_host((beg, nxt), groups, False, mlen, glue, case)["host_slice_us"]})
        row["device_under_host_copy_back"] = bool(row["context_and_extract"]["max_us"] < row["host_copy_back_us"])
        print(json.dumps(row), flush=True)
        ws_big.free()

    # ---- (c) the matches themselves
    sp = DeviceArray.from_numpy(xm.plane_of(picked + 3), pad_to=0)
    op = DeviceArray.from_numpy(xm.plane_of(picked + 8), pad_to=0)
    nb_o = lib.acm_extract_workspace_bytes(picked.size, 0)
    ws_o = DeviceArray(nb_o)

    def only_matching():
        m.extract_async(d, N, sp, op, picked.size, out, N + 4096, xinfo, end_inclusive=True, terminator=-1,
                        workspace=(ws_o.ptr, nb_o))

    only_matching()
    info, mlen = figures()
    row = dict(common, case="only_matching", ranges=int(info[0]), output_bytes=mlen)
    row.update(timed({"extract": only_matching, "d2d_copy": d2d(max(mlen, 1))}, args.seconds))
    row.update(check_against_host((sp, op), picked.size, True, mlen, b"", "only_matching"))
    print(json.dumps(row), flush=True)
    m.close()


if __name__ == "__main__":
    main()
