"""What line prefixes cost: acm_line_context_lines_async and acm_format_async per 32 MiB batch of line-structured text
(tools/extract_bench.py's: sentiment words, a newline for every 20th space: lines of about 114 bytes), one JSON line
per case:

  every_line        every line its own range, with name:line:offset: in front; beside it, in the same run and
                    alternating with it, acm_extract_async over the same ranges
  one_in_100_C2     1 line in 100 holds a record, two lines of context either side, glue "--\\n": the per-line context
                    pass and the format pass; beside them the group-form context pass and the extract
  only_matching     a 6-byte match in each of those lines with name:line:offset: in front (the line numbers from
                    acm_line_number_async over the starts, timed with it)

Each case is also held against the host path: the text and the planes copied back (timed alone: what the device path
saves before any formatting), then the lines formatted in Python.  Device events around each run, median, minimum and
maximum over the repeats.

python tools/format_bench.py [--seconds 0.5] [--out profiles/format_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import format_model as fm
import line_model as lm
from extract_bench import N, lined_text, timed
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher

NAME = b"corpus/sentiment.txt"


def host_format(text, begins, ends, kinds, nums, glue):
    """the lines formatted on the host as the model does it, joined once"""
    parts, prev = [], False
    for b, e, k, n in zip(begins.tolist(), ends.tolist(), kinds.tolist(), nums.tolist()):
        sep = b":" if k & 1 else b"-"
        if k & 2 and prev:
            parts.append(glue)
        parts.append(NAME + sep + b"%d" % (n + 1) + sep + b"%d" % b + sep)
        parts.append(text[b:e])
        prev = True
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "format_bench.jsonl"))
    args = ap.parse_args()
    a = Automaton()
    a.add(b"\x00never\x00", 0)
    a.compile()
    m = Matcher(a, 0, max_text=N)
    a.close()
    lib = m.lib
    t = lined_text(21)
    tb = t.tobytes()
    _, e_info, e_st = lm.index(t)
    lines = int(e_st.size)
    lcap = lines + 1
    d = DeviceArray.from_numpy(t)
    starts, linfo = DeviceArray(lcap * 4), DeviceArray(32)
    nb_ix = lib.acm_line_index_workspace_bytes(N)
    ws_ix = DeviceArray(nb_ix)
    m.line_index_async(d, N, starts, lcap, linfo, workspace=(ws_ix.ptr, nb_ix))
    rel, beg, nxt, kind, cnt = (DeviceArray((lcap + 2) * 4) for _ in range(5))
    g_rel, g_beg, g_nxt = (DeviceArray((lcap + 2) * 4) for _ in range(3))
    cinfo, xinfo = DeviceArray(16), DeviceArray(32)
    nb_ctx = max(lib.acm_line_context_lines_workspace_bytes(lcap, 0), lib.acm_line_context_workspace_bytes(lcap, 0),
                 lib.acm_line_select_workspace_bytes(lcap))
    ws_ctx = DeviceArray(nb_ctx)
    cap = 2 * N
    out = DeviceArray(cap + 4096)
    names, name_off = fm.name_table([NAME], 0)
    d_names = DeviceArray.from_numpy(np.frombuffer(names, dtype=np.uint8))
    d_name_off = DeviceArray.from_numpy(name_off, pad_to=0)
    nb_fm = max(lib.acm_format_workspace_bytes(lcap, 0), lib.acm_extract_workspace_bytes(lcap, 0))
    ws_fm = DeviceArray(nb_fm)
    common = {"tool": "format_bench", "batch_bytes": N, "lines": lines, "tile_bytes": 16384, "name_bytes": len(NAME)}
    prefix = dict(number=True, offset=True, names=d_names, name_off=d_name_off, names_bytes=len(names))
    rows = []

    def figures():
        r = xinfo.to_numpy(np.int32, 8)
        return r, (int(np.uint32(r[3])) << 32) | int(np.uint32(r[2]))

    def host_path(planes, k, glue, mlen, incl=False):
        """(copy-back us, format us): the text and the planes copied back, then formatted on the host; the device's
        output is compared with it"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.to_numpy(np.uint8, N)
        cols = [p.to_numpy(np.int32, k + 1)[1:] for p in planes]
        t1 = time.perf_counter()
        kinds = cols[3] if len(cols) > 3 else np.ones(k, dtype=np.int32)
        exp = host_format(tb, cols[0], cols[1] + (1 if incl else 0), kinds, cols[2], glue)
        t2 = time.perf_counter()
        assert mlen == len(exp) and out.to_numpy(np.uint8, mlen).tobytes() == exp
        return round((t1 - t0) * 1e6, 1), round((t2 - t1) * 1e6, 1)

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- (a) every line its own range
    none = DeviceArray.from_numpy(np.zeros(2, dtype=np.int32), pad_to=0)
    m.line_select_async(starts, lcap, linfo, 0, N, none, 0, rel, beg, nxt, lcap + 2, invert=True,
                        workspace=(ws_ctx.ptr, lib.acm_line_select_workspace_bytes(lcap)))
    k = int(beg.to_numpy(np.int32, 1)[0])
    assert k == lines

    def format_lines():
        m.format_async(d, N, beg, nxt, k, out, cap, xinfo, num_plane=rel, terminator=0x0A, workspace=(ws_fm.ptr, nb_fm), **prefix)

    def extract_lines():
        m.extract_async(d, N, beg, nxt, k, out, cap, xinfo, terminator=0x0A, workspace=(ws_fm.ptr, nb_fm))

    extract_lines()
    _, plain_len = figures()
    format_lines()
    _, mlen = figures()
    row = dict(common, case="every_line", ranges=k, output_bytes=mlen, extract_output_bytes=plain_len)
    row.update(timed({"format": format_lines, "extract": extract_lines}, args.seconds))
    format_lines()
    row["host_copy_back_us"], row["host_format_us"] = host_path((beg, nxt, rel), k, b"", mlen)
    row["format_over_extract"] = round(row["format"]["median_us"] / row["extract"]["median_us"], 2)
    row["output_over_extract_output"] = round(mlen / plain_len, 2)
    row["format_GBps_in_plus_out"] = round((N + mlen) / row["format"]["median_us"] / 1e3, 1)
    emit(row)

    # ---- (b) 1 line in 100 with two lines of context
    picked = e_st[::100]
    picked = picked[picked + 9 < N]
    offs = DeviceArray.from_numpy(fm.plane_of(picked + 3), pad_to=0)
    glue = b"--\n"

    def context_lines():
        m.line_context_lines_async(starts, lcap, linfo, 0, N, offs, picked.size, rel, beg, nxt, kind, lcap + 2, cinfo, before=2,
                                   after=2, workspace=(ws_ctx.ptr, nb_ctx))

    def format_kept():
        m.format_async(d, N, beg, nxt, lcap, out, cap, xinfo, kind_plane=kind, num_plane=rel, glue=glue, terminator=0x0A,
                       workspace=(ws_fm.ptr, nb_fm), **prefix)

    def context_groups():
        m.line_context_async(starts, lcap, linfo, 0, N, offs, picked.size, g_rel, g_beg, g_nxt, lcap + 2, cinfo, before=2,
                             after=2, lines_out=cnt, workspace=(ws_ctx.ptr, nb_ctx))

    def extract_groups():
        m.extract_async(d, N, g_beg, g_nxt, lcap, out, cap, xinfo, glue=glue, terminator=0x0A, workspace=(ws_fm.ptr, nb_fm))

    context_groups()
    extract_groups()
    _, plain_len = figures()
    context_lines()
    format_kept()
    _, mlen = figures()
    kept = int(beg.to_numpy(np.int32, 1)[0])
    exp_lines, exp_ctx = fm.context_lines(e_st, e_info, 0, N, picked + 3, False, 2, 2)
    assert kept == len(exp_lines[0]) and cinfo.to_numpy(np.int32, 4).tolist() == exp_ctx.tolist()
    row = dict(common, case="one_in_100_C2", ranges=kept, groups=int(exp_ctx[2]), output_bytes=mlen, extract_output_bytes=plain_len)
    row.update(timed({"context_lines": context_lines, "format": format_kept,
                      "context_lines_and_format": lambda: (context_lines(), format_kept()),
                      "context_and_extract": lambda: (context_groups(), extract_groups())}, args.seconds))
    context_lines()
    format_kept()
    torch.cuda.synchronize()
    t0 = time.perf_counter()                  # the host path reads the text and the records
    d.to_numpy(np.uint8, N)
    offs.to_numpy(np.int32, picked.size + 1)
    row["host_copy_back_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    row["host_format_us"] = host_path((beg, nxt, rel, kind), kept, glue, mlen)[1]
    row["lines_over_groups"] = round(row["context_lines_and_format"]["median_us"] / row["context_and_extract"]["median_us"], 2)
    row["device_under_host_copy_back"] = bool(row["context_lines_and_format"]["max_us"] < row["host_copy_back_us"])
    emit(row)

    # ---- (c) the matches themselves
    sp = DeviceArray.from_numpy(fm.plane_of(picked + 3), pad_to=0)
    op = DeviceArray.from_numpy(fm.plane_of(picked + 8), pad_to=0)
    num = DeviceArray((picked.size + 2) * 4)

    def only_matching():
        m.line_number_async(starts, lcap, linfo, sp.ptr + 4, picked.size, num.ptr + 4)
        m.format_async(d, N, sp, op, picked.size, out, cap, xinfo, end_inclusive=True, num_plane=num, terminator=0x0A,
                       workspace=(ws_fm.ptr, nb_fm), **prefix)

    only_matching()
    info, mlen = figures()
    row = dict(common, case="only_matching", ranges=int(info[0]), output_bytes=mlen)
    row.update(timed({"number_and_format": only_matching}, args.seconds))
    only_matching()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    text = d.to_numpy(np.uint8, N)
    s, o, ln = (p.to_numpy(np.int32, picked.size + 1)[1:] for p in (sp, op, num))
    t1 = time.perf_counter()
    text = text.tobytes()
    exp = b"".join(NAME + b":%d:%d:" % (n + 1, b) + text[b:e + 1] + (b"" if text[e] == 0x0A else b"\n")
                   for b, e, n in zip(s.tolist(), o.tolist(), ln.tolist()))
    t2 = time.perf_counter()
    assert out.to_numpy(np.uint8, mlen).tobytes() == exp
    row["host_copy_back_us"], row["host_format_us"] = round((t1 - t0) * 1e6, 1), round((t2 - t1) * 1e6, 1)
    row["device_under_host_copy_back"] = bool(row["number_and_format"]["max_us"] < row["host_copy_back_us"])
    emit(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    m.close()


if __name__ == "__main__":
    main()
