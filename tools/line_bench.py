"""What the line passes cost: per 32 MiB batch, the line index (acm_line_index_async) next to the scan
of the same text, and the number and select passes behind that scan.  The two workloads of
tools/segment_bench.py: sentiment text with a newline every ~140 bytes, and clamav2000 text, which has a
newline byte every 256 or so.  Device events around each call, medians over repeated runs; the line
starts go to an array of n / 16 cells (every line has room; the INT32_MAX tail is part of the time).

python tools/line_bench.py [--seconds 0.5] [--once]     (--once: one call each, for a kernel trace)

Writes one JSON line per workload to profiles/line_bench.jsonl.  Kernel times: run it under
rocprofv3 --kernel-trace --stats with --once and keep the kernel_stats.csv as
profiles/line_kernel_stats.csv.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fixtures
import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher

N = 32 << 20
BULK_TBPS = 5.6   # the sparse pipeline's bulk kernel reads the text at this rate


def measure(name, set_name, text, seconds, once):
    path, hx, max_len = fixtures.set_source(set_name)
    a = Automaton()
    a.load_file(path, hx, max_len)
    a.compile()
    m = Matcher(a, 0, max_text=N)
    a.close()
    n = int(text.size)
    cap = m.plane_capacity
    lcap = n // 16
    d = DeviceArray.from_numpy(text)
    idx_ws = m.lib.acm_line_index_workspace_bytes(n)
    sel_ws = m.lib.acm_line_select_workspace_bytes(lcap)
    starts, info, ws, ws2 = DeviceArray(lcap * 4), DeviceArray(32), DeviceArray(idx_ws), DeviceArray(sel_ws)
    num, rel, beg, nxt = (DeviceArray(cap * 4) for _ in range(4))

    def scan():
        m.scan_async(d, n)

    def index():
        m.line_index_async(d, n, starts, lcap, info, workspace=(ws.ptr, idx_ws))

    def number():
        m.line_number_async(starts, lcap, info, m.off_plane.ptr + 4, cap - 2, num, d_count=m.off_plane)

    def select():
        m.line_select_async(starts, lcap, info, 0, n, m.off_plane, cap - 2, rel, beg, nxt, cap, workspace=(ws2.ptr, sel_ws))

    calls = (("scan", scan), ("index", index), ("number", number), ("select", select))
    for _ in range(1 if once else 3):   # warm-up (AUTO settles on its pipeline)
        for _, f in calls:
            f()
    torch.cuda.synchronize()
    h_info = info.to_numpy(np.int32, 8)
    assert int(h_info[0]) <= lcap and int(h_info[1]) == int(np.count_nonzero(text == 0x0A))
    records = int(m.pat_plane.to_numpy(np.int32, 1)[0])
    selected = int(rel.to_numpy(np.int32, 1)[0])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k, _ in calls}
    spent = 0.0
    while not once and (spent < 4 * seconds or len(t["scan"]) < 10):
        for key, f in calls:
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: float(np.median(v)) * 1e3 if v else None for k, v in t.items()}
    floor_us = n / (BULK_TBPS * 1e12) * 1e6
    out = {"workload": name, "pipeline": m.path_taken(n), "bytes": n, "lines": int(h_info[0]), "line_cells": lcap,
           "records": records, "lines_selected": selected, "runs": len(t["scan"]),
           "one_read_floor_us": round(floor_us, 1)}
    for k, v in med.items():
        out[k + "_us"] = round(v, 1) if v is not None else None
    if med["index"]:
        out["index_over_floor"] = round(med["index"] / floor_us, 2)
        out["index_GBps"] = round(n / med["index"] / 1e3, 1)
    for b in (d, starts, info, ws, ws2, num, rel, beg, nxt):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_bench.jsonl"))
    args = ap.parse_args()
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    text = synth.word_corpus(N, 21, words)
    sp = np.flatnonzero(text == 0x20)
    text[sp[np.random.default_rng(1).random(sp.size) < 0.05]] = 0x0A   # a line every ~140 bytes
    rows = [measure("sentiment, ~140-byte lines", "sentiment", text, args.seconds, args.once)]
    print(json.dumps(rows[-1]), flush=True)
    clam = [p for p, _ in fixtures.oracle_for("clamav2000").patterns()]
    text = synth.clamav_corpus(N, 11, clam, 200)
    rows.append(measure("clamav2000, newline bytes of binary text", "clamav2000", text, args.seconds, args.once))
    print(json.dumps(rows[-1]), flush=True)
    if not args.once:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
