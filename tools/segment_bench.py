"""What a segmented scan costs: per 32 MiB batch, the plain scan (A) against the scan that reports
final states followed by the segment pass (B, acm_segment_matches_async), and the segment pass alone.
Two workloads: sentiment text cut into tweet-sized segments (~140 bytes) and clamav2000 text cut
into 4 KiB "files".  Device events around each run, medians over repeated runs.

python tools/segment_bench.py [--seconds 0.5]
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
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib

N = 32 << 20


def measure(name, set_name, text, starts, seconds):
    path, hx, max_len = fixtures.set_source(set_name)
    a = Automaton()
    a.load_file(path, hx, max_len)
    a.compile()
    m = Matcher(a, 0, max_text=N)
    a.close()
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)
    d_st = DeviceArray.from_numpy(starts, pad_to=0)
    ws_bytes = m.lib.acm_segment_workspace_bytes(cap - 2)
    ws, pat, off = DeviceArray(ws_bytes), DeviceArray(cap * 4), DeviceArray(cap * 4)

    def plain():
        m.scan_async(d, text.size)

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)

    def segment():
        m.segment_async(m.pat_plane, m.off_plane, cap - 2, d_st, starts.size, text.size, pat, off, cap,
                        workspace=(ws.ptr, ws_bytes))

    def segmented():
        scan_state()
        segment()

    for f in (plain, segmented):   # warm-up (AUTO settles on its pipeline)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    records = int(m.pat_plane.to_numpy(np.int32, 1)[0])
    plain()
    path = m.path_taken(text.size)
    kept = int(pat.to_numpy(np.int32, 1)[0])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {"plain": [], "segmented": [], "segment_pass": []}
    spent = 0.0
    while spent < 3 * seconds or len(t["plain"]) < 10:
        for key, f in (("plain", plain), ("segmented", segmented), ("segment_pass", segment)):
            if key == "segment_pass":
                scan_state()
                torch.cuda.synchronize()
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
    out = {"workload": name, "pipeline": path, "segments": int(starts.size), "records_in": records,
           "records_kept": kept, "runs": len(t["plain"]), "plain_us": round(med["plain"], 1),
           "scan_plus_segment_us": round(med["segmented"], 1), "segment_pass_us": round(med["segment_pass"], 1),
           "added_us": round(med["segmented"] - med["plain"], 1),
           "added_pct": round(100 * (med["segmented"] / med["plain"] - 1), 1)}
    for b in (d, d_st, ws, pat, off):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    text = synth.word_corpus(N, 21, words)
    rng = np.random.default_rng(1)
    starts = np.concatenate([[0], np.cumsum(rng.integers(100, 181, N // 100))])
    starts = starts[starts < N].astype(np.int32)
    print(json.dumps(measure("sentiment, ~140-byte segments", "sentiment", text, starts, args.seconds)), flush=True)
    clam = [p for p, _ in fixtures.oracle_for("clamav2000").patterns()]
    text = synth.clamav_corpus(N, 11, clam, 200)
    starts = np.arange(0, N, 4096, dtype=np.int32)
    print(json.dumps(measure("clamav2000, 4 KiB files", "clamav2000", text, starts, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
