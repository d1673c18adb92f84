"""What counting on the device saves: per 32 MiB batch, results on the host at the end of the timed region,
  records path   STATE scan + segment pass (HEAD) + copy-back of m + 2 cells of both planes
  tally path     STATE scan + segment pass (STATE) + tally (per-class totals, per-segment rows) + copy-back
                 of the rows and the totals
and the passes alone on the same records: the tally, k_segment's two launches, and STATE + all patterns
tallied against acm_expand_matches_async.  Two workloads: sentiment text in ~140-byte segments with two
classes (sign of the pattern id), and clamav2000 text in 4 KiB files with one class per signature (totals
only: 8192 files x 2000 signatures of rows would be 65 MB, more than the records they replace).
Device events on one stream around each run, host copies into pinned memory inside the timed region,
medians and the 5th / 95th percentile over repeated runs.

python tools/tally_bench.py [--seconds 0.5] [--out profiles/tally_bench.jsonl]
rocprofv3 --kernel-trace --stats -d DIR -- python tools/tally_bench.py --seconds 0.1    (kernel times, a run of its own)
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
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib, api

N = 32 << 20


def measure(name, set_name, text, starts, classes, seconds, want_rows=True):
    path, hx, max_len = fixtures.set_source(set_name)
    a = Automaton()
    a.load_file(path, hx, max_len)
    a.compile()
    m = Matcher(a, 0, max_text=N)
    if classes == "sign":
        labels, cmap = api.class_map(np.sign(a.iids()))
        C = len(labels)
    else:
        cmap, C = None, a.num_patterns
    a.close()
    cap, S = m.plane_capacity, int(starts.size)
    mr = cap - 2
    d = DeviceArray.from_numpy(text)
    d_st = DeviceArray.from_numpy(starts, pad_to=0)
    d_map = DeviceArray.from_numpy(cmap, pad_to=0) if cmap is not None else None
    seg_wsb, tal_wsb, exp_wsb = (m.lib.acm_segment_workspace_bytes(mr), m.lib.acm_tally_workspace_bytes(mr, C),
                                 m.lib.acm_expand_workspace_bytes(mr))
    seg_ws, tal_ws, exp_ws = DeviceArray(seg_wsb), DeviceArray(tal_wsb), DeviceArray(exp_wsb)
    pat, off = DeviceArray(cap * 4), DeviceArray(cap * 4)
    xcap = 8 * cap
    xpat, xoff = DeviceArray(xcap * 4), DeviceArray(xcap * 4)
    tot, rows, lead = DeviceArray(C * 8), DeviceArray(max(S * C * 4 if want_rows else 0, 16)), DeviceArray(max(C * 4, 16))
    RB = S * C * 4 if want_rows else 0   # bytes of the per-segment rows
    host = torch.empty(max(2 * cap * 4, RB + C * 16), dtype=torch.uint8).pin_memory()
    hp = host.data_ptr()

    def d2h(dst_off, src, nbytes):
        _lib.check(m.lib.acm_rt_memcpy_d2h(hp + dst_off, src.ptr, nbytes, None), "acm_rt_memcpy_d2h")

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)

    def segment(report):
        m.segment_async(m.pat_plane, m.off_plane, mr, d_st, S, text.size, pat, off, cap, report=report,
                        workspace=(seg_ws.ptr, seg_wsb))

    def tally(planes=None, all_patterns=False, with_rows=want_rows):
        p, o = planes if planes is not None else (pat, off)
        m.tally_async(p, o, mr, tot, report=_lib.REPORT_STATE, all_patterns=all_patterns, class_of=d_map, num_classes=C,
                      seg_start=d_st if with_rows else None, segments=S if with_rows else 0,
                      seg_class=rows if with_rows else None, lead=lead, workspace=(tal_ws.ptr, tal_wsb))

    kept = [0]

    def records_path():
        scan_state()
        segment(_lib.REPORT_HEAD)
        d2h(0, pat, 4)
        torch.cuda.synchronize()          # the count decides how much comes back, as Matcher.scan_segments does
        n = min(int(np.frombuffer(host.numpy()[:4].tobytes(), dtype=np.int32)[0]), cap - 2)
        kept[0] = n
        d2h(0, pat, (n + 2) * 4)
        d2h(cap * 4, off, (n + 2) * 4)

    def tally_path():
        scan_state()
        segment(_lib.REPORT_STATE)
        tally()
        if want_rows:
            d2h(0, rows, RB)
        d2h(RB, tot, C * 8)
        d2h(RB + C * 8, lead, C * 4)

    def expand_path():
        scan_state()
        _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, mr, xpat.ptr, xoff.ptr, xcap,
                                                  exp_ws.ptr, exp_wsb, None), "acm_expand_matches_async")

    def all_tally_path():
        scan_state()
        tally(planes=(m.pat_plane, m.off_plane), all_patterns=True, with_rows=False)

    runs = {"records_path": records_path, "tally_path": tally_path, "scan_plus_expand": expand_path,
            "scan_plus_all_patterns_tally": all_tally_path,
            "segment_pass_alone": lambda: segment(_lib.REPORT_STATE), "tally_pass_alone": tally}
    for f in runs.values():   # warm-up (AUTO settles on its pipeline)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    records = int(m.pat_plane.to_numpy(np.int32, 1)[0])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or len(t["tally_path"]) < 10:
        for key, f in runs.items():   # alternating, so drift hits every path alike
            if key.endswith("_alone"):
                scan_state()
                if key == "tally_pass_alone":
                    segment(_lib.REPORT_STATE)
                torch.cuda.synchronize()
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    out = {"workload": name, "pipeline": m.path_taken(text.size), "segments": S, "classes": C, "records_in": records,
           "records_kept": kept[0], "runs": len(t["tally_path"]),
           "copy_back_records_bytes": 2 * (kept[0] + 2) * 4, "per_segment_rows": want_rows,
           "copy_back_tally_bytes": RB + C * 12}
    for k, v in t.items():
        us = np.array(v) * 1e3
        out[k + "_us"] = round(float(np.median(us)), 1)
        out[k + "_p5_p95_us"] = [round(float(np.percentile(us, 5)), 1), round(float(np.percentile(us, 95)), 1)]
    out["tally_path_saves_us"] = round(out["records_path_us"] - out["tally_path_us"], 1)
    for b in (d, d_st, d_map, seg_ws, tal_ws, exp_ws, pat, off, xpat, xoff, tot, rows, lead):
        if b is not None:
            b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tally_bench.jsonl"))
    args = ap.parse_args()
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    text = synth.word_corpus(N, 21, words)
    rng = np.random.default_rng(1)
    starts = np.concatenate([[0], np.cumsum(rng.integers(100, 181, N // 100))])
    starts = starts[starts < N].astype(np.int32)
    lines = [measure("sentiment, ~140-byte segments, 2 classes", "sentiment", text, starts, "sign", args.seconds)]
    print(json.dumps(lines[-1]), flush=True)
    clam = [p for p, _ in fixtures.oracle_for("clamav2000").patterns()]
    text = synth.clamav_corpus(N, 11, clam, 200)
    starts = np.arange(0, N, 4096, dtype=np.int32)
    lines.append(measure("clamav2000, 4 KiB files, identity classes", "clamav2000", text, starts, "identity", args.seconds,
                         want_rows=False))
    print(json.dumps(lines[-1]), flush=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
