"""What normalised scanning costs: per 32 MiB batch, the normalise pass (acm_normalize_async: three launches) and the
remap (acm_normalize_remap_async) next to a device-to-device copy of the same bytes and to acm_line_index_async on the
same text, the closest existing pass that reads the text once.  Three inputs: text with nothing to drop (no blanks, no
'%': every byte is copied), the sentiment word corpus squeezed ('ws'), and a percent-dense synthetic (a triple every
six bytes, decoded and squeezed).  Device events around each call, medians over repeated runs.  No threshold.

python tools/normalize_bench.py [--seconds 0.5] [--once]     (--once: one call each, for a kernel trace)

Writes one JSON line per input to profiles/normalize_bench.jsonl.  Kernel times: run it under
rocprofv3 --kernel-trace --stats with --once.
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

import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib

N = 32 << 20
RECORDS = 1 << 16            # records the remap carries back: sparse, as a scan's are


def measure(name, text, flags, seconds, once):
    a = Automaton()
    a.add(b"needle", 0)
    a.compile()
    m = Matcher(a, 0, max_text=4096)
    a.close()
    n = int(text.size)
    d = DeviceArray.from_numpy(text)
    out, copy = DeviceArray(n + 32), DeviceArray(n + 32)
    keep, block, info, rinfo = DeviceArray((n + 63) // 64 * 8), DeviceArray((n // 1024 + 2) * 4), DeviceArray(32), DeviceArray(32)
    nws = m.lib.acm_normalize_workspace_bytes(n, 0)
    lws = m.lib.acm_line_index_workspace_bytes(n)
    ws, ws2 = DeviceArray(nws), DeviceArray(lws)
    lcap = n // 16
    starts, linfo = DeviceArray(lcap * 4), DeviceArray(32)

    def normalize():
        m.normalize_async(d, n, flags, out, n, keep, block, info, workspace=(ws.ptr, nws))

    normalize()
    torch.cuda.synchronize()
    h = info.to_numpy(np.int32, 8)
    mlen = int(h[0])
    offs = np.sort(np.random.default_rng(3).integers(0, max(mlen, 1), RECORDS)).astype(np.int32)
    plane = DeviceArray.from_numpy(np.r_[np.int32(RECORDS), offs, np.int32(0)].astype(np.int32))
    mapped = DeviceArray((RECORDS + 2) * 4)

    def remap():
        m.normalize_remap_async(d, n, flags, keep, block, plane, RECORDS, mapped, rinfo)

    def d2d():
        _lib.check(m.lib.acm_rt_memcpy_d2d(copy.ptr, d.ptr, n, None), "acm_rt_memcpy_d2d")

    def index():
        m.line_index_async(d, n, starts, lcap, linfo, workspace=(ws2.ptr, lws))

    calls = (("normalize", normalize), ("remap", remap), ("copy", d2d), ("line_index", index))
    for _ in range(1 if once else 3):
        for _, f in calls:
            f()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k, _ in calls}
    spent = 0.0
    while not once and (spent < 4 * seconds or len(t["copy"]) < 10):
        for key, f in calls:
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: float(np.median(v)) * 1e3 if v else None for k, v in t.items()}
    moved = 2 * n + n // 4 + mlen                       # text twice, the keep words written and read, the output
    res = {"input": name, "bytes": n, "flags": flags, "m": mlen, "dropped": int(h[1]), "triples": int(h[2]),
           "blanks_emitted": int(h[3]), "records": RECORDS, "runs": len(t["copy"]), "bytes_moved": moved}
    for k, v in med.items():
        res[k + "_us"] = round(v, 1) if v is not None else None
    if med["normalize"]:
        res["normalize_over_copy"] = round(med["normalize"] / med["copy"], 2)
        res["normalize_over_line_index"] = round(med["normalize"] / med["line_index"], 2)
        res["normalize_GBps_moved"] = round(moved / med["normalize"] / 1e3, 1)
        res["copy_GBps_moved"] = round(2 * n / med["copy"] / 1e3, 1)
    for b in (d, out, copy, keep, block, info, rinfo, ws, ws2, starts, linfo, plane, mapped):
        b.free()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize_bench.jsonl"))
    args = ap.parse_args()
    rng = np.random.default_rng(5)
    plain = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)[rng.integers(0, 36, N)]
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    real = synth.word_corpus(N, 21, words)
    dense = plain.copy()
    at = np.arange(0, N - 3, 6)
    dense[at], dense[at + 1], dense[at + 2] = 0x25, 0x32, np.where(rng.random(at.size) < 0.5, 0x30, 0x41)   # %20 or %2A
    rows = []
    for name, text, flags in (("nothing to drop", plain, _lib.NORM_PERCENT | _lib.NORM_SQUEEZE),
                              ("sentiment words, ws", real, _lib.NORM_SQUEEZE),
                              ("percent-dense, url,ws", dense, _lib.NORM_PERCENT | _lib.NORM_SQUEEZE)):
        rows.append(measure(name, text, flags, args.seconds, args.once))
        print(json.dumps(rows[-1]), flush=True)
    if not args.once:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
