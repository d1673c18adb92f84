"""What the rewrite pass costs: acm_rewrite_async per 32 MiB batch alone, for three replacement mixes (every pattern
masked, every pattern deleted, every pattern grown to twice its length), the whole scan -> expand -> select ->
rewrite chain, and beside them in the same process a device-to-device copy of the same bytes (the roofline the copy
kernel is judged against) and the select pass alone.  Two workloads: the bench's ClamAV text (random bytes, 4096
planted signatures: the output is one long gap) and a match-dense text (sentiment words: a match per ~44 bytes).
The pass is given the select pass's record count rounded up to 4096 and an output buffer of the size it reports,
as a caller who sizes its buffers would.  The host-side alternative is timed once beside it: the text and the records
copied back and the serial splice of tests/rewrite_model.py.  Device events around each run, medians over repeated
runs, one JSON line.

python tools/rewrite_bench.py [--seconds 0.5] [--source-form TEXT] >> profiles/rewrite_bench.jsonl

The library does not say how it was built, so --source-form names the copy kernel's source-load form in the line: the
default is the default build's; for the other form rebuild csrc/rewrite.hip with -DACM_REWRITE_UNALIGNED_SOURCE
(DESIGN.md 6p has the commands) and pass --source-form "one unaligned 16-byte load".
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

import fixtures
import rewrite_model
import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib

N = 32 << 20
MIXES = ("fill", "delete", "grow2x")


def replacement(mix, pattern):
    return {"fill": (b"*", True), "delete": (b"", False), "grow2x": (pattern + pattern, False)}[mix]


def measure(name, set_name, text, seconds):
    path, hx, max_len = fixtures.set_source(set_name)
    rows = {}
    for mix in MIXES:
        a = Automaton()
        a.load_file(path, hx, max_len)
        pats = [a.pattern(i)[0] for i in range(a.num_patterns)]
        repl = [replacement(mix, p) if p else None for p in pats]
        for i, r in enumerate(repl):
            if r is not None:
                a.set_replacement(i, **({"fill": r[0]} if r[1] else {"data": r[0]}))
        a.compile()
        m = Matcher(a, 0, max_text=N)
        a.close()
        cap = m.plane_capacity
        acap = 4 * cap
        d = DeviceArray.from_numpy(text)
        copy_dst = DeviceArray(N + 16)
        xp, xo, pat, off = (DeviceArray(acap * 4) for _ in range(4))
        sel_info, info = DeviceArray(16), DeviceArray(32)
        nb_ex = m.lib.acm_expand_workspace_bytes(cap - 2)
        ws_ex = DeviceArray(nb_ex)

        def scan_expand():
            m.scan_async(d, text.size, report=_lib.REPORT_STATE)
            _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, acap,
                                                      ws_ex.ptr, nb_ex, m.stream), "acm_expand_matches_async")

        scan_expand()
        entries = int(xp.to_numpy(np.int32, 1)[0])
        assert entries <= acap - 2
        mr_sel = (entries + 4096) & ~4095
        nb_sel = m.lib.acm_select_workspace_bytes(mr_sel)
        ws_sel = DeviceArray(nb_sel)

        def select():
            m.select_async(xp, xo, mr_sel, pat, off, acap, sel_info, workspace=(ws_sel.ptr, nb_sel))

        select()
        selected = int(pat.to_numpy(np.int32, 1)[0])
        mr = (selected + 4096) & ~4095
        nb_rw = m.lib.acm_rewrite_workspace_bytes(mr, 0)
        ws_rw = DeviceArray(nb_rw)
        # the figures alone first: the output's length sizes its buffer
        m.rewrite_async(d, text.size, pat, off, mr, None, 0, info, workspace=(ws_rw.ptr, nb_rw))
        figures = info.to_numpy(np.int32, 8)
        out_len = (int(figures[3]) << 32) | (int(figures[2]) & 0xFFFFFFFF)
        out_cap = (out_len + 4096) & ~4095
        out = DeviceArray(out_cap + 16)

        def rewrite():
            m.rewrite_async(d, text.size, pat, off, mr, out, out_cap, info, workspace=(ws_rw.ptr, nb_rw))

        def chain():
            scan_expand()
            select()
            rewrite()

        def d2d_copy():
            _lib.check(m.lib.acm_rt_memcpy_d2d(copy_dst.ptr, d.ptr, text.size, m.stream), "acm_rt_memcpy_d2d")

        runs = {"rewrite_pass": rewrite, "d2d_copy": d2d_copy}
        if mix == MIXES[0]:
            runs.update({"select_pass": select, "scan_expand_select": lambda: (scan_expand(), select()),
                         "scan_expand_select_rewrite": chain})
        for f in runs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t = {k: [] for k in runs}
        spent = 0.0
        while spent < len(runs) * seconds or len(t["rewrite_pass"]) < 20:
            for key, f in runs.items():
                ev[0].record()
                f()
                ev[1].record()
                torch.cuda.synchronize()
                ms = ev[0].elapsed_time(ev[1])
                t[key].append(ms)
                spent += ms / 1e3
        med = {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}
        got_info = info.to_numpy(np.int32, 8).tolist()
        row = {"used": got_info[0], "skipped": got_info[1], "output_bytes": out_len, "bytes_in_spans": got_info[4],
               "max_records": mr, "rewrite_workspace_bytes": int(nb_rw), "runs": len(t["rewrite_pass"])}
        row.update({k + "_us": v for k, v in med.items()})
        row["rewrite_over_d2d_copy"] = round(med["rewrite_pass"] / med["d2d_copy"], 2)
        row["rewrite_GBps_in_plus_out"] = round((text.size + out_len) / med["rewrite_pass"] / 1e3, 1)
        if mix == MIXES[0]:
            # the host-side alternative, once: the text and the records copied back, then the model's serial splice
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_text = d.to_numpy(np.uint8, text.size)
            cells = pat.to_numpy(np.int32, selected + 1)[1:]
            offs = off.to_numpy(np.int32, selected + 1)[1:]
            t1 = time.perf_counter()
            model = rewrite_model.RewriteModel([len(p) for p in pats], repl)
            hout, hinfo, _, _ = model.run(host_text.tobytes(), cells, offs)
            t2 = time.perf_counter()
            assert hinfo[:6] == got_info[:6], (hinfo, got_info)
            assert out.to_numpy(np.uint8, out_len).tobytes() == hout
            row["host_copy_back_us"] = round((t1 - t0) * 1e6, 1)
            row["host_model_splice_us"] = round((t2 - t1) * 1e6, 1)
            row["pipeline"] = m.path_taken(text.size)
            row["list_entries"] = entries
            row["selected"] = selected
        rows[mix] = row
        for b in (d, copy_dst, xp, xo, pat, off, sel_info, info, ws_ex, ws_sel, ws_rw, out):
            b.free()
        m.close()
    return {"workload": name, "mixes": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--source-form", default="two aligned 16-byte loads and a byte align (the default build)")
    args = ap.parse_args()
    path, hx, max_len = fixtures.set_source("clamav2000")
    a = Automaton()
    a.load_file(path, hx, max_len)
    clam = [a.pattern(i)[0] for i in range(a.num_patterns)]
    a.close()
    rows = [measure("clamav2000, 4096 planted", "clamav2000", synth.clamav_corpus(N, 11, clam), args.seconds)]
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    rows.append(measure("sentiment words", "sentiment", synth.word_corpus(N, 21, words), args.seconds))
    print(json.dumps({"tool": "rewrite_bench", "source_form": args.source_form, "batch_bytes": N, "tile_bytes": 16384, "workloads": rows}), flush=True)


if __name__ == "__main__":
    main()
