"""What the select pass costs: acm_select_matches_async per 32 MiB batch alone, and the whole scan -> expand ->
select chain beside the same chain without it, in one process.  Two workloads: the bench's ClamAV text (random
bytes, 4096 planted signatures: few records, the pass costs its launches) and a match-dense text (sentiment
words: about a record per 35 bytes).  The pass orders max_records cells, so it is given the planes' record count
rounded up to 4096, as a caller who sizes its planes would.  The host-side alternative is timed once beside it:
every record copied back and the serial loop of tests/select_model.py.  The launches of one call are counted by
capturing it into a HIP graph on a stream of its own and counting the graph's nodes: they must be
16 + ceil(log2(max_records + 1)) whatever the planes hold.  Device events around each run, medians over repeated
runs, one JSON line.

python tools/select_bench.py [--seconds 0.5] >> profiles/select_bench.jsonl
"""
import argparse
import ctypes as C
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
import select_model
import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib

N = 32 << 20


def launches_of(m, enqueue):
    """kernel launches enqueue(stream) makes: the nodes of the graph it is captured into (nothing runs)"""
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    _lib.check(m.lib.acm_rt_stream_create(C.byref(stream)), "acm_rt_stream_create")
    graph, nodes = C.c_void_p(), C.c_size_t(0)
    assert hip.hipStreamBeginCapture(stream, 0) == 0           # hipStreamCaptureModeGlobal
    try:
        enqueue(stream)
    finally:
        rc = hip.hipStreamEndCapture(stream, C.byref(graph))
    assert rc == 0 and graph.value
    assert hip.hipGraphGetNodes(graph, None, C.byref(nodes)) == 0
    hip.hipGraphDestroy(graph)
    _lib.check(m.lib.acm_rt_stream_destroy(stream), "acm_rt_stream_destroy")
    return int(nodes.value)


def rounds_for(n):
    return int(n).bit_length()                                 # ceil(log2(n + 1))


def measure(name, set_name, text, seconds):
    path, hx, max_len = fixtures.set_source(set_name)
    a = Automaton()
    a.load_file(path, hx, max_len)
    a.compile()
    lens = [len(a.pattern(i)[0]) for i in range(a.num_patterns)]
    m = Matcher(a, 0, max_text=N)
    patterns = a.num_patterns
    a.close()
    cap = m.plane_capacity
    acap = 4 * cap
    d = DeviceArray.from_numpy(text)
    xp, xo, pat, off, start, info = (DeviceArray(acap * 4), DeviceArray(acap * 4), DeviceArray(acap * 4), DeviceArray(acap * 4),
                                     DeviceArray(acap * 4), DeviceArray(16))
    nb_ex = m.lib.acm_expand_workspace_bytes(cap - 2)
    ws_ex = DeviceArray(nb_ex)

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)

    def expand():
        _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, acap,
                                                  ws_ex.ptr, nb_ex, m.stream), "acm_expand_matches_async")

    scan_state()
    expand()
    entries = int(xp.to_numpy(np.int32, 1)[0])
    assert entries <= acap - 2
    mr = (entries + 4096) & ~4095
    nb_sel = m.lib.acm_select_workspace_bytes(mr)
    ws_sel = DeviceArray(nb_sel)

    def select(stream=None, max_records=mr):
        m.select_async(xp, xo, max_records, pat, off, acap, info, start_out=start, workspace=(ws_sel.ptr, nb_sel), stream=stream)

    def chain_without():
        scan_state()
        expand()

    def chain():
        scan_state()
        expand()
        select()

    runs = {"scan_state": scan_state, "expand": expand, "select_pass": select, "scan_expand": chain_without,
            "scan_expand_select": chain}
    for f in runs.values():   # warm-up (AUTO settles on its pipeline)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    pipeline = m.path_taken(text.size)
    # the launch count, at the size the pass is timed at and at sizes either side of a power of two, whatever the
    # planes hold (a count cell above max_records, and an empty plane: max_records 0)
    counted = {}
    for r in sorted({mr, 0, 1, 4095, 4096, min(mr, 65535), min(mr, 65536)}):
        counted[r] = launches_of(m, lambda s, r=r: select(s, r))
        assert counted[r] == 16 + rounds_for(r), (r, counted[r])
    select()
    selected = int(pat.to_numpy(np.int32, 1)[0])
    sel_info = info.to_numpy(np.int32, 4).tolist()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or len(t["scan_state"]) < 20:
        for key, f in runs.items():   # (xp, xo hold the last expansion: the pass only reads them)
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}
    # the host-side alternative, once: every record copied back, then the model's serial loop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cells = xp.to_numpy(np.int32, entries + 1)[1:]
    offs = xo.to_numpy(np.int32, entries + 1)[1:]
    t1 = time.perf_counter()
    hp, ho, hs, hinfo = select_model.SelectModel(lens).run(cells, offs)
    t2 = time.perf_counter()
    assert hp.size == selected and hinfo == sel_info, (hp.size, selected, hinfo, sel_info)
    assert np.array_equal(pat.to_numpy(np.int32, selected + 1)[1:], hp)
    out = {"workload": name, "pipeline": pipeline, "patterns": patterns, "list_entries": entries, "max_records": mr,
           "eligible": sel_info[0], "dropped": sel_info[1], "selected": selected, "select_launches": counted[mr],
           "select_launches_expected": 16 + rounds_for(mr), "launches_by_max_records": {str(k): v for k, v in counted.items()},
           "doubling_rounds": rounds_for(mr), "select_workspace_bytes": int(nb_sel), "runs": len(t["scan_state"])}
    out.update({k + "_us": v for k, v in med.items()})
    out["select_us_per_launch"] = round(med["select_pass"] / counted[mr], 2)
    out["chain_with_over_without"] = round(med["scan_expand_select"] / med["scan_expand"], 2)
    out["host_copy_back_us"] = round((t1 - t0) * 1e6, 1)
    out["host_model_loop_us"] = round((t2 - t1) * 1e6, 1)
    for b in (d, xp, xo, pat, off, start, info, ws_ex, ws_sel):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    path, hx, max_len = fixtures.set_source("clamav2000")
    a = Automaton()
    a.load_file(path, hx, max_len)
    clam = [a.pattern(i)[0] for i in range(a.num_patterns)]
    a.close()
    rows = [measure("clamav2000, 4096 planted", "clamav2000", synth.clamav_corpus(N, 11, clam), args.seconds)]
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    rows.append(measure("sentiment words", "sentiment", synth.word_corpus(N, 21, words), args.seconds))
    print(json.dumps({"tool": "select_bench", "batch_bytes": N, "workloads": rows}), flush=True)


if __name__ == "__main__":
    main()
