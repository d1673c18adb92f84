"""What position constraints cost: the position pass (acm_position_matches_async) per 32 MiB batch beside the
word pass and the case pass over the same records, in one process.  Two workloads: sentiment words with
punctuation (many records) and clamav2000 text with 200 planted signatures (few records: the passes cost
their two launches).  Every tenth pattern is constrained, alternately from the start (0..4096) and from the
end (L..65536) of its text; the texts are 64 KiB pieces of the batch (512 starts), the last one ends with
the batch.  The pass is timed over states (first and all form) and over the pattern-form planes of the
expansion (all form).  Device events around each run, medians over repeated runs, one JSON line.

python tools/position_bench.py [--seconds 0.5] >> profiles/position_bench.jsonl
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
PIECE = 64 << 10


def punctuate(text, seed):
    """sentiment words with punctuation: a tenth of the spaces become '.', ',', '!', '?', '"', newline"""
    t = text.copy()
    sp = np.flatnonzero(t == ord(" "))
    rng = np.random.default_rng(seed)
    pick = sp[rng.random(sp.size) < 0.1]
    t[pick] = np.frombuffer(b".,!?\"\n", dtype=np.uint8)[rng.integers(0, 6, pick.size)]
    return t


def measure(name, set_name, text, seconds):
    path, hx, max_len = fixtures.set_source(set_name)
    a = Automaton()
    a.load_file(path, hx, max_len)
    a.compile()
    constrained = 0
    for i in range(0, a.num_patterns, 10):
        L = len(a.pattern(i)[0])
        if i % 20:
            a.set_position(i, L, 65536, from_end=True)
        else:
            a.set_position(i, 0, 4096)
        constrained += 1
    m = Matcher(a, 0, max_text=N)
    patterns = a.num_patterns
    a.close()
    cap = m.plane_capacity
    acap = 4 * cap
    d = DeviceArray.from_numpy(text)
    starts = np.arange(0, text.size, PIECE, dtype=np.int32)
    d_st = DeviceArray.from_numpy(starts, pad_to=0)
    nb = {k: f(acap) for k, f in (("pos", m.lib.acm_position_workspace_bytes), ("word", m.lib.acm_word_workspace_bytes),
                                  ("case", m.lib.acm_case_workspace_bytes), ("ex", m.lib.acm_expand_workspace_bytes))}
    ws = {k: DeviceArray(v) for k, v in nb.items()}
    pat, off, xp, xo, info = (DeviceArray(acap * 4), DeviceArray(acap * 4), DeviceArray(acap * 4), DeviceArray(acap * 4),
                              DeviceArray(16))

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)

    def position(all_patterns, heads=False):
        sp, so, mr = (xp, xo, acap - 2) if heads else (m.pat_plane, m.off_plane, cap - 2)
        m.position_async(sp, so, mr, pat, off, acap, info, report=_lib.REPORT_HEAD if heads else _lib.REPORT_STATE,
                         seg_start=d_st, segments=starts.size, text_end=text.size, open_end=text.size,
                         all_patterns=all_patterns, workspace=(ws["pos"].ptr, nb["pos"]))

    def word(all_patterns):
        m.word_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, pat, off, acap, seg_start=d_st,
                     segments=starts.size, all_patterns=all_patterns, workspace=(ws["word"].ptr, nb["word"]))

    def case(all_patterns):
        m.case_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, pat, off, acap, all_patterns=all_patterns,
                     workspace=(ws["case"].ptr, nb["case"]))

    runs = {
        "scan_state": scan_state,
        "position_pass_first": lambda: position(False),
        "position_pass_all": lambda: position(True),
        "position_pass_heads_all": lambda: position(True, True),
        "position_pass_heads_first": lambda: position(False, True),
        "word_pass_head": lambda: word(False),
        "word_pass_all": lambda: word(True),
        "case_pass_head": lambda: case(False),
        "case_pass_all": lambda: case(True),
    }
    scan_state()
    assert m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, acap,
                                          ws["ex"].ptr, nb["ex"], m.stream) == 0
    entries = int(xp.to_numpy(np.int32, 1)[0])
    assert entries <= acap - 2
    for f in runs.values():   # warm-up (AUTO settles on its pipeline)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    scan_state()
    records = int(m.pat_plane.to_numpy(np.int32, 1)[0])
    pipeline = m.path_taken(text.size)
    counts = {}
    for key, f in runs.items():
        if key != "scan_state":
            f()
            counts[key] = int(pat.to_numpy(np.int32, 1)[0])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or len(t["scan_state"]) < 20:
        for key, f in runs.items():   # (the planes hold the last scan_state's records: the passes only read them)
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}
    out = {"workload": name, "pipeline": pipeline, "patterns": patterns, "constrained": constrained,
           "starts": int(starts.size), "records": records, "list_entries": entries, "runs": len(t["scan_state"])}
    out.update({k + "_records": v for k, v in counts.items()})
    out.update({k + "_us": v for k, v in med.items()})
    out["position_over_word_first"] = round(med["position_pass_first"] / med["word_pass_head"], 2)
    out["position_over_word_all"] = round(med["position_pass_all"] / med["word_pass_all"], 2)
    for b in [d, d_st, pat, off, xp, xo, info] + list(ws.values()):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    text = punctuate(synth.word_corpus(N, 21, words), 2)
    rows = [measure("sentiment words, spaces and punctuation", "sentiment", text, args.seconds)]
    path, hx, max_len = fixtures.set_source("clamav2000")
    a = Automaton()
    a.load_file(path, hx, max_len)
    clam = [a.pattern(i)[0] for i in range(a.num_patterns)]
    a.close()
    text = synth.clamav_corpus(N, 11, clam, 200)
    rows.append(measure("clamav2000, 200 planted", "clamav2000", text, args.seconds))
    print(json.dumps({"tool": "position_bench", "batch_bytes": N, "workloads": rows}), flush=True)


if __name__ == "__main__":
    main()
