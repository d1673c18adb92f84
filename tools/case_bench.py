"""What case sensitivity per pattern costs: the case pass (acm_case_matches_async) per 32 MiB batch on the
clamav2000 workload with every second pattern flagged ACM_PATTERN_NOCASE, beside the word pass
(acm_word_matches_async) over the same records, both in the head and the all form, in one process.
Two texts: the usual corpus (200 planted signatures: few records, the passes cost their two launches) and
one planted densely with the signatures in random case (many records, most exact candidates fail).
Device events around each run, medians over repeated runs.

python tools/case_bench.py [--seconds 0.5] >> profiles/case_bench.jsonl
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


def patterns():
    path, hx, max_len = fixtures.set_source("clamav2000")
    a = Automaton()
    a.load_file(path, hx, max_len)
    pats = [a.pattern(i)[0] for i in range(a.num_patterns)]
    a.close()
    return pats


def random_case(t, seed):
    t = t.copy()
    letter = ((t | 0x20) >= ord("a")) & ((t | 0x20) <= ord("z"))
    t[letter & (np.random.default_rng(seed).random(t.size) < 0.5)] ^= 0x20
    return t


def measure(name, pats, text, seconds):
    a = Automaton()
    for i, p in enumerate(pats):
        a.add(p, i, nocase=bool(i & 1))
    a.compile()
    assert a.mixed_case
    m = Matcher(a, 0, max_text=N)
    a.close()
    cap = m.plane_capacity
    acap = 4 * cap
    d = DeviceArray.from_numpy(text)
    cs_bytes = m.lib.acm_case_workspace_bytes(cap - 2)
    wd_bytes = m.lib.acm_word_workspace_bytes(cap - 2)
    cs, wd, pat, off = DeviceArray(cs_bytes), DeviceArray(wd_bytes), DeviceArray(acap * 4), DeviceArray(acap * 4)

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)

    def case(all_patterns):
        m.case_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, pat, off, acap, all_patterns=all_patterns,
                     workspace=(cs.ptr, cs_bytes))

    def word(all_patterns):
        m.word_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, pat, off, acap, all_patterns=all_patterns,
                     workspace=(wd.ptr, wd_bytes))

    runs = {
        "scan_state": scan_state,
        "case_pass_head": lambda: case(False),
        "case_pass_all": lambda: case(True),
        "word_pass_head": lambda: word(False),
        "word_pass_all": lambda: word(True),
    }
    for f in runs.values():   # warm-up (AUTO settles on its pipeline)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    scan_state()
    records = int(m.pat_plane.to_numpy(np.int32, 1)[0])
    pipeline = m.path_taken(text.size)
    counts = {}
    for key, f in (("case_head", lambda: case(False)), ("case_all", lambda: case(True)), ("word_head", lambda: word(False)),
                   ("word_all", lambda: word(True))):
        f()
        counts[key] = int(pat.to_numpy(np.int32, 1)[0])
    ex_bytes = m.lib.acm_expand_workspace_bytes(cap - 2)
    ex = DeviceArray(ex_bytes)
    assert m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, pat.ptr, off.ptr, acap, ex.ptr,
                                          ex_bytes, m.stream) == 0
    entries = int(pat.to_numpy(np.int32, 1)[0])
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
    out = {"workload": name, "pipeline": pipeline, "patterns": len(pats), "flagged": len(pats) // 2, "records": records,
           "list_entries": entries, "case_records_head": counts["case_head"], "case_entries_all": counts["case_all"],
           "word_records_head": counts["word_head"], "word_entries_all": counts["word_all"], "runs": len(t["scan_state"]),
           "scan_state_us": med["scan_state"], "case_pass_head_us": med["case_pass_head"],
           "case_pass_all_us": med["case_pass_all"], "word_pass_head_us": med["word_pass_head"],
           "word_pass_all_us": med["word_pass_all"],
           "case_over_word_head": round(med["case_pass_head"] / med["word_pass_head"], 2),
           "case_over_word_all": round(med["case_pass_all"] / med["word_pass_all"], 2)}
    for b in (d, cs, wd, ex, pat, off):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    pats = patterns()
    text = synth.clamav_corpus(N, 11, pats, 200)
    print(json.dumps(measure("clamav2000, 200 planted", pats, text, args.seconds)), flush=True)
    text = random_case(synth.clamav_corpus(N, 12, pats, 200000), 5)
    print(json.dumps(measure("clamav2000, 200000 planted in random case", pats, text, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
