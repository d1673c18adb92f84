"""What whole-word matching costs: per 32 MiB batch, the plain scan (A) against the scan that reports
final states followed by the word pass (B, acm_word_matches_async), and the word pass alone, in the
head form (first word-bounded pattern per offset) and the all form (every word-bounded pattern).
Two workloads: sentiment words with spaces and punctuation (the LDS walk), and clamav2000 text (the
sparse pipeline).  Also reports how many of the plain scan's records are sub-word hits: records
whose every pattern touches a word byte.  Device events around each run, medians over repeated runs.

python tools/word_bench.py [--seconds 0.5]
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
    m = Matcher(a, 0, max_text=N)
    a.close()
    cap = m.plane_capacity
    acap = 4 * cap
    d = DeviceArray.from_numpy(text)
    ws_bytes = m.lib.acm_word_workspace_bytes(cap - 2)
    ex_bytes = m.lib.acm_expand_workspace_bytes(cap - 2)
    ws, ex, pat, off = DeviceArray(ws_bytes), DeviceArray(ex_bytes), DeviceArray(acap * 4), DeviceArray(acap * 4)

    def plain():
        m.scan_async(d, text.size)

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)

    def word(all_patterns):
        m.word_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, pat, off, acap, all_patterns=all_patterns,
                     workspace=(ws.ptr, ws_bytes))

    def expand():
        check = m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, pat.ptr, off.ptr,
                                               acap, ex.ptr, ex_bytes, m.stream)
        assert check == 0

    runs = {
        "plain": plain,
        "words_head": lambda: (scan_state(), word(False)),
        "words_all": lambda: (scan_state(), word(True)),
        "expand": lambda: (scan_state(), expand()),
        "word_pass_head": lambda: word(False),
        "word_pass_all": lambda: word(True),
    }
    alone = {"word_pass_head", "word_pass_all"}
    for f in runs.values():   # warm-up (AUTO settles on its pipeline)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    plain()
    records = int(m.pat_plane.to_numpy(np.int32, 1)[0])
    pipeline = m.path_taken(text.size)
    counts = {}
    for key in ("head", "all"):
        scan_state()
        word(key == "all")
        counts[key] = int(pat.to_numpy(np.int32, 1)[0])
    scan_state()
    expand()
    entries = int(pat.to_numpy(np.int32, 1)[0])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or len(t["plain"]) < 10:
        for key, f in runs.items():
            if key in alone:
                scan_state()
                torch.cuda.synchronize()
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}
    out = {"workload": name, "pipeline": pipeline, "lds_walk": m.lds_resident(), "records": records,
           "word_records_head": counts["head"], "subword_records": records - counts["head"],
           "list_entries": entries, "word_entries_all": counts["all"], "runs": len(t["plain"]),
           "plain_us": med["plain"], "scan_plus_words_head_us": med["words_head"],
           "scan_plus_words_all_us": med["words_all"], "scan_plus_expand_us": med["expand"],
           "word_pass_head_us": med["word_pass_head"], "word_pass_all_us": med["word_pass_all"],
           "added_head_us": round(med["words_head"] - med["plain"], 1),
           "added_head_pct": round(100 * (med["words_head"] / med["plain"] - 1), 1)}
    for b in (d, ws, ex, pat, off):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    text = punctuate(synth.word_corpus(N, 21, words), 2)
    print(json.dumps(measure("sentiment words, spaces and punctuation", "sentiment", text, args.seconds)), flush=True)
    clam = [p for p, _ in fixtures.oracle_for("clamav2000").patterns()]
    text = synth.clamav_corpus(N, 11, clam, 200)
    print(json.dumps(measure("clamav2000", "clamav2000", text, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
