"""What ASCII case folding costs: a nocase matcher on text T (A) against a case-sensitive matcher of
the folded patterns on fold(T) (B).  A and B produce the same records and do the same matching
work, so their ratio is the price of the fold in the kernels.  Launch groups of 32 MiB batches,
A and B alternating in one process, device events around each group.

python tools/nocase_bench.py [--batches 4] [--seconds 0.5]
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
FOLD = np.arange(256, dtype=np.uint8)
FOLD[ord("a"):ord("z") + 1] -= 0x20


def scramble(t, seed):
    t = np.array(t, dtype=np.uint8, copy=True)
    letter = ((t | 0x20) >= ord("a")) & ((t | 0x20) <= ord("z"))
    t[letter & (np.random.default_rng(seed).random(t.size) < 0.5)] ^= 0x20
    return t


class Side:
    """a matcher and a launch group of batches, each with its own text, workspace and planes"""

    def __init__(self, patterns, nocase, texts, mode):
        a = Automaton(nocase=nocase)
        for p, iid in patterns:
            a.add(p, iid)
        a.compile()
        self.m = Matcher(a, 0, max_text=N, plane_capacity=16)
        a.close()
        self.mode = self.m.set_mode(mode)
        self.cap = 8 << 20
        ws_bytes = self.m.lib.acm_scan_workspace_bytes(self.m.dfa, N)
        self.bufs = []
        self.batches = []
        for t in texts:
            d, ws = DeviceArray.from_numpy(t), DeviceArray(ws_bytes)
            pat, off = DeviceArray(self.cap * 4), DeviceArray(self.cap * 4)
            self.bufs += [d, ws, pat, off]
            self.batches.append(self.m.make_batch(d, t.size, None, pat, off, self.cap, (ws, ws_bytes)))
        self.planes = [(self.bufs[4 * k + 2], self.bufs[4 * k + 3]) for k in range(len(texts))]

    def run(self):
        self.m.enqueue_many(self.batches)

    def records(self, k):
        p = self.planes[k][0].to_numpy(np.int32, self.cap)
        q = self.planes[k][1].to_numpy(np.int32, self.cap)
        c = int(p[0])
        return q[1:1 + c].copy(), p[1:1 + c].copy(), int(p[c + 1])

    def close(self):
        for b in self.bufs:
            b.free()
        self.m.close()


def measure(name, patterns, texts, mode, seconds):
    folded = [(bytes(FOLD[np.frombuffer(p, dtype=np.uint8)]) if p else b"", iid) for p, iid in patterns]
    a = Side(patterns, True, texts, mode)
    b = Side(folded, False, [FOLD[t] for t in texts], mode)
    for s in (a, b):   # warm-up (AUTO settles on its pipeline), and A == B
        for _ in range(3):
            s.run()
    torch.cuda.synchronize()
    for k in range(len(texts)):
        ra, rb = a.records(k), b.records(k)
        assert ra[0].size == rb[0].size and np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) \
            and ra[2] == rb[2], "A and B differ on batch %d" % k
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {"A": [], "B": []}
    spent = 0.0
    while spent < 2 * seconds or len(t["A"]) < 5:
        for key, s in (("A", a), ("B", b)):
            ev[0].record()
            s.run()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    gb = len(texts) * N / 1e9
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"workload": name, "mode": mode, "records_per_batch": int(a.records(0)[0].size),
           "batches_per_group": len(texts), "groups_each": len(t["A"]),
           "A_nocase_GBps": round(gb / (med["A"] / 1e3), 1), "B_folded_GBps": round(gb / (med["B"] / 1e3), 1),
           "A_over_B": round(med["B"] / med["A"], 3)}
    a.close()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", default=None, help="clamav-auto | clamav-chain | sentiment")
    args = ap.parse_args()
    work = []
    clam = fixtures.oracle_for("clamav2000").patterns()
    clam_pats = [p for p, _ in clam]
    clam_texts = [scramble(synth.clamav_corpus(N, 11 + k, clam_pats, 200), 31 + k) for k in range(args.batches)]
    work.append(("clamav-auto", "clamav2000", clam, clam_texts, "auto"))
    work.append(("clamav-chain", "clamav2000", clam, clam_texts, "chain"))
    senti = fixtures.oracle_for("sentiment").patterns()
    words = open(os.path.join(ROOT, "tests", "data", "sentiment", "top5000_words.txt")).read().split()
    senti_texts = [scramble(synth.word_corpus(N, 21 + k, words), 41 + k) for k in range(args.batches)]
    work.append(("sentiment", "sentiment (LDS walk)", senti, senti_texts, "auto"))
    for key, name, pats, texts, mode in work:
        if args.only and key != args.only:
            continue
        print(json.dumps(measure(name, pats, texts, mode, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
