"""Generate tests/golden/golden.json from the REFERENCE's own acsmx.c.

Run in the build container (needs /root/reference; uses oracle/_ref, i.e. the
reference's acsmx.c compiled unmodified behind oracle/ref_harness.c):

    python tests/golden/make_golden.py

For every fixture pattern set the reference builds its DFA; we record state
count, max pattern length, a digest of the serialised table (defined cells
only) and, for seeded synthetic texts, the record stream the serial walk over
the reference's state_table produces (count, FNV-1a digest, final state,
first records).  The texts themselves are regenerated from seeds
(tests/synth.py); their sha256 is stored so generator drift is detected.

The reference ships no expected outputs: these vectors are what
pins the oracle and the HIP path.

    python tests/golden/make_golden.py compiled

writes tests/golden/compiled_reference.json instead: what
test_oracle_golden.py::test_oracle_equals_compiled_reference compares the oracle with
(state count, sha256 of the whole table, the match lists of sampled states, a scan from a
drawn state and the all-patterns walk over the reference's table and match lists), so that
the comparison holds where oracle/_ref cannot be built.  The same test still compares
live wherever oracle/_ref exists.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)

import orc  # noqa: E402
import synth  # noqa: E402

FULL = 32 << 20


def ref_and_patterns(path, hex_, max_len):
    # parse with the oracle's loader (ocl_worker.c parser restatement), build with the reference
    o = orc.Oracle()
    o.load(path, hex_, max_len)
    pats = o.patterns()
    r = orc.RefAcsmx()
    for b, iid in pats:
        r.add(b, iid)
    r.compile()
    return r, pats


def text_for(spec, pats):
    kind = spec["kind"]
    if kind == "file":
        return np.fromfile(os.path.join(orc.DATA, spec["path"]), dtype=np.uint8)
    if kind == "clamav":
        return synth.clamav_corpus(spec["n"], spec["seed"], [p for p, _ in pats], spec["n_plant"])
    if kind == "words":
        words = open(os.path.join(orc.DATA, "sentiment", "top5000_words.txt")).read().split()
        return synth.word_corpus(spec["n"], spec["seed"], words)
    if kind == "repeat":
        p = pats[spec["pattern"]][0]
        return np.frombuffer((p * (spec["n"] // len(p) + 1))[: spec["n"]], dtype=np.uint8).copy()
    if kind == "zeros":
        return np.zeros(spec["n"], dtype=np.uint8)
    raise KeyError(kind)


def main():
    tmp = tempfile.mkdtemp()
    sets = [
        # name, path, hex, max_len, texts
        ("tests", orc.pattern_set("tests")[0], False, -1,
         [{"kind": "file", "path": "ref_tests/input.txt"}]),
        ("tests1", orc.pattern_set("tests1")[0], False, -1,
         [{"kind": "file", "path": "ref_tests/1/input.txt"}]),
        ("tests2", orc.pattern_set("tests2")[0], False, -1,
         [{"kind": "words", "n": 1 << 20, "seed": 3}]),
        ("tests3", orc.pattern_set("tests3")[0], False, -1,
         [{"kind": "file", "path": "ref_tests/3/lala2_uncat.txt"}]),
        ("sentiment", orc.pattern_set("sentiment")[0], False, -1,
         [{"kind": "words", "n": 1 << 20, "seed": 11},
          {"kind": "words", "n": FULL, "seed": 11}]),
        ("clamav2000", orc.clamav_file(2000, tmp), True, -1,
         [{"kind": "clamav", "n": 1 << 20, "seed": 7, "n_plant": 256},
          {"kind": "clamav", "n": FULL, "seed": 7, "n_plant": 4096},
          {"kind": "repeat", "n": 1 << 20, "pattern": 5},
          {"kind": "zeros", "n": 1 << 20}]),
        ("clamav2000_m12", orc.clamav_file(2000, tmp), True, 12,
         [{"kind": "clamav", "n": FULL, "seed": 7, "n_plant": 4096}]),
        ("clamav10000", orc.clamav_file(10000, tmp), True, -1,
         [{"kind": "clamav", "n": FULL, "seed": 9, "n_plant": 4096}]),
        ("clamav15000", orc.clamav_file(15000, tmp), True, -1,
         [{"kind": "clamav", "n": 1 << 20, "seed": 8, "n_plant": 256},
          {"kind": "clamav", "n": FULL, "seed": 8, "n_plant": 4096}]),
        ("clamav15000_m12", orc.clamav_file(15000, tmp), True, 12,
         [{"kind": "clamav", "n": FULL, "seed": 8, "n_plant": 4096}]),
    ]
    out = {"generator": "tests/golden/make_golden.py", "source": "reference acsmx.c via oracle/_ref",
           "sets": {}}
    for name, path, hex_, max_len, texts in sets:
        print("==", name, flush=True)
        r, pats = ref_and_patterns(path, hex_, max_len)
        entry = {
            "hex": hex_, "max_len": max_len,
            "patterns": len(pats),
            "states": r.num_states,
            "max_pattern_len": r.max_pattern_len,
            "texts": [],
        }
        if r.num_states <= 100000:
            entry["table_digest"] = "%016x" % orc.table_digest(r.table())
        for spec in texts:
            t = text_for(spec, pats)
            pos, pat, fs = r.scan(t)
            rec = dict(spec)
            rec.update({
                "sha256": hashlib.sha256(t.tobytes()).hexdigest(),
                "count": int(pos.size),
                "records_digest": "%016x" % orc.records_digest(pos, pat),
                "final_state": int(fs),
                "first_records": [[int(a), int(b)] for a, b in zip(pos[:8], pat[:8])],
            })
            entry["texts"].append(rec)
            print("   ", spec, "->", pos.size, "records, final", fs, flush=True)
        out["sets"][name] = entry
    with open(os.path.join(HERE, "golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote golden.json")


COMPILED_SETS = ["tests", "tests1", "tests3", "sentiment", "clamav2000_m12"]
HEX_SAMPLES = ["00ff10", "deadBEEF", "0a0B0c0D", "7f"]


def match_lists_sha256(obj, nstates):
    """sha256 over the match lists of every (nstates // 2000)-th state, as the test samples them."""
    h = hashlib.sha256()
    for s in range(0, nstates, max(1, nstates // 2000)):
        h.update(json.dumps(obj.match_list(s)).encode() + b"\n")
    return h.hexdigest()


def compiled():
    import fixtures
    out = {"generator": "tests/golden/make_golden.py compiled", "source": "reference acsmx.c via oracle/_ref",
           "hex_to_bytes": {h: orc.RefAcsmx().hex_to_bytes(h).hex() for h in HEX_SAMPLES}, "sets": {}}
    for name in COMPILED_SETS:
        o = fixtures.oracle_for(name)
        r = orc.RefAcsmx()
        for b, iid in o.patterns():
            r.add(b, iid)
        r.compile()
        table = np.ascontiguousarray(r.table(), dtype=np.int32)
        rng = np.random.default_rng(5)
        text = fixtures.text_for({"kind": "clamav", "n": 1 << 16, "seed": 5, "n_plant": 64}, fixtures.patterns_of(name))
        init = int(rng.integers(0, r.num_states))
        pos, pat, fs = r.scan(text, init)
        # all-patterns walk: every pattern of the reference's match list of the state entered at each hit
        flat = table.reshape(-1, 512)
        exp_pos, exp_pat, state = [], [], init
        for k, c in enumerate(text[:1 << 14]):
            nxt = int(flat[state, c])
            if nxt < 0:
                nxt = -nxt
                for p in r.match_list(nxt):
                    exp_pos.append(k)
                    exp_pat.append(p)
            state = nxt
        out["sets"][name] = {
            "states": r.num_states, "max_pattern_len": r.max_pattern_len,
            "table_sha256": hashlib.sha256(table.tobytes()).hexdigest(),
            "match_lists_sha256": match_lists_sha256(r, r.num_states),
            "init_state": init,
            "scan": {"count": int(pos.size), "records_digest": "%016x" % orc.records_digest(pos, pat), "final_state": int(fs)},
            "walk": {"count": len(exp_pos), "final_state": state,
                     "records_digest": "%016x" % orc.records_digest(np.array(exp_pos, dtype=np.uint32),
                                                                     np.array(exp_pat, dtype=np.int32))},
        }
        print("==", name, out["sets"][name]["states"], "states", flush=True)
    with open(os.path.join(HERE, "compiled_reference.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote compiled_reference.json")


if __name__ == "__main__":
    compiled() if sys.argv[1:] == ["compiled"] else main()
