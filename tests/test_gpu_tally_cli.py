"""acm_grep -c: exact counts per file and per pattern, tallied on the device.  A worker's files are one
stream; the counts are those of tests/tally_model.py over the records the oracle (or the word model) gives
for that stream, a record belonging to the file that holds its last byte.  Buffers are smaller than the
files, file sizes are no multiples of -B, and -R is small, so the bucket planes drop records while the
counts stay exact."""
import os
import re

import numpy as np
import pytest

import fixtures
import word_model as wm
from tally_model import tally
from test_gpu_acm_grep import CLI, run
from test_gpu_words_cli import write_files
from test_host_segments import oracle_segments

pytestmark = pytest.mark.gpu

FILE_LINE = re.compile(r"^Count file '(.*)': (\d+)$", re.M)
PAT_LINE = re.compile(r"^Count pattern (-?\d+) \('(.*)'\): (\d+)$", re.M)

CASES = {   # flags, text mode
    "plain": ([], False), "A": (["-A"], False), "S": (["-S"], False), "t-S": (["-t", "-S"], True),
    "W": (["-W"], False), "i": (["-i"], False), "W-A-S": (["-W", "-A", "-S"], False),
}


def records(model, folded, stream, bounds, flags):
    """(offsets, patterns) of the records a worker reports for its stream"""
    starts = None
    if "-S" in flags:
        s = set(bounds[:-1].tolist())
        if "-t" in flags:
            s |= set((np.flatnonzero(stream == ord("\n")) + 1).tolist())
        starts = np.array(sorted(x for x in s if x < stream.size), dtype=np.int64)
    if "-W" in flags:
        return model.words(stream, wm.DEFAULT, "-A" in flags, starts=starts)[:2]
    m = folded if "-i" in flags else model
    t = wm.FOLD[stream] if "-i" in flags else stream
    if "-A" in flags:
        return m.scan_all(t, starts=starts)[:2]
    if starts is not None:
        return oracle_segments(m.o, t, starts)[:2]
    return m.o.scan(t)[:2]


@pytest.mark.parametrize("workers", [1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_counts(gpu, tmp_path, case, workers):
    flags, text_mode = CASES[case]
    name = "sentiment"
    model, folded = wm.WordModel(name), wm.WordModel(name, True)
    path, _, _ = fixtures.set_source(name)
    files = write_files(tmp_path, model, "-i" in flags, 5)
    B = 256 if text_mode else 64
    args = ["-f", ",".join(p for p, _ in files), "-p", path, "-B", str(B), "-D", "0", "-G", "16", "-L", "64",
            "-w", str(workers), "-R", "3"] + flags
    per_file = {}
    per_pat = np.zeros(len(model.pats), dtype=np.uint64)
    for w in range(workers):
        mine = files[w::workers]
        stream = np.concatenate([t for _, t in mine])
        bounds = np.cumsum([0] + [t.size for _, t in mine])
        offs, pats = records(model, folded, stream, bounds, flags)
        total, rows, lead = tally(offs, pats, np.zeros(len(model.pats), np.int32), 1, bounds[:-1])
        assert not lead.any()
        for (p, _), n in zip(mine, rows[:, 0].tolist()):
            per_file[p] = n
        per_pat += tally(offs, pats, None, len(model.pats))[0]
    _, stats, out = run(CLI, args + ["-c"])
    got_files = FILE_LINE.findall(out)
    assert got_files == [(p, str(per_file[p])) for p, _ in files]
    iids = [iid for _, iid in model.o.patterns()]
    want = [(str(iids[i]), model.pats[i].decode(), str(int(per_pat[i]))) for i in range(len(model.pats)) if per_pat[i]]
    assert PAT_LINE.findall(out) == want
    assert int(stats["Matches"]) == sum(per_file.values()) == int(per_pat.sum()) > 1000
    assert int(stats["Kernel launches"]) > 10        # files straddle the buffers
    if not text_mode:
        assert int(stats["Matches reported"]) < int(stats["Matches"])   # -R 3: the bucket planes drop records
    assert out.index("Count file") < out.index("-------------- STATS")
    _, _, plain_out = run(CLI, args)
    assert "Count" not in plain_out
    assert out.replace("\r", "").count("\n") > plain_out.count("\n")
