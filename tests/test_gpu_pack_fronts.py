"""The glue at a block's front, in both instantiations of the range-packing core (acm_extract_async, acm_format_async):
the place kernel decides it from the block summaries of the sum kernel, the last block in front that has a used range.
3 * 1024 + 8 cells are four blocks of the record grid, a tile of 1024 cells each; all cells but four are skipped, so
whole blocks of skipped cells lie between two used ranges.  Every call runs from poisoned buffers and is compared whole
with its model; the extract and the format pass with every range a head are compared with each other on the device."""
import numpy as np
import pytest

import extract_model as xm
import format_model as fm
import ops_guard as og
from gpu_pattern_matching_amd import DeviceArray
from test_gpu_extract import Extract, random_text, upload_text
from test_gpu_extract import run as extract_run
from test_gpu_format import ALL, Format
from test_gpu_format import run as format_run

pytestmark = pytest.mark.gpu

TILE_CELLS, MAX_BLOCKS = 1024, 1024          # record_pass.h: kTile, kMaxBlocks
CELLS = 3 * TILE_CELLS + 8
TEXT = random_text(4096, 31, newline=0)          # no range ends in the terminator
GLUE = b"--\n"
SEL_HEAD = fm.SELECTED | fm.HEAD
NAMES = [b"", b"first/file", b"second"]       # text id 0: what lies in front of the first start


def test_the_grid_has_four_blocks_of_one_tile():
    """grid_for and share_of (record_pass.h) for CELLS cells: block j owns the cells [1024 j, 1024 (j + 1))"""
    tiles = (CELLS + TILE_CELLS - 1) // TILE_CELLS
    blocks = max(1, min(tiles, MAX_BLOCKS))
    per = (tiles + blocks - 1) // blocks
    assert (tiles, blocks, per) == (4, 4, 1)


def planes(used):
    """begin and end cells of CELLS ranges: used = {cell: (begin, bytes)}, every other cell skipped (a poison begin)"""
    b, e = np.full(CELLS, og.FILL32, dtype=np.int64), np.zeros(CELLS, dtype=np.int64)
    for cell, (at, k) in used.items():
        assert 1 <= k <= 20
        b[cell], e[cell] = at, at + k
    return b, e


def both_passes(lib, dt, used, seg, later_head, what):
    """the extract and the format pass (flags 0 and all, the later range a head or not) over the used ranges, each against
    its model; then the extract against the format pass with every range a head, on the device.  Returns the extract's
    model dict."""
    b, e = planes(used)
    ex = extract_run(lib, TEXT, b, e, glue=GLUE, term=0x0A, seg=seg, d_text=dt, what=what)
    cells = sorted(used)
    for head in (True, False):
        kinds = np.full(CELLS, og.FILL32, dtype=np.int64)     # (the kind of a skipped range is not looked at)
        kinds[cells] = SEL_HEAD
        kinds[later_head] = SEL_HEAD if head else fm.SELECTED
        for flags in (0, ALL):
            full = format_run(lib, TEXT, b, e, flags, kinds=kinds, nums=np.arange(CELLS), nbase=1, names=NAMES[:len(seg) + 1],
                              glue=GLUE, term=0x0A, seg=seg, seg_num=[5] * len(seg), d_text=dt,
                              what="%s, flags %d, head %d" % (what, flags, head))
            if head and flags == 0:
                for k in ("out", "m", "at"):
                    assert full[k] == ex[k], "%s: the two models differ in %s" % (what, k)
                assert full["info"].tolist() == ex["info"].tolist() and full["seg_out"].tolist() == ex["seg_out"].tolist()
    # the two instantiations, from the same device planes
    dev = [DeviceArray.from_numpy(xm.plane_of(p), pad_to=0) for p in (b, e, np.full(CELLS, SEL_HEAD))]
    cap, at_cap = ex["m"] + 37, len(cells) + 5
    x = Extract(lib, dt, len(TEXT), dev[0], dev[1], CELLS, cap, glue=GLUE, term=0x0A, at_cap=at_cap, seg=seg).read(what)
    f = Format(lib, dt, len(TEXT), dev[0], dev[1], CELLS, cap, kind=dev[2], glue=GLUE, term=0x0A, at_cap=at_cap,
               seg=seg).read(what)
    for k in x:
        assert np.array_equal(x[k], f[k]), "%s: the extract and the format pass of heads differ in %s" % (what, k)
    for d in dev:
        d.free()
    return ex


@pytest.mark.parametrize("shift", (0, 5))
@pytest.mark.parametrize("block", (1, 2, 3))
def test_a_front_behind_skipped_cells(gpu, lib, block, shift):
    """a used range in the last cell of block 0, the next one in block `block`: block - 1 whole blocks of skipped cells
    between them, and `shift` skipped cells at the front of its own block"""
    later = block * TILE_CELLS + shift
    used = {3: (40, 9), TILE_CELLS - 1: (100, 7), later: (300, 13), later + 2: (330, 20)}
    dt = upload_text(TEXT)
    for seg, same_text in (([30], True), ([30, 200], False)):
        ex = both_passes(lib, dt, used, seg, later, "block %d + %d, %d starts" % (block, shift, len(seg)))
        # the second and fourth range always follow one of their text; the third does iff no start lies between
        want = TEXT[40:49] + b"\n" + GLUE + TEXT[100:107] + b"\n" + (GLUE if same_text else b"") + TEXT[300:313] + b"\n" + \
            GLUE + TEXT[330:350] + b"\n"
        assert ex["out"] == want and ex["info"][0] == 4
    dt.free()


@pytest.mark.parametrize("shift", (0, 5))
def test_no_glue_behind_blocks_without_a_used_range(gpu, lib, shift):
    """nothing used in block 0 (and in block 1): the first used range of the call is a block's front and has no glue"""
    dt = upload_text(TEXT)
    for block in (1, 2):
        later = block * TILE_CELLS + shift
        used = {later: (300, 13), later + 2: (330, 20)}
        ex = both_passes(lib, dt, used, [30], later, "nothing in front of block %d + %d" % (block, shift))
        assert ex["out"] == TEXT[300:313] + b"\n" + GLUE + TEXT[330:350] + b"\n" and ex["at"] == [0, 14 + len(GLUE)]
    dt.free()
