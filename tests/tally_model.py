"""Match tallies in numpy (test infrastructure only): what acm_tally_matches_async must give for a list of
(offset, pattern) entries, a class per pattern and an attribution grid of segment starts."""
import numpy as np


def tally(offs, pats, class_of, num_classes, starts=None):
    """(class_total uint64[C], seg_class int32[S, C] or None, lead int32[C]).  class_of None: the identity.
    An entry whose class is outside [0, C) counts nowhere; an entry at offset o belongs to the last k with
    starts[k] <= o, one in front of starts[0] to the lead."""
    pats = np.asarray(pats, dtype=np.int64)
    cls = pats if class_of is None else np.asarray(class_of, dtype=np.int64)[pats]
    ok = (cls >= 0) & (cls < num_classes)
    cls, offs = cls[ok], np.asarray(offs, dtype=np.int64)[ok]
    total = np.bincount(cls, minlength=num_classes).astype(np.uint64)
    lead = np.zeros(num_classes, dtype=np.int32)
    if starts is None or len(starts) == 0:
        return total, None, lead
    k = np.searchsorted(np.asarray(starts, dtype=np.int64), offs, side="right") - 1
    rows = np.zeros((len(starts), num_classes), dtype=np.int32)
    np.add.at(rows, (k[k >= 0], cls[k >= 0]), 1)
    np.add.at(lead, cls[k < 0], 1)
    return total, rows, lead
