"""The launch recorder of the GPU tests: what a call launched, read from the library's dispatch record."""
import torch

from semantichuman_amd import _lib


def launches(fn):
    """fn() with the dispatch record on -> (its result, the ordered list of (kernel name, shape tag) it launched).  The record is
    switched off again whatever fn does."""
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        rec = [(k, tag) for k, tag, _ in _lib.profile_records_by_kernel()]
    finally:
        _lib.profile_enable(False)
    return out, rec


def recorded(fn):
    """fn() with the dispatch record on -> (its result, the set of kernel names it launched)."""
    out, rec = launches(fn)
    return out, {k for k, _ in rec}


def launch_counts(fn):
    """fn() with the dispatch record on -> (its result, kernel name -> how often it was launched)."""
    out, rec = launches(fn)
    names = [k for k, _ in rec]
    return out, {k: names.count(k) for k in set(names)}
