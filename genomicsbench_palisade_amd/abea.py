"""Host mirror of gb_abea_align (include/gb_bsw_abea.h): adaptive banded event alignment, the batch form of f5c's
align() (benchmarks/abea/src/align.c:169-548), executed by csrc/bsw_abea.hip.

Reads are gen.AbeaReads (one model, concatenated ASCII bases and event means, per-read lengths and scalings).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import GbError, check, lib

K = 6
BANDWIDTH = 100
MAX_SEQ_LEN = 1 << 20
MAX_EVENTS = 1 << 21

READ_DTYPE = np.dtype([("seq_off", "<i8"), ("event_off", "<i8"), ("seq_len", "<i4"), ("n_events", "<i4"),
                       ("scale", "<f4"), ("shift", "<f4")])
PAIR_DTYPE = np.dtype([("ref_pos", "<i4"), ("read_pos", "<i4")])
STAT_DTYPE = np.dtype([("n_pairs", "<i4"), ("n_raw", "<i4"), ("max_gap", "<i4"), ("spanned", "<i4"),
                       ("end_event", "<i4"), ("no_end_cell", "<i4"), ("fills", "<i4"), ("pad", "<i4"),
                       ("end_score", "<f4"), ("pad2", "<f4"), ("sum_emission", "<f8")])
assert READ_DTYPE.itemsize == 32 and PAIR_DTYPE.itemsize == 8 and STAT_DTYPE.itemsize == 48


def _decl():
    L = lib()
    if getattr(L, "_abea_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_abea_align.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, vp]
    L.gb_abea_align_timing.argtypes = [vp, vp, vp]
    L.gb_abea_align_plan.argtypes = [vp, vp, vp]
    L._abea_decl = True
    return L


def _buf(a):
    return a.ctypes.data if len(a) else None


def read_records(reads):
    """gb_abea_read records of a gen.AbeaReads."""
    rd = np.zeros(reads.n, READ_DTYPE)
    for f in ("seq_off", "event_off", "seq_len", "n_events", "scale", "shift"):
        rd[f] = getattr(reads, f)
    return rd


def align_raw(model, seqs, events, records, pair_cap):
    """gb_abea_align as it is: (status, pairs buffer, pair_off, stats, pairs_used). No exception."""
    L = _decl()
    model = np.ascontiguousarray(model, np.float32)
    n = len(records)
    pairs = np.zeros(max(int(pair_cap), 0), PAIR_DTYPE)
    off = np.zeros(n + 1, np.int64)
    stats = np.zeros(n, STAT_DTYPE)
    used = ctypes.c_int64(-1)
    st = L.gb_abea_align(_buf(model), _buf(seqs), len(seqs), _buf(events), len(events), _buf(records), n, _buf(pairs),
                         int(pair_cap), off.ctypes.data, _buf(stats), ctypes.addressof(used))
    return st, pairs, off, stats, used.value


def align(reads, pair_cap=None):
    """Aligns every read: (pairs, pair_off, stats). Read r owns pairs[pair_off[r]:pair_off[r + 1]] (its
    stats["n_raw"] pairs before the QC, in the reference's final order); stats["n_pairs"] is align()'s return
    value, 0 where the QC fails."""
    cap = reads.pair_cap() if pair_cap is None else pair_cap
    st, pairs, off, stats, used = align_raw(reads.model, reads.seqs, reads.events, read_records(reads), cap)
    check(st, "gb_abea_align")
    return pairs[:used], off, stats


def timing():
    """(fill ms, walk ms, cells) of this thread's last device call."""
    f, t, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_int64()
    check(_decl().gb_abea_align_timing(ctypes.addressof(f), ctypes.addressof(t), ctypes.addressof(c)),
          "gb_abea_align_timing")
    return f.value, t.value, c.value


def plan():
    """(chunks, waves, workspace bytes) of this thread's last device call."""
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    check(_decl().gb_abea_align_plan(ctypes.addressof(a), ctypes.addressof(b), ctypes.addressof(c)),
          "gb_abea_align_plan")
    return a.value, b.value, c.value


__all__ = ["GbError", "align", "align_raw", "plan", "read_records", "timing"]
