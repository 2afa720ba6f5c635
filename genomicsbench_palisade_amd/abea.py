"""Host mirror of gb_abea_align (include/gb_bsw_abea.h): adaptive banded event alignment, the batch form of f5c's
align() (benchmarks/abea/src/align.c:169-548), executed by csrc/bsw_abea.hip.

Reads are gen.AbeaReads (one model, concatenated ASCII bases and event means, per-read lengths and scalings).

Below it, the mirror of gb_abea_hmm_score (include/gb_bsw_abea_hmm.h): the methylation profile-HMM scores, the
batch form of profile_hmm_score (src/hmm.c:620-727), executed by csrc/bsw_abea_hmm.hip over gen.AbeaHmmItems.

Last, the mirror of gb_abea_hmm_align (include/gb_bsw_abea_viterbi.h): Viterbi event alignment with traceback, the
batch form of profile_hmm_align (src/eventalign.c:703-911), executed by csrc/bsw_abea_viterbi.hip over
gen.AbeaAlignItems.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import GbError, check, lib
from .gen import ABEA_HMM_ITEM_DTYPE, ABEA_HMM_READ_DTYPE

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


# ---- gb_abea_hmm_score (include/gb_bsw_abea_hmm.h): methylation profile-HMM scores, csrc/bsw_abea_hmm.hip ----

HMM_MODEL_SIZE = 15625
HMM_MAX_KMERS = 256
HMM_MAX_EVENTS = 65536
HMM_LOGSUM_TBL = 16000
HMM_READ_DTYPE = ABEA_HMM_READ_DTYPE
HMM_ITEM_DTYPE = ABEA_HMM_ITEM_DTYPE


def _hmm_decl():
    L = lib()
    if getattr(L, "_abea_hmm_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_abea_hmm_score.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp]
    L.gb_abea_hmm_timing.argtypes = [vp, vp]
    L.gb_abea_hmm_logsum_table.argtypes = [vp]
    L._abea_hmm_decl = True
    return L


def hmm_score_raw(model, seqs, events, reads, items, scores=None):
    """gb_abea_hmm_score as it is: (status, scores). No exception. `scores` is the buffer the call writes (a new
    one of NaN by default), so that a refusal can be seen to leave it untouched."""
    L = _hmm_decl()
    model = np.ascontiguousarray(model, np.float32)
    seqs = np.ascontiguousarray(seqs, np.uint8)
    events = np.ascontiguousarray(events, np.float32)
    reads = np.ascontiguousarray(reads, HMM_READ_DTYPE)
    items = np.ascontiguousarray(items, HMM_ITEM_DTYPE)
    if scores is None:
        scores = np.full(len(items), np.nan, np.float32)
    st = L.gb_abea_hmm_score(_buf(model), _buf(seqs), len(seqs), _buf(events), len(events), _buf(reads), len(reads),
                             _buf(items), len(items), _buf(scores))
    return st, scores


def hmm_score(x):
    """profile_hmm_score of every item of a gen.AbeaHmmItems: float32 [n], bit for bit the reference's."""
    st, scores = hmm_score_raw(x.model, x.seqs, x.events, x.reads, x.items)
    check(st, "gb_abea_hmm_score")
    return scores


def hmm_timing():
    """(kernel ms, cells) of this thread's last device call of hmm_score."""
    ms, c = ctypes.c_float(), ctypes.c_int64()
    check(_hmm_decl().gb_abea_hmm_timing(ctypes.addressof(ms), ctypes.addressof(c)), "gb_abea_hmm_timing")
    return ms.value, c.value


def hmm_logsum_table():
    """The 16 000 entries of the p7_FLogsum table the library built."""
    t = np.zeros(HMM_LOGSUM_TBL, np.float32)
    check(_hmm_decl().gb_abea_hmm_logsum_table(t.ctypes.data), "gb_abea_hmm_logsum_table")
    return t


# ---- gb_abea_hmm_align (include/gb_bsw_abea_viterbi.h): Viterbi alignment with traceback, csrc/bsw_abea_viterbi.hip ----

HMM_ALIGN_MODEL_SIZE = 4096
HMM_PATH_DTYPE = np.dtype([("event_idx", "<i4"), ("kmer_idx", "<i4"), ("l_fm", "<f4"), ("state", "S1"), ("pad", "u1", (3,))])
assert HMM_PATH_DTYPE.itemsize == 16


def _hmm_align_decl():
    L = lib()
    if getattr(L, "_abea_hmm_align_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_abea_hmm_align.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]
    L.gb_abea_hmm_align_timing.argtypes = [vp, vp, vp]
    L.gb_abea_hmm_align_plan.argtypes = [vp, vp]
    L._abea_hmm_align_decl = True
    return L


def hmm_align_need(items):
    """The path_cap the call asks for: rows + k-mers - 1 summed over HMM_ITEM_DTYPE records."""
    items = np.asarray(items, HMM_ITEM_DTYPE)
    rows = np.abs(items["event_stop"].astype(np.int64) - items["event_start"]) + 1
    return int((rows + items["seq_len"].astype(np.int64) - K).sum())


def hmm_align_raw(model, seqs, events, reads, items, path_cap=None, path=None, path_off=None):
    """gb_abea_hmm_align as it is: (status, path buffer, path_off, path_used). No exception. `path` and
    `path_off` are the buffers the call writes (new ones by default, path_off of -1), so that a refusal can be
    seen to leave them untouched; path_used starts as -1."""
    L = _hmm_align_decl()
    model = np.ascontiguousarray(model, np.float32)
    seqs = np.ascontiguousarray(seqs, np.uint8)
    events = np.ascontiguousarray(events, np.float32)
    reads = np.ascontiguousarray(reads, HMM_READ_DTYPE)
    items = np.ascontiguousarray(items, HMM_ITEM_DTYPE)
    cap = hmm_align_need(items) if path_cap is None else int(path_cap)
    if path is None:
        path = np.zeros(max(cap, 0), HMM_PATH_DTYPE)
    if path_off is None:
        path_off = np.full(len(items) + 1, -1, np.int64)
    used = ctypes.c_int64(-1)
    st = L.gb_abea_hmm_align(_buf(model), _buf(seqs), len(seqs), _buf(events), len(events), _buf(reads), len(reads),
                             _buf(items), len(items), _buf(path), cap, path_off.ctypes.data, ctypes.addressof(used))
    return st, path, path_off, used.value


def hmm_align(x):
    """profile_hmm_align of every item of a gen.AbeaAlignItems: (records, path_off). Item i owns
    records[path_off[i]:path_off[i + 1]], HMM_PATH_DTYPE, in the reference's final order and bit for bit its."""
    st, path, off, used = hmm_align_raw(x.model, x.seqs, x.events, x.reads, x.items)
    check(st, "gb_abea_hmm_align")
    return path[:used], off


def hmm_align_timing():
    """(fill ms, walk ms, cells) of this thread's last device call of hmm_align."""
    f, w, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_int64()
    check(_hmm_align_decl().gb_abea_hmm_align_timing(ctypes.addressof(f), ctypes.addressof(w), ctypes.addressof(c)),
          "gb_abea_hmm_align_timing")
    return f.value, w.value, c.value


def hmm_align_plan():
    """(chunks, largest chunk's workspace bytes) of this thread's last device call of hmm_align."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(_hmm_align_decl().gb_abea_hmm_align_plan(ctypes.addressof(a), ctypes.addressof(b)), "gb_abea_hmm_align_plan")
    return a.value, b.value


__all__ = ["GbError", "HMM_PATH_DTYPE", "align", "align_raw", "hmm_align", "hmm_align_need", "hmm_align_plan",
           "hmm_align_raw", "hmm_align_timing", "hmm_logsum_table", "hmm_score", "hmm_score_raw", "hmm_timing", "plan",
           "read_records", "timing"]
