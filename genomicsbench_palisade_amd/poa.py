"""Partial order alignment and window consensus (include/gb_bsw_poa.h): ctypes mirror of gb_poa_*."""
from __future__ import annotations

import ctypes

import numpy as np

from . import check, lib

MAX_LEN, MAX_NODES = 65536, 1048576
SW, NW, OV = 0, 1, 2
LINEAR, AFFINE, CONVEX = 0, 1, 2
CLASS_WAVE, CLASS_GROUP, CLASS_LONG = 0, 1, 2
WAVE_MAX_LEN, GROUP_MAX_LEN = 256, 1024


def size_class(seq_len):
    """The fill kernel's size class of a sequence length."""
    return CLASS_WAVE if seq_len <= WAVE_MAX_LEN else CLASS_GROUP if seq_len <= GROUP_MAX_LEN else CLASS_LONG


NEG_INF = -(1 << 31) + 1024

PARAMS_DTYPE = np.dtype([(f, "i1") for f in ("m", "n", "g", "e", "q", "c", "type", "pad")])
ITEM_DTYPE = np.dtype([("node_off", "<i8"), ("edge_off", "<i8"), ("seq_off", "<i8"), ("n_nodes", "<i4"),
                       ("n_edges", "<i4"), ("seq_len", "<i4"), ("pad", "<i4")])
assert PARAMS_DTYPE.itemsize == 8 and ITEM_DTYPE.itemsize == 40

BENCH = (2, -4, -6, -2, -25, -1)  # the benchmark's own setting: -o 4,24 -e 2,1, convex


class _Graphs(ctypes.Structure):
    _fields_ = [("node_base", ctypes.c_void_p), ("node_id", ctypes.c_void_p), ("node_out", ctypes.c_void_p),
                ("in_end", ctypes.c_void_p), ("pred_rank", ctypes.c_void_p), ("n_nodes", ctypes.c_int64),
                ("n_edges", ctypes.c_int64)]


def _decl():
    L = lib()
    if getattr(L, "_poa_decl", False):
        return L
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.gb_poa_subtype.argtypes = [vp, vp]
    L.gb_poa_item_bytes.argtypes = [i32, i32, i32]
    L.gb_poa_item_bytes.restype = i64
    L.gb_poa_align.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, i64, vp, vp]
    L.gb_poa_consensus.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    L.gb_poa_timing.argtypes = [vp, vp, vp, vp]
    L.gb_poa_plan.argtypes = [vp, vp]
    L._poa_decl = True
    return L


def _buf(a):
    return a.ctypes.data if len(a) else None


def params(m=BENCH[0], n=BENCH[1], g=BENCH[2], e=None, q=None, c=None, type=NW):
    """A gb_poa_params record with spoa's defaults for the shorter forms: e = g, then q = g and c = e."""
    e = g if e is None else e
    q = g if q is None else q
    c = e if c is None else c
    p = np.zeros(1, PARAMS_DTYPE)
    p[0] = (m, n, g, e, q, c, type, 0)
    return p


def subtype(p):
    """LINEAR, AFFINE or CONVEX, by spoa's rule."""
    p = np.ascontiguousarray(p, PARAMS_DTYPE)
    s = ctypes.c_int32(-1)
    check(_decl().gb_poa_subtype(p.ctypes.data, ctypes.addressof(s)), "gb_poa_subtype")
    return s.value


def item_bytes(sub, n_nodes, seq_len):
    """An item's share of the device workspace."""
    return int(_decl().gb_poa_item_bytes(int(sub), int(n_nodes), int(seq_len)))


class View:
    """A graph in rank order: base (u8), id (i32), out (u8), in_end (i32) per node, pred (i32) per in-edge."""

    def __init__(self, base, id, out, in_end, pred):
        self.base = np.ascontiguousarray(base, np.uint8)
        self.id = np.ascontiguousarray(id, np.int32)
        self.out = np.ascontiguousarray(out, np.uint8)
        self.in_end = np.ascontiguousarray(in_end, np.int32)
        self.pred = np.ascontiguousarray(pred, np.int32)

    @property
    def n(self):
        return len(self.base)


class Batch:
    """The arrays of gb_poa_align for a list of (View, sequence bytes) items."""

    def __init__(self, views, seqs):
        def cat(parts, dt):
            return np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)

        seqs = [np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, np.uint8)
                for s in seqs]
        self.base = cat([v.base for v in views], np.uint8)
        self.id = cat([v.id for v in views], np.int32)
        self.out = cat([v.out for v in views], np.uint8)
        self.in_end = cat([v.in_end for v in views], np.int32)
        self.pred = cat([v.pred for v in views], np.int32)
        self.seqs = cat(seqs, np.uint8)
        self.items = np.zeros(len(views), ITEM_DTYPE)
        no = eo = so = 0
        for k, (v, s) in enumerate(zip(views, seqs)):
            self.items[k] = (no, eo, so, v.n, len(v.pred), len(s), 0)
            no, eo, so = no + v.n, eo + len(v.pred), so + len(s)

    def need(self):
        it = self.items
        live = (it["n_nodes"] > 0) & (it["seq_len"] > 0)
        return int((it["n_nodes"].astype(np.int64) + it["seq_len"])[live].sum())


def align_raw(p, b, pair_cap=None, scores=None, pairs=None, pair_off=None, items=None, n_nodes=None, n_edges=None,
              seq_bytes=None):
    """gb_poa_align as it is: (status, scores, pair buffer, pair_off, pair_used). No exception. The buffers the
    call writes are new ones by default (scores of -7, pairs of -9, pair_off of -1; pair_used starts as -1), so
    that a refusal can be seen to leave them untouched. `items`, `n_nodes`, `n_edges` and `seq_bytes` replace the
    batch's own, for the refusals."""
    L = _decl()
    p = np.ascontiguousarray(p, PARAMS_DTYPE)
    items = b.items if items is None else np.ascontiguousarray(items, ITEM_DTYPE)
    cap = b.need() if pair_cap is None else int(pair_cap)
    if scores is None:
        scores = np.full(len(items), -7, np.int32)
    if pairs is None:
        pairs = np.full(2 * max(cap, 0), -9, np.int32)
    if pair_off is None:
        pair_off = np.full(len(items) + 1, -1, np.int64)
    g = _Graphs(_buf(b.base), _buf(b.id), _buf(b.out), _buf(b.in_end), _buf(b.pred),
                len(b.base) if n_nodes is None else n_nodes, len(b.pred) if n_edges is None else n_edges)
    used = ctypes.c_int64(-1)
    st = L.gb_poa_align(p.ctypes.data, ctypes.addressof(g), _buf(b.seqs), len(b.seqs) if seq_bytes is None else seq_bytes,
                        _buf(items), len(items), _buf(scores), _buf(pairs), cap, pair_off.ctypes.data,
                        ctypes.addressof(used))
    return st, scores, pairs, pair_off, used.value


def align(p, views, seqs):
    """SisdAlignmentEngine::align of every (view, sequence): (scores, pairs as an (n, 2) array, pair_off)."""
    st, scores, pairs, off, used = align_raw(p, Batch(views, seqs))
    check(st, "gb_poa_align")
    return scores, pairs[:2 * used].reshape(-1, 2), off


def pack_windows(windows, quals=None):
    """(win_off, seq_off, bytes, weights or None) of a list of windows, each a list of byte strings; quals, if
    given, has the same shape and turns into spoa's weights (quality byte - 33)."""
    win_off, seq_off, parts, wparts = [0], [0], [], []
    for w, reads in enumerate(windows):
        for k, r in enumerate(reads):
            parts.append(np.frombuffer(bytes(r), np.uint8))
            seq_off.append(seq_off[-1] + len(r))
            if quals is not None:
                qv = np.frombuffer(bytes(quals[w][k]), np.uint8)
                assert len(qv) == len(r)
                wparts.append((qv.astype(np.int64) - 33).astype(np.uint32))
        win_off.append(win_off[-1] + len(reads))
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    wt = None if quals is None else (np.concatenate(wparts) if wparts else np.zeros(0, np.uint32))
    return np.asarray(win_off, np.int64), np.asarray(seq_off, np.int64), data, wt


def consensus_raw(p, win_off, seq_off, data, weights=None, cons_cap=None, cons=None, cons_off=None, node_count=None,
                  n_seqs=None, n_bytes=None):
    """gb_poa_consensus as it is: (status, cons buffer, cons_off, cons_used, node_count, n_alignments)."""
    L = _decl()
    p = np.ascontiguousarray(p, PARAMS_DTYPE)
    win_off, seq_off = np.ascontiguousarray(win_off, np.int64), np.ascontiguousarray(seq_off, np.int64)
    data = np.ascontiguousarray(data, np.uint8)
    nw = len(win_off) - 1
    cap = int(seq_off[-1] - seq_off[0]) if cons_cap is None else int(cons_cap)
    if cons is None:
        cons = np.full(max(cap, 0), 0x21, np.uint8)
    if cons_off is None:
        cons_off = np.full(nw + 1, -1, np.int64)
    if node_count is None:
        node_count = np.full(nw, -7, np.int32)
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.uint32)
    used, done = ctypes.c_int64(-1), ctypes.c_int64(-1)
    st = L.gb_poa_consensus(p.ctypes.data, win_off.ctypes.data, nw, seq_off.ctypes.data,
                            len(seq_off) - 1 if n_seqs is None else n_seqs, _buf(data),
                            len(data) if n_bytes is None else n_bytes, None if weights is None else _buf(weights),
                            _buf(cons), cap, cons_off.ctypes.data, ctypes.addressof(used), _buf(node_count),
                            ctypes.addressof(done))
    return st, cons, cons_off, used.value, node_count, done.value


def consensus(p, windows, quals=None):
    """The heaviest-bundle consensus of every window: (list of bytes, node counts, alignments done)."""
    win_off, seq_off, data, wt = pack_windows(windows, quals)
    st, cons, off, used, nodes, done = consensus_raw(p, win_off, seq_off, data, wt)
    check(st, "gb_poa_consensus")
    return [cons[off[w]:off[w + 1]].tobytes() for w in range(len(windows))], nodes, done


def timing():
    """(fill ms, walk ms, host ms, cells) of this thread's last align or consensus."""
    f, w, h, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float(), ctypes.c_int64()
    check(_decl().gb_poa_timing(ctypes.addressof(f), ctypes.addressof(w), ctypes.addressof(h), ctypes.addressof(c)),
          "gb_poa_timing")
    return f.value, w.value, h.value, c.value


def plan():
    """(chunks, largest chunk's workspace bytes) of this thread's last align or consensus."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(_decl().gb_poa_plan(ctypes.addressof(a), ctypes.addressof(b)), "gb_poa_plan")
    return a.value, b.value
