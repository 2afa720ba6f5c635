"""De Bruijn graph assembly of regions (include/gb_fmi_dbg.h): ctypes mirror of gb_dbg_*, and the region loop of the
reference's driver (windows)."""
from __future__ import annotations

import bisect
import ctypes

import numpy as np

from . import check, lib

MAX_K = 64
MAX_EDGES = 536870911
DEFAULTS = (15, 5, 50, 20, 40)  # k0, k_step, k_max, min_qual, min_weight

SUMMARY = np.dtype([("k", "<i4"), ("n_graphs", "<i4"), ("cyclic", "<i4"), ("n_nodes", "<i4"), ("n_edges", "<i4"),
                    ("n_ref_and_read", "<i4"), ("redone", "<i4"), ("reserved", "<i4"), ("node_weight_sum", "<i8"),
                    ("edge_weight_sum", "<i8")])
GRAPH_FIELDS = ("src", "off", "colours", "position", "weight", "n_edges", "edge_to", "edge_weight")


def _decl():
    L = lib()
    if getattr(L, "_dbg_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_dbg_assemble.argtypes = [vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, ctypes.c_int, vp]
    L.gb_dbg_free.argtypes = [vp]
    L.gb_dbg_free.restype = None
    L.gb_dbg_summary.argtypes = [vp, vp, i64]
    L.gb_dbg_export.argtypes = [vp, i64, i64] + [vp] * 9
    L.gb_dbg_timing.argtypes = [vp] * 8
    L.gb_dbg_plan.argtypes = [vp] * 4
    L._dbg_decl = True
    return L


def _buf(a):
    return a.ctypes.data if len(a) else None


def _bytes(x):
    if isinstance(x, np.ndarray):
        return np.asarray(x, np.uint8)
    return np.frombuffer(x.encode() if isinstance(x, str) else bytes(x), np.uint8)


def _csr(parts):
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    data = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    return np.ascontiguousarray(data), off


class Regions:
    """ref_bytes u8, ref_off i64[n + 1], ref_start i32[n], read_first / read_last i64[n]"""

    def __init__(self, ref_bytes, ref_off, ref_start, read_first, read_last):
        self.ref_bytes = np.ascontiguousarray(ref_bytes, np.uint8)
        self.ref_off = np.ascontiguousarray(ref_off, np.int64)
        self.ref_start = np.ascontiguousarray(ref_start, np.int32)
        self.read_first = np.ascontiguousarray(read_first, np.int64)
        self.read_last = np.ascontiguousarray(read_last, np.int64)

    def __len__(self):
        return len(self.ref_start)

    def take(self, order):
        """The regions `order`, in that order, over the same read pool."""
        order = np.asarray(order, np.int64)
        data, off = _csr([self.ref_bytes[self.ref_off[i]:self.ref_off[i + 1]] for i in order])
        return Regions(data, off, self.ref_start[order], self.read_first[order], self.read_last[order])


class Reads:
    """seq u8, qual u8, read_off i64[n + 1], flag u32[n]"""

    def __init__(self, seq, qual, read_off, flag):
        self.seq = np.ascontiguousarray(seq, np.uint8)
        self.qual = np.ascontiguousarray(qual, np.uint8)
        self.read_off = np.ascontiguousarray(read_off, np.int64)
        self.flag = np.ascontiguousarray(flag, np.uint32)
        assert len(self.seq) == len(self.qual)

    def __len__(self):
        return len(self.flag)


def pack(regions, reads):
    """(Regions, Reads) from lists: regions of (reference, ref_start, read_first, read_last), reads of
    (sequence, qualities, flag); texts are bytes, str or u8 arrays, qualities a u8 array or a list of numbers."""
    refs, off = _csr([_bytes(r[0]) for r in regions])
    seq, roff = _csr([_bytes(r[0]) for r in reads])
    qual, _ = _csr([np.asarray(r[1], np.uint8) for r in reads])
    return (Regions(refs, off, [r[1] for r in regions], [r[2] for r in regions], [r[3] for r in regions]),
            Reads(seq, qual, roff, [r[2] for r in reads]))


class Assembly:
    """A gb_dbg handle."""

    def __init__(self, regions, reads, params=DEFAULTS, keep=False):
        L = _decl()
        self.regions, self.reads, self.keep = regions, reads, bool(keep)
        self._h = ctypes.c_void_p(None)
        p = (ctypes.c_int32 * 5)(*[int(x) for x in params]) if params is not None else None
        check(L.gb_dbg_assemble(_buf(regions.ref_bytes), len(regions.ref_bytes), regions.ref_off.ctypes.data,
                                _buf(regions.ref_start), _buf(regions.read_first), _buf(regions.read_last),
                                len(regions), _buf(reads.seq), _buf(reads.qual), len(reads.seq),
                                reads.read_off.ctypes.data, _buf(reads.flag), len(reads), p, int(self.keep),
                                ctypes.byref(self._h)), "gb_dbg_assemble")

    def close(self):
        if self._h:
            _decl().gb_dbg_free(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def summary(self):
        """A structured array (SUMMARY), one entry a region."""
        out = np.zeros(len(self.regions), SUMMARY)
        check(_decl().gb_dbg_summary(self._h, _buf(out), len(out)), "gb_dbg_summary")
        return out

    def graph(self, i):
        """The final graph of region i (keep=True): a dict of GRAPH_FIELDS, edge_to and edge_weight as (n, 4)."""
        L = _decl()
        n = ctypes.c_int64(-1)
        st = L.gb_dbg_export(self._h, int(i), 0, *([None] * 8), ctypes.addressof(n))
        if not self.keep or n.value < 0:
            check(st, "gb_dbg_export")
        n = max(n.value, 0)
        g = {f: np.zeros(n, np.int32) for f in GRAPH_FIELDS}
        g["weight"], g["edge_to"] = np.zeros(n, np.int64), np.full((n, 4), -1, np.int32)
        g["edge_weight"] = np.zeros((n, 4), np.int64)
        used = ctypes.c_int64(-1)
        check(L.gb_dbg_export(self._h, int(i), n, *[_buf(g[f]) for f in GRAPH_FIELDS], ctypes.addressof(used)),
              "gb_dbg_export")
        assert used.value == n
        return g


def assemble(regions, reads, params=DEFAULTS, keep=False):
    """Regions and Reads (or lists, as pack takes them) through gb_dbg_assemble."""
    if not isinstance(regions, Regions):
        regions, reads = pack(regions, reads)
    return Assembly(regions, reads, params, keep)


def timing():
    """{pack, build, rank, edges, cycle, redo (ms), positions, valid_positions} of this thread's last call."""
    f = [ctypes.c_float(0) for _ in range(6)]
    n = [ctypes.c_int64(0) for _ in range(2)]
    check(_decl().gb_dbg_timing(*[ctypes.addressof(x) for x in f + n]), "gb_dbg_timing")
    d = dict(zip(("pack", "build", "rank", "edges", "cycle", "redo"), [x.value for x in f]))
    d["positions"], d["valid_positions"] = n[0].value, n[1].value
    return d


def plan():
    """{max_table_slots, workspace_bytes, chunks, rounds} of this thread's last call."""
    v = [ctypes.c_int64(0) for _ in range(4)]
    check(_decl().gb_dbg_plan(*[ctypes.addressof(x) for x in v]), "gb_dbg_plan")
    return dict(zip(("max_table_slots", "workspace_bytes", "chunks", "rounds"), [x.value for x in v]))


def windows(pos, end, longest, beg, stop, region=1500):
    """The reference driver's region loop over reads sorted by pos (setWindowPointers and bisectReadsLeft):
    (assem_start, ref_start, ref_end, read_first, read_last) of every region of [beg, stop). ValueError where the
    reference exits with "read start pointer > read end pointer"."""
    pos = [int(x) for x in pos]
    end = [int(x) for x in end]
    n = len(pos)
    shift = max(100, min(1000, region // 2))
    out = []
    for k in range(beg, stop, shift):
        a0, a1 = k, min(k + region, stop)
        r0, r1 = max(0, a0 - region), a1 + region
        if n == 0:
            first = last = 0
        else:
            first = bisect.bisect_left(pos, max(1, a0 - longest))
            last = bisect.bisect_left(pos, a1)
            while first < n and end[first] <= a0:
                first += 1
            if first > last:
                raise ValueError(f"region {a0}..{a1}: read start pointer {first} > read end pointer {last}")
            last = min(last, n)
        out.append((a0, r0, r1, first, last))
    return out
