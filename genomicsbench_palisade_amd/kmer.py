"""K-mer counting and the solid k-mer index (include/gb_fmi_kmer.h): ctypes mirror of gb_kmer_*."""
from __future__ import annotations

import ctypes

import numpy as np

from . import check, lib

MAX_K = 31
TILE = 4096


def _decl():
    L = lib()
    if getattr(L, "_kmer_decl", False):
        return L
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    L.gb_kmer_count.argtypes = [ctypes.c_int, vp, i64, vp, i64, vp]
    L.gb_kmer_free.argtypes = [vp]
    L.gb_kmer_free.restype = None
    L.gb_kmer_counts_stats.argtypes = [vp, vp, vp, vp, vp]
    L.gb_kmer_counts_export.argtypes = [vp, vp, vp, i64, vp]
    L.gb_kmer_counts_freq.argtypes = [vp, vp, i64, vp]
    L.gb_kmer_counts_hist.argtypes = [vp, vp, i64]
    L.gb_kmer_index.argtypes = [vp, i32, f32, i32, f32, vp]
    L.gb_kmer_idx_free.argtypes = [vp]
    L.gb_kmer_idx_free.restype = None
    L.gb_kmer_idx_stats.argtypes = [vp, vp, vp, vp, vp]
    L.gb_kmer_idx_export.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64]
    L.gb_kmer_timing.argtypes = [vp] * 8
    L.gb_kmer_plan.argtypes = [vp, vp, vp]
    L._kmer_decl = True
    return L


def _buf(a):
    return a.ctypes.data if len(a) else None


def pack_reads(reads):
    """(bytes u8, seq_off i64) of a list of reads (bytes, str or u8 arrays)."""
    parts = [np.frombuffer(r.encode() if isinstance(r, str) else bytes(r), np.uint8) if not isinstance(r, np.ndarray)
             else np.asarray(r, np.uint8) for r in reads]
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    data = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    return np.ascontiguousarray(data), off


class Index:
    """The index of one gb_kmer_index call: codes (u64, ascending), off (i64, n + 1), pos (i64 global positions),
    rep_codes (u64, ascending), repetitive_frequency."""

    def __init__(self, codes, off, pos, rep_codes, repetitive_frequency):
        self.codes, self.off, self.pos, self.rep_codes = codes, off, pos, rep_codes
        self.repetitive_frequency = repetitive_frequency


class Counts:
    """A resident gb_kmer_counts handle."""

    def __init__(self, k, data, off):
        L = _decl()
        self.data = np.ascontiguousarray(data, np.uint8)
        self.seq_off = np.ascontiguousarray(off, np.int64)
        self.k = int(k)
        self._h = ctypes.c_void_p(None)
        check(L.gb_kmer_count(self.k, _buf(self.data), len(self.data), self.seq_off.ctypes.data,
                              len(self.seq_off) - 1, ctypes.byref(self._h)), "gb_kmer_count")

    def close(self):
        if self._h:
            _decl().gb_kmer_free(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        """{n_distinct, n_occurrences, n_over15, max_count}"""
        v = [ctypes.c_int64(-1) for _ in range(4)]
        check(_decl().gb_kmer_counts_stats(self._h, *[ctypes.addressof(x) for x in v]), "gb_kmer_counts_stats")
        return dict(zip(("n_distinct", "n_occurrences", "n_over15", "max_count"), [x.value for x in v]))

    def export(self):
        """(codes u64 ascending, counts u32)"""
        n = self.stats()["n_distinct"]
        codes, counts, used = np.zeros(n, np.uint64), np.zeros(n, np.uint32), ctypes.c_int64(-1)
        check(_decl().gb_kmer_counts_export(self._h, _buf(codes), _buf(counts), n, ctypes.addressof(used)),
              "gb_kmer_counts_export")
        assert used.value == n
        return codes, counts

    def freq(self, codes):
        codes = np.ascontiguousarray(codes, np.uint64)
        out = np.zeros(len(codes), np.uint32)
        check(_decl().gb_kmer_counts_freq(self._h, _buf(codes), len(codes), _buf(out)), "gb_kmer_counts_freq")
        return out

    def hist(self, n_bins):
        out = np.zeros(n_bins, np.int64)
        check(_decl().gb_kmer_counts_hist(self._h, out.ctypes.data, n_bins), "gb_kmer_counts_hist")
        return out

    def index(self, min_freq=1, select_rate=0.4, tandem_freq=0, repeat_rate=100.0):
        L = _decl()
        x = ctypes.c_void_p(None)
        check(L.gb_kmer_index(self._h, int(min_freq), float(select_rate), int(tandem_freq), float(repeat_rate),
                              ctypes.byref(x)), "gb_kmer_index")
        try:
            v = [ctypes.c_int64(-1) for _ in range(4)]
            check(L.gb_kmer_idx_stats(x, *[ctypes.addressof(y) for y in v]), "gb_kmer_idx_stats")
            nc, ne, nr, rf = [y.value for y in v]
            codes, off, pos = np.zeros(nc, np.uint64), np.zeros(nc + 1, np.int64), np.zeros(ne, np.int64)
            rep = np.zeros(nr, np.uint64)
            # ctypes passes None for an empty array, which the call takes as "skip": off is never empty
            codes_arg = codes if nc else np.zeros(1, np.uint64)
            check(L.gb_kmer_idx_export(x, codes_arg.ctypes.data, off.ctypes.data, nc, _buf(pos), ne, _buf(rep), nr),
                  "gb_kmer_idx_export")
            return Index(codes, off, pos, rep, rf)
        finally:
            L.gb_kmer_idx_free(x)


def count(k, reads):
    """Counts of a list of reads, or of (bytes u8, seq_off i64)."""
    if isinstance(reads, tuple):
        return Counts(k, *reads)
    return Counts(k, *pack_reads(reads))


def freq(counts, codes):
    return counts.freq(codes)


def hist(counts, n_bins):
    return counts.hist(n_bins)


def index(counts, min_freq=1, select_rate=0.4, tandem_freq=0, repeat_rate=100.0):
    return counts.index(min_freq, select_rate, tandem_freq, repeat_rate)


def locate(seq_off, pos):
    """Global positions to (read, strand, offset): strand 0 is the forward read, 1 its reverse complement."""
    seq_off = np.asarray(seq_off, np.int64)
    pos = np.asarray(pos, np.int64)
    base = 2 * (seq_off - seq_off[0])
    length = np.diff(seq_off)
    read = np.searchsorted(base, pos, side="right") - 1
    within = pos - base[read]
    strand = (within >= length[read]).astype(np.int64)
    return read, strand, within - strand * length[read]


def timing():
    """{pack, extract, sort, reduce, lookup, select, fill (ms), occurrences} of this thread's last calls."""
    f = [ctypes.c_float(0) for _ in range(7)]
    n = ctypes.c_int64(0)
    check(_decl().gb_kmer_timing(*[ctypes.addressof(x) for x in f], ctypes.addressof(n)), "gb_kmer_timing")
    d = dict(zip(("pack", "extract", "sort", "reduce", "lookup", "select", "fill"), [x.value for x in f]))
    d["occurrences"] = n.value
    return d


def plan():
    """(tile in keys, sort passes, workspace bytes)"""
    v = [ctypes.c_int64(0) for _ in range(3)]
    check(_decl().gb_kmer_plan(*[ctypes.addressof(x) for x in v]), "gb_kmer_plan")
    return tuple(x.value for x in v)
