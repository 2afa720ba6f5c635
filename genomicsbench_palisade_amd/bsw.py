"""Host mirror of the reference banded-SW interface (BandedPairWiseSW::getScores16 over SeqPair,
benchmarks/bsw/bandedSWA.h:92-101,120-124,195-200), executed by csrc/bsw.hip.

Pairs are gen.BswPairs (flattened target/query buffers, SeqPair.idr/idq = offsets into them).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import check, lib

# SeqPair (bandedSWA.h:92-101) == gb_seqpair (include/gb_bsw.h), 72 bytes
SEQPAIR_DTYPE = np.dtype([("idr", "<i8"), ("idq", "<i8"), ("id", "<i8"), ("len1", "<i4"), ("len2", "<i4"),
                          ("h0", "<i4"), ("seqid", "<i4"), ("regid", "<i4"), ("score", "<i4"), ("tle", "<i4"),
                          ("gtle", "<i4"), ("qle", "<i4"), ("gscore", "<i4"), ("max_off", "<i4"),
                          ("_pad", "<i4")])
assert SEQPAIR_DTYPE.itemsize == 72

# out6 order used by the C ABI, the oracle and the reference shim
OUT_FIELDS = ("score", "qle", "tle", "gtle", "gscore", "max_off")


class Params(ctypes.Structure):
    """gb_bsw_params: BandedPairWiseSW constructor arguments + getScores16's w."""
    _fields_ = [("o_del", ctypes.c_int32), ("e_del", ctypes.c_int32), ("o_ins", ctypes.c_int32),
                ("e_ins", ctypes.c_int32), ("zdrop", ctypes.c_int32), ("end_bonus", ctypes.c_int32),
                ("w", ctypes.c_int32), ("mat", ctypes.c_int8 * 25)]

    def as_array(self):
        """{o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w} as the oracle takes them."""
        return np.array([self.o_del, self.e_del, self.o_ins, self.e_ins, self.zdrop, self.end_bonus, self.w],
                        np.int32)

    def mat_array(self):
        return np.array(list(self.mat), np.int8)


def fill_scmat(a=1, b=4, ambig=-1):
    """bwa_fill_scmat (main_banded.cpp:77-88)."""
    m = np.full((5, 5), ambig, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(-1)


def default_params(**kw):
    """The benchmark's settings (main_banded.cpp:53-57,846): 1/4/-1, gaps 6+1, zdrop 100, end_bonus 5, w 100."""
    p = Params(6, 1, 6, 1, 100, 5, 100)
    mat = kw.pop("mat", None)
    if mat is None:
        mat = fill_scmat(kw.pop("match", 1), kw.pop("mismatch", 4), kw.pop("ambig", -1))
    for k, v in kw.items():
        setattr(p, k, int(v))
    for k in range(25):
        p.mat[k] = int(mat[k])
    return p


def seqpairs(pairs):
    """SeqPair records for a BswPairs set, ids batch-local like loadPairs (main_banded.cpp:177-197)."""
    sp = np.zeros(pairs.n, SEQPAIR_DTYPE)
    sp["idr"], sp["idq"], sp["id"] = pairs.toff, pairs.qoff, np.arange(pairs.n)
    sp["len1"], sp["len2"], sp["h0"] = pairs.tlen, pairs.qlen, pairs.h0
    for f in ("seqid", "regid", "score", "tle", "gtle", "qle", "gscore", "max_off"):
        sp[f] = -1
    return sp


def _decl():
    L = lib()
    if getattr(L, "_bsw_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_bsw_batch_create.argtypes = [vp, vp, i64, vp, i64, vp, i64, ctypes.POINTER(vp)]
    L.gb_bsw_batch_run.argtypes = [vp]
    L.gb_bsw_batch_sync.argtypes = [vp]
    L.gb_bsw_batch_results.argtypes = [vp, vp, vp, vp, vp]
    L.gb_bsw_batch_timing.argtypes = [vp, vp]
    L.gb_bsw_batch_destroy.argtypes = [vp]
    L.gb_bsw_get_scores16.argtypes = [vp, vp, i64, vp, i64, vp, i64]
    L.gb_bsw_default_params.argtypes = [vp]
    L._bsw_decl = True
    return L


def _buf(a):
    return a.ctypes.data if len(a) else None


class BswBatch:
    """Pairs resident on the current device; run() extends them all (one kernel launch)."""

    def __init__(self, pairs, params=None):
        L = _decl()
        self.pairs = pairs
        self.params = params if params is not None else default_params()
        self._sp = seqpairs(pairs)
        self.h = ctypes.c_void_p()
        check(L.gb_bsw_batch_create(ctypes.byref(self.params), _buf(self._sp), pairs.n, _buf(pairs.tgt),
                                    len(pairs.tgt), _buf(pairs.qry), len(pairs.qry), ctypes.byref(self.h)),
              "gb_bsw_batch_create")

    def run(self):
        check(_decl().gb_bsw_batch_run(self.h), "gb_bsw_batch_run")

    def sync(self):
        check(_decl().gb_bsw_batch_sync(self.h), "gb_bsw_batch_sync")

    def results(self, want_cells=True):
        """(out6 int32 [n,6] = score,qle,tle,gtle,gscore,max_off; cells int32 [n] or None; total cells)."""
        n = self.pairs.n
        out6 = np.zeros((max(n, 1), 6), np.int32)
        cells = np.zeros(max(n, 1), np.int32) if want_cells else None
        tot = ctypes.c_int64()
        check(_decl().gb_bsw_batch_results(self.h, None, out6.ctypes.data,
                                           cells.ctypes.data if want_cells else None, ctypes.byref(tot)),
              "gb_bsw_batch_results")
        return out6[:n], (cells[:n] if want_cells else None), tot.value

    def timing(self):
        ms = ctypes.c_float()
        check(_decl().gb_bsw_batch_timing(self.h, ctypes.byref(ms)), "gb_bsw_batch_timing")
        return ms.value

    def close(self):
        if self.h:
            _decl().gb_bsw_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def get_scores16(pairs, params=None):
    """One-shot getScores16: returns the SeqPair array with score/tle/gtle/qle/gscore/max_off filled."""
    params = params if params is not None else default_params()
    sp = seqpairs(pairs)
    check(_decl().gb_bsw_get_scores16(ctypes.byref(params), _buf(sp), pairs.n, _buf(pairs.tgt), len(pairs.tgt),
                                      _buf(pairs.qry), len(pairs.qry)), "gb_bsw_get_scores16")
    return sp


def get_scores8(pairs, params=None, w_match: int = 1):
    """One-shot getScores8 (the 8-bit path's domain only: len1, len2 < 128, h0 + min(len1, len2) *
    w_match < 128, bwamem.cpp:2152-2155; raises GbError for any other pair)."""
    params = params if params is not None else default_params()
    sp = seqpairs(pairs)
    L = _decl()
    L.gb_bsw_get_scores8.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    check(L.gb_bsw_get_scores8(ctypes.byref(params), w_match, _buf(sp), pairs.n, _buf(pairs.tgt), len(pairs.tgt),
                               _buf(pairs.qry), len(pairs.qry), None), "gb_bsw_get_scores8")
    return sp


# ---- banded global alignment with CIGAR traceback (ksw_global2, tools/bwa/ksw.c:504-606) ----------

# gb_bsw_gpair (include/gb_bsw.h), 48 bytes
GPAIR_DTYPE = np.dtype([("idr", "<i8"), ("idq", "<i8"), ("len1", "<i4"), ("len2", "<i4"), ("w", "<i4"),
                        ("score", "<i4"), ("n_cigar", "<i4"), ("nm", "<i4"), ("cigar_off", "<i8")])
assert GPAIR_DTYPE.itemsize == 48
GLOBAL_MAX_TLEN = 2047
CIGAR_OPS = "MID"  # op codes 0, 1, 2 of ksw_global2's len << 4 | op


def _decl_global():
    L = _decl()
    if getattr(L, "_bsw_global_decl", False):
        return L
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.gb_bsw_global.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp]
    L.gb_bsw_global_band.argtypes = [vp, i32, i32, i32]
    L.gb_bsw_global_timing.argtypes = [vp, vp]
    L._bsw_global_decl = True
    return L


def gpairs(pairs, w):
    """gb_bsw_gpair records for a BswPairs set; w is one band half-width or one per pair."""
    gp = np.zeros(pairs.n, GPAIR_DTYPE)
    gp["idr"], gp["idq"] = pairs.toff, pairs.qoff
    gp["len1"], gp["len2"] = pairs.tlen, pairs.qlen
    gp["w"] = w
    for f in ("score", "n_cigar", "nm", "cigar_off"):
        gp[f] = -1
    return gp


def global_align(pairs, w, params=None, want_cigar=True):
    """ksw_global2 for every pair of a BswPairs set (h0 is ignored) with band half-width w (scalar or
    per pair): (score, n_cigar, nm, cigar_off, cigar) as numpy arrays; pair p's operations are
    cigar[cigar_off[p] : cigar_off[p] + n_cigar[p]], each len << 4 | op with M = 0, I = 1, D = 2.
    want_cigar=False asks for scores only: n_cigar 0, nm -1, an empty cigar."""
    params = params if params is not None else default_params()
    gp = gpairs(pairs, w)
    cap = int(pairs.tlen.astype(np.int64).sum() + pairs.qlen.astype(np.int64).sum()) if want_cigar else 0
    cigar = np.zeros(max(cap, 1), np.uint32)
    used = ctypes.c_int64(0)
    check(_decl_global().gb_bsw_global(ctypes.byref(params), _buf(gp), pairs.n, _buf(pairs.tgt), len(pairs.tgt),
                                       _buf(pairs.qry), len(pairs.qry), cigar.ctypes.data if want_cigar else None,
                                       cap, ctypes.byref(used)), "gb_bsw_global")
    return (gp["score"].copy(), gp["n_cigar"].copy(), gp["nm"].copy(), gp["cigar_off"].copy(),
            cigar[:used.value].copy())


def global_timing():
    """(fill_ms, walk_ms): device time of this thread's last global_align, summed over its chunks."""
    a, b = ctypes.c_float(), ctypes.c_float()
    check(_decl_global().gb_bsw_global_timing(ctypes.byref(a), ctypes.byref(b)), "gb_bsw_global_timing")
    return a.value, b.value


def global_band(len2, len1, w_cap=100, params=None):
    """bwa_gen_cigar2's band half-width (bwa.c:151-160) for a query of len2 against a target of len1;
    w_cap is its w_ argument. Scalars give an int, arrays an int32 array."""
    params = params if params is not None else default_params()
    L = _decl_global()

    def one(q, t):
        w = L.gb_bsw_global_band(ctypes.byref(params), int(q), int(t), int(w_cap))
        check(min(w, 0), "gb_bsw_global_band")
        return w
    if np.ndim(len2) == 0 and np.ndim(len1) == 0:
        return one(len2, len1)
    q, t = np.broadcast_arrays(np.asarray(len2), np.asarray(len1))
    # the rule depends on (len2, len1) only: evaluate each distinct pair of lengths once
    key = q.astype(np.int64) * 4096 + t.astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    vals = np.array([one(k // 4096, k % 4096) for k in uniq.tolist()], np.int32)
    return vals[inv].reshape(q.shape)


def cigar_string(ops):
    """'30M1D29M' for an array of len << 4 | op."""
    return "".join(f"{int(o) >> 4}{CIGAR_OPS[int(o) & 15]}" for o in ops)


# ---- unbanded local alignment with sub-optimal score and start (ksw_align2, tools/bwa/ksw.c:63-365) ----

# gb_bsw_lpair (include/gb_bsw.h), 56 bytes
LPAIR_DTYPE = np.dtype([("idr", "<i8"), ("idq", "<i8"), ("len1", "<i4"), ("len2", "<i4"), ("xtra", "<i4"),
                        ("score", "<i4"), ("te", "<i4"), ("qe", "<i4"), ("score2", "<i4"), ("te2", "<i4"),
                        ("tb", "<i4"), ("qb", "<i4")])
assert LPAIR_DTYPE.itemsize == 56
LOCAL_FIELDS = ("score", "te", "qe", "score2", "te2", "tb", "qb")  # kswr_t's order
LOCAL_MAX_TLEN = 16383
# tools/bwa/ksw.h:6-9; the low 16 bits of xtra are the XSUBO / XSTOP threshold
KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000


def _decl_local():
    L = _decl()
    if getattr(L, "_bsw_local_decl", False):
        return L
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.gb_bsw_local.argtypes = [vp, vp, i64, vp, i64, vp, i64]
    L.gb_bsw_local_xtra.argtypes = [vp, i32, i32]
    L.gb_bsw_local_timing.argtypes = [vp]
    L._bsw_local_decl = True
    return L


def lpairs(pairs, xtra):
    """gb_bsw_lpair records for a BswPairs set; xtra is one value or one per pair."""
    lp = np.zeros(pairs.n, LPAIR_DTYPE)
    lp["idr"], lp["idq"] = pairs.toff, pairs.qoff
    lp["len1"], lp["len2"] = pairs.tlen, pairs.qlen
    lp["xtra"] = xtra
    for f in LOCAL_FIELDS:
        lp[f] = -1
    return lp


def local_align(pairs, xtra, params=None):
    """ksw_align2 for every pair of a BswPairs set (h0 is ignored) under xtra = KSW_X* flags |
    threshold (scalar or per pair): (score, te, qe, score2, te2, tb, qb) as int32 arrays."""
    params = params if params is not None else default_params()
    lp = lpairs(pairs, xtra)
    check(_decl_local().gb_bsw_local(ctypes.byref(params), _buf(lp), pairs.n, _buf(pairs.tgt), len(pairs.tgt),
                                     _buf(pairs.qry), len(pairs.qry)), "gb_bsw_local")
    return tuple(lp[f].copy() for f in LOCAL_FIELDS)


def local_xtra(len2, min_seed_len=19, params=None):
    """mem_matesw's xtra (bwamem_pair.c:150) for a mate of len2 bases: XSUBO | XSTART | (len2 * a < 250
    ? XBYTE : 0) | min_seed_len * a with a = mat[0]. A scalar gives an int, an array an int32 array."""
    params = params if params is not None else default_params()
    L = _decl_local()

    def one(q):
        x = L.gb_bsw_local_xtra(ctypes.byref(params), int(q), int(min_seed_len))
        check(min(x, 0), "gb_bsw_local_xtra")
        return x
    if np.ndim(len2) == 0:
        return one(len2)
    q = np.asarray(len2)
    uniq, inv = np.unique(q, return_inverse=True)
    return np.array([one(k) for k in uniq.tolist()], np.int32)[inv].reshape(q.shape)


def local_timing():
    """Kernel ms of this thread's last local_align, summed over its chunks."""
    a = ctypes.c_float()
    check(_decl_local().gb_bsw_local_timing(ctypes.byref(a)), "gb_bsw_local_timing")
    return a.value


# ---- CIGAR, NM and MD from reference coordinates (bwa_gen_cigar2, tools/bwa/bwa.c:121-208) ----------

# gb_bsw_cpair (include/gb_bsw.h), 64 bytes
CPAIR_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("idq", "<i8"), ("len2", "<i4"), ("w", "<i4"), ("score", "<i4"),
                        ("n_cigar", "<i4"), ("nm", "<i4"), ("md_len", "<i4"), ("cigar_off", "<i8"), ("md_off", "<i8")])
assert CPAIR_DTYPE.itemsize == 64
CIGAR_FIELDS = ("score", "n_cigar", "nm", "md_len", "cigar_off", "md_off")


def _decl_gencigar():
    L = _decl_global()
    if getattr(L, "_bsw_gencigar_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_ref_create.argtypes = [vp, i64, ctypes.POINTER(vp)]
    L.gb_ref_load_pac.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.gb_ref_info.argtypes = [vp, vp]
    L.gb_ref_destroy.argtypes = [vp]
    L.gb_ref_fetch.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp]
    L.gb_bsw_gen_cigar.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp]
    L.gb_bsw_gen_cigar_retry.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp]
    L.gb_bsw_gen_cigar_timing.argtypes = [vp, vp, vp, vp]
    L._bsw_gencigar_decl = True
    return L


def pack_pac(codes):
    """bwa's 2-bit packing of base codes 0..3: base l in byte l >> 2 at shift (~l & 3) << 1 (_set_pac,
    tools/bwa/bntseq.c:42)."""
    c = np.asarray(codes, np.uint8)
    if len(c) < 1 or (c > 3).any():
        raise ValueError("a packed reference holds at least one base, codes 0..3 only")
    c4 = np.zeros((len(c) + 3) // 4 * 4, np.uint8)
    c4[:len(c)] = c
    c4 = c4.reshape(-1, 4)
    return (c4[:, 0] << 6 | c4[:, 1] << 4 | c4[:, 2] << 2 | c4[:, 3]).astype(np.uint8)


class Ref:
    """gb_ref: a packed reference, uploaded to the current device by the first call that uses it."""

    def __init__(self, handle):
        self.h = handle
        n = ctypes.c_int64()
        check(_decl_gencigar().gb_ref_info(self.h, ctypes.byref(n)), "gb_ref_info")
        self.l_pac = n.value

    @classmethod
    def from_pac(cls, pac, l_pac):
        """From (l_pac + 3) // 4 packed bytes in bwa's layout."""
        pac = np.ascontiguousarray(pac, np.uint8)
        if len(pac) < (int(l_pac) + 3) // 4:
            raise ValueError("pac is shorter than (l_pac + 3) // 4 bytes")
        h = ctypes.c_void_p()
        check(_decl_gencigar().gb_ref_create(pac.ctypes.data, int(l_pac), ctypes.byref(h)), "gb_ref_create")
        return cls(h)

    @classmethod
    def from_codes(cls, codes):
        """From base codes 0..3, one per byte (packed here with numpy)."""
        return cls.from_pac(pack_pac(codes), len(codes))

    @classmethod
    def from_pac_file(cls, path):
        """From a bwa .pac file."""
        h = ctypes.c_void_p()
        check(_decl_gencigar().gb_ref_load_pac(os.fsencode(path), ctypes.byref(h)), "gb_ref_load_pac")
        return cls(h)

    def fetch(self, beg, end):
        """bns_get_seq for every region (beg[r], end[r]) of the doubled coordinate space: (bytes uint8,
        off int64 [n], len int32 [n]); region r is bytes[off[r] : off[r] + len[r]]."""
        beg = np.ascontiguousarray(np.atleast_1d(beg), np.int64)
        end = np.ascontiguousarray(np.atleast_1d(end), np.int64)
        n = len(beg)
        off, ln = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
        # an upper bound on the total without repeating the clamps: |end - beg| per region
        cap = int(np.minimum(np.abs(end - beg), 2 * self.l_pac).sum())
        out = np.zeros(max(cap, 1), np.uint8)
        check(_decl_gencigar().gb_ref_fetch(self.h, _buf(beg), _buf(end), n, out.ctypes.data, cap, off.ctypes.data,
                                            ln.ctypes.data), "gb_ref_fetch")
        return out[:int(ln[:n].sum())].copy(), off[:n], ln[:n]

    def close(self):
        if self.h:
            _decl_gencigar().gb_ref_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cpairs(queries, rb, re, w):
    """(gb_bsw_cpair records, flat query buffer) for a list of uint8 code arrays and their regions; w is
    one value or one per pair. The out fields start at -1."""
    n = len(queries)
    cp = np.zeros(n, CPAIR_DTYPE)
    ql = np.array([len(q) for q in queries], np.int64)
    cp["rb"], cp["re"], cp["len2"], cp["w"] = rb, re, ql, w
    cp["idq"] = np.concatenate([[0], np.cumsum(ql)[:-1]]) if n else 0
    for f in CIGAR_FIELDS:
        cp[f] = -1
    qbuf = np.concatenate([np.asarray(q, np.uint8) for q in queries]) if n else np.zeros(0, np.uint8)
    return cp, np.ascontiguousarray(qbuf)


def md_cap(rb, re):
    """GB_BSW_MD_CAP summed over the regions: the md capacity that always suffices."""
    d = np.abs(np.asarray(re, np.int64) - np.asarray(rb, np.int64))
    return int((3 * d + 1).sum())


def _gen_cigar_call(fn, what, ref, queries, rb, re, w, params, want_cigar, want_md, truesc=None):
    params = params if params is not None else default_params()
    if want_md and not want_cigar:
        raise ValueError("MD needs the CIGAR: want_md requires want_cigar")
    cp, qbuf = cpairs(queries, rb, re, w)
    d = np.abs(cp["re"] - cp["rb"])
    ccap = int((d + cp["len2"]).sum()) if want_cigar else 0
    mcap = md_cap(cp["rb"], cp["re"]) if want_md else 0
    cigar, md = np.zeros(max(ccap, 1), np.uint32), np.zeros(max(mcap, 1), np.uint8)
    cu, mu = ctypes.c_int64(0), ctypes.c_int64(0)
    args = [ctypes.byref(params), ref.h, _buf(cp), len(cp), _buf(qbuf), len(qbuf)]
    tries = None
    if truesc is not None:
        ts = np.ascontiguousarray(truesc, np.int32)
        tries = np.zeros(max(len(cp), 1), np.int32)
        args.append(_buf(ts))
    args += [cigar.ctypes.data if want_cigar else None, ccap, ctypes.byref(cu),
             md.ctypes.data if want_md else None, mcap, ctypes.byref(mu)]
    if truesc is not None:
        args.append(tries.ctypes.data)
    check(fn(*args), what)
    res = {f: cp[f].copy() for f in CIGAR_FIELDS}
    res["w"] = cp["w"].copy()
    res["cigar"] = cigar[:cu.value].copy()
    res["md"] = md[:mu.value].tobytes()
    if tries is not None:
        res["tries"] = tries[:len(cp)]
    return res


def gen_cigar(ref, queries, rb, re, w, params=None, want_cigar=True, want_md=True):
    """bwa_gen_cigar2 for every (query, region [rb, re) of ref's doubled coordinate space, w). Returns a
    dict: score, n_cigar, nm, md_len, cigar_off, md_off (arrays, one entry per pair), cigar (uint32,
    len << 4 | op) and md (bytes); pair p owns cigar[cigar_off[p] : cigar_off[p] + n_cigar[p]] and
    md[md_off[p] : md_off[p] + md_len[p]]. A pair the reference rejects has n_cigar 0, nm -1, md_len 0
    and score -1 (the value this wrapper starts from). want_cigar=False asks for scores only."""
    return _gen_cigar_call(_decl_gencigar().gb_bsw_gen_cigar, "gb_bsw_gen_cigar", ref, queries, rb, re, w, params,
                           want_cigar, want_md)


def gen_cigar_retry(ref, queries, rb, re, w, truesc, params=None, want_cigar=True, want_md=True):
    """gen_cigar inside mem_reg2aln's re-banding loop (tools/bwa/bwamem.c:1154-1163): the same dict plus
    w (each pair's band argument on its last try) and tries."""
    return _gen_cigar_call(_decl_gencigar().gb_bsw_gen_cigar_retry, "gb_bsw_gen_cigar_retry", ref, queries, rb, re, w,
                           params, want_cigar, want_md, truesc=truesc)


def gen_cigar_timing():
    """(fetch_ms, fill_ms, walk_ms, md_ms): device time of this thread's last gen_cigar / gen_cigar_retry."""
    t = [ctypes.c_float() for _ in range(4)]
    check(_decl_gencigar().gb_bsw_gen_cigar_timing(*[ctypes.byref(x) for x in t]), "gb_bsw_gen_cigar_timing")
    return tuple(x.value for x in t)


# ---- seed extension from chains (mem_chain2aln, tools/bwa/bwamem.c:632-824) ----------

# gb_bsw_seed (mem_seed_t), gb_bsw_region and gb_bsw_c2a_raw (include/gb_bsw.h)
SEED_DTYPE = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4"), ("score", "<i4"), ("_pad", "<i4")])
REGION_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"),
                         ("truesc", "<i4"), ("w", "<i4"), ("seedcov", "<i4"), ("seedlen0", "<i4"), ("chain", "<i4"),
                         ("seed", "<i4"), ("_pad", "<i4")])
C2A_RAW_DTYPE = np.dtype([("out6", "<i4", (2, 6)), ("tries", "<i4", (2,)), ("skipped", "<i4"), ("_pad", "<i4")])
assert SEED_DTYPE.itemsize == 24 and REGION_DTYPE.itemsize == 56 and C2A_RAW_DTYPE.itemsize == 64
REGION_FIELDS = ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov", "seedlen0", "chain", "seed")


def _decl_chain2aln():
    L = _decl_gencigar()
    if getattr(L, "_bsw_c2a_decl", False):
        return L
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.gb_bsw_chain2aln.argtypes = [vp, i32, i32, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.gb_bsw_chain2aln_timing.argtypes = [vp, vp, vp, vp]
    L._bsw_c2a_decl = True
    return L


def chain_csr(queries, chains):
    """The three CSR levels of gb_bsw_chain2aln for a list of uint8 code arrays and, per read, a list of
    chains, each a list of seeds (rbeg, qbeg, len, score): (qbuf, idq, l_query, read_chain_off,
    chain_seed_off, seeds)."""
    n = len(queries)
    ql = np.array([len(q) for q in queries], np.int64)
    idq = np.concatenate([[0], np.cumsum(ql)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    qbuf = np.concatenate([np.asarray(q, np.uint8) for q in queries]) if n else np.zeros(0, np.uint8)
    rco = np.zeros(n + 1, np.int64)
    rco[1:] = np.cumsum([len(c) for c in chains])
    flat = [c for rc in chains for c in rc]
    cso = np.zeros(len(flat) + 1, np.int64)
    cso[1:] = np.cumsum([len(c) for c in flat])
    seeds = np.zeros(int(cso[-1]), SEED_DTYPE)
    rows = [s for c in flat for s in c]
    if rows:
        a = np.array(rows, np.int64).reshape(-1, 4)
        seeds["rbeg"], seeds["qbeg"], seeds["len"], seeds["score"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return np.ascontiguousarray(qbuf), idq, ql.astype(np.int32), rco, cso, seeds


def chain2aln_csr(ref, qbuf, idq, l_query, read_chain_off, chain_seed_off, seeds, params=None, pen_clip5=5,
                  pen_clip3=5, contig_end=None, want_raw=True, reg_cap=None):
    """gb_bsw_chain2aln on CSR arrays (see chain_csr). Returns a dict: regs (REGION_DTYPE, packed in read
    order), reg_off, n_reg (per read), raw (C2A_RAW_DTYPE per seed, or None). reg_cap defaults to the
    number of seeds, which always suffices."""
    params = params if params is not None else default_params()
    qbuf = np.ascontiguousarray(qbuf, np.uint8)
    idq = np.ascontiguousarray(idq, np.int64)
    l_query = np.ascontiguousarray(l_query, np.int32)
    rco = np.ascontiguousarray(read_chain_off, np.int64)
    cso = np.ascontiguousarray(chain_seed_off, np.int64)
    seeds = np.ascontiguousarray(seeds, SEED_DTYPE)
    n = len(idq)
    ce = None if contig_end is None else np.ascontiguousarray(contig_end, np.int64)
    cap = len(seeds) if reg_cap is None else int(reg_cap)
    regs = np.zeros(max(cap, 1), REGION_DTYPE)
    reg_off, n_reg = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
    raw = np.zeros(max(len(seeds), 1), C2A_RAW_DTYPE) if want_raw else None
    used = ctypes.c_int64(0)
    check(_decl_chain2aln().gb_bsw_chain2aln(
        ctypes.byref(params), int(pen_clip5), int(pen_clip3), ref.h, None if ce is None else ce.ctypes.data,
        0 if ce is None else len(ce), _buf(qbuf), len(qbuf), n, _buf(idq), _buf(l_query), rco.ctypes.data,
        cso.ctypes.data, _buf(seeds), regs.ctypes.data, cap, reg_off.ctypes.data, n_reg.ctypes.data,
        ctypes.byref(used), raw.ctypes.data if want_raw else None), "gb_bsw_chain2aln")
    return {"regs": regs[:used.value].copy(), "reg_off": reg_off[:n], "n_reg": n_reg[:n],
            "raw": raw[:len(seeds)] if want_raw else None}


def chain2aln(ref, queries, chains, **kw):
    """mem_chain2aln for every read: queries is a list of uint8 code arrays, chains[r] the read's chains
    in order, each a list of seeds (rbeg, qbeg, len, score). Keywords and result as chain2aln_csr."""
    return chain2aln_csr(ref, *chain_csr(queries, chains), **kw)


def chain2aln_timing():
    """(gather_ms, ext_ms[4] = left w, left 2w, right w, right 2w, finish_ms, filter_ms): device time of this
    thread's last chain2aln, summed over its chunks; 0 for a round that launched nothing."""
    g, f, t = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    e = (ctypes.c_float * 4)()
    check(_decl_chain2aln().gb_bsw_chain2aln_timing(ctypes.byref(g), e, ctypes.byref(f), ctypes.byref(t)),
          "gb_bsw_chain2aln_timing")
    return g.value, tuple(e), f.value, t.value


# ---- chains from seeds (mem_chain after mem_collect_intv, mem_chain_flt; tools/bwa/bwamem.c:251-385) ----

# gb_bsw_mem and gb_bsw_chain_info (include/gb_bsw.h)
MEM_DTYPE = np.dtype([("read", "<i4"), ("m", "<i4"), ("n", "<i4"), ("n_coord", "<i4"), ("s", "<i8")])
CHAIN_INFO_DTYPE = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("is_alt", "<i4"), ("w", "<i4"), ("kept", "<i4"),
                             ("l_rep", "<i4"), ("frac_rep", "<f4")])
assert MEM_DTYPE.itemsize == 24 and CHAIN_INFO_DTYPE.itemsize == 32
CHAIN_INFO_FIELDS = ("pos", "rid", "is_alt", "w", "kept", "l_rep", "frac_rep")
MKCHAIN_DEV_COORDS = 65536  # GB_BSW_MKCHAIN_DEV_COORDS


class ChainOpt(ctypes.Structure):
    """gb_bsw_chain_opt: the mem_opt_t fields mem_chain and mem_chain_flt read."""
    _fields_ = [("w", ctypes.c_int32), ("max_chain_gap", ctypes.c_int32), ("max_occ", ctypes.c_int32),
                ("min_seed_len", ctypes.c_int32), ("min_chain_weight", ctypes.c_int32),
                ("max_chain_extend", ctypes.c_int32), ("mask_level", ctypes.c_float), ("drop_ratio", ctypes.c_float)]


def _decl_mkchain():
    L = _decl_chain2aln()
    if getattr(L, "_bsw_mkchain_decl", False):
        return L
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.gb_bsw_chain_default_opt.argtypes = [vp]
    L.gb_bsw_chain_default_opt.restype = None
    L.gb_bsw_seeds2chains.argtypes = [vp, i32, i64, vp, vp, i64, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, i64,
                                      vp, vp]
    L.gb_bsw_seeds2chains_timing.argtypes = [vp, vp, vp, vp]
    L._bsw_mkchain_decl = True
    return L


def chain_opt(**kw):
    """bwa's defaults (bwamem.c:50-86): w 100, max_chain_gap 10000, max_occ 500, min_seed_len 19,
    min_chain_weight 0, max_chain_extend 1 << 30, mask_level 0.5, drop_ratio 0.5; keywords override."""
    o = ChainOpt()
    _decl_mkchain().gb_bsw_chain_default_opt(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, float(v) if k in ("mask_level", "drop_ratio") else int(v))
    return o


def mems_from_smems(smems, counts):
    """gb_bsw_mem records from gb_fmi_results' structured array (fields rid, m, n, s) and the counts of
    gb_fmi_sa_entries."""
    mems = np.zeros(len(smems), MEM_DTYPE)
    mems["read"], mems["m"], mems["n"], mems["s"] = smems["rid"], smems["m"], smems["n"], smems["s"]
    mems["n_coord"] = counts
    return mems


def seeds2chains_raw(l_pac, l_query, mems, coords, opt=None, stage=1, contig_end=None, contig_is_alt=None,
                     chain_cap=None, seed_cap=None, fill=0, n_coords=None):
    """gb_bsw_seeds2chains without the status check: a dict with status, chains_used, seeds_used and the
    four output arrays at their full capacity, every byte preset to `fill` (what a refused call or a call
    with too small a cap must leave alone). n_coords overrides the coordinate count passed (the caps keep
    following len(coords)): for the refusals that look at the count alone."""
    opt = opt if opt is not None else chain_opt()
    l_query = np.ascontiguousarray(l_query, np.int32)
    mems = np.ascontiguousarray(mems, MEM_DTYPE)
    coords = np.ascontiguousarray(coords, np.int64)
    n = len(l_query)
    ce = None if contig_end is None else np.ascontiguousarray(contig_end, np.int64)
    alt = None if contig_is_alt is None else np.ascontiguousarray(contig_is_alt, np.uint8)
    ccap = len(coords) if chain_cap is None else int(chain_cap)
    scap = len(coords) if seed_cap is None else int(seed_cap)

    def out(count, dtype):
        a = np.zeros(count, dtype)
        a.view(np.uint8)[:] = fill
        return a
    rco, cso = out(n + 1, np.int64), out(ccap + 1, np.int64)
    seeds, info = out(max(scap, 1), SEED_DTYPE), out(max(ccap, 1), CHAIN_INFO_DTYPE)
    cu, su = ctypes.c_int64(-1), ctypes.c_int64(-1)
    st = _decl_mkchain().gb_bsw_seeds2chains(
        ctypes.byref(opt), int(stage), int(l_pac), None if ce is None else ce.ctypes.data,
        None if alt is None else alt.ctypes.data, 0 if ce is None else len(ce), n, _buf(l_query), _buf(mems),
        len(mems), _buf(coords), len(coords) if n_coords is None else int(n_coords), rco.ctypes.data, cso.ctypes.data, seeds.ctypes.data, info.ctypes.data,
        ccap, scap, ctypes.byref(cu), ctypes.byref(su))
    return {"status": st, "chains_used": cu.value, "seeds_used": su.value, "read_chain_off": rco,
            "chain_seed_off": cso, "seeds": seeds, "info": info}


def seeds2chains(l_pac, l_query, mems, coords, **kw):
    """gb_bsw_seeds2chains: mem_chain (stage=0) and mem_chain_flt (stage=1, the default) for every read.
    mems is a MEM_DTYPE array grouped by read (mems_from_smems), coords the coordinates in SMEM order.
    Keywords: opt (chain_opt()), stage, contig_end, contig_is_alt, chain_cap, seed_cap (the caps default to
    the number of coordinates, which always suffices). Returns a dict with the CSR arguments of
    chain2aln_csr (read_chain_off, chain_seed_off, seeds) and info (CHAIN_INFO_DTYPE per chain)."""
    r = seeds2chains_raw(l_pac, l_query, mems, coords, **kw)
    check(r["status"], "gb_bsw_seeds2chains")
    nc, ns = r["chains_used"], r["seeds_used"]
    return {"read_chain_off": r["read_chain_off"], "chain_seed_off": r["chain_seed_off"][:nc + 1],
            "seeds": r["seeds"][:ns], "info": r["info"][:nc]}


def seeds2chains_timing():
    """(build_ms, filter_ms, emit_ms, host_reads) of this thread's last seeds2chains: the device time of the
    three kernel groups (0 on the host path) and the reads that took the host path."""
    t = [ctypes.c_float() for _ in range(3)]
    h = ctypes.c_int64(0)
    check(_decl_mkchain().gb_bsw_seeds2chains_timing(*[ctypes.byref(x) for x in t], ctypes.byref(h)),
          "gb_bsw_seeds2chains_timing")
    return t[0].value, t[1].value, t[2].value, h.value


# ---- from regions to primaries (mem_sort_dedup_patch, mem_mark_primary_se, MAPQ; bwamem.c:406-558, 993-1041) ----

# gb_bsw_alnreg (include/gb_bsw.h): mem_alnreg_t's fields plus mapq
ALNREG_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8")] + [(k, "<i4") for k in (
    "qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary",
    "secondary_all", "seedlen0", "n_comp", "is_alt")] + [("frac_rep", "<f4"), ("mapq", "<i4"), ("hash", "<u8")])
assert ALNREG_DTYPE.itemsize == 96
ALNREG_FIELDS = ALNREG_DTYPE.names


class RegOpt(ctypes.Structure):
    """gb_bsw_reg_opt: the mem_opt_t fields mem_sort_dedup_patch, mem_mark_primary_se, mem_reorder_primary5 and
    mem_approx_mapq_se read."""
    _fields_ = ([(k, ctypes.c_int32) for k in "a b o_del e_del o_ins e_ins w max_chain_gap min_seed_len".split()]
                + [(k, ctypes.c_float) for k in "mask_level mask_level_redun mapQ_coef_len".split()]
                + [(k, ctypes.c_int32) for k in "mapQ_coef_fac T primary5".split()])


_REG_OPT_FLOATS = ("mask_level", "mask_level_redun", "mapQ_coef_len")


def _decl_regs():
    L = _decl_mkchain()
    if getattr(L, "_bsw_regs_decl", False):
        return L
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.gb_bsw_reg_default_opt.argtypes = [vp]
    L.gb_bsw_reg_default_opt.restype = None
    L.gb_bsw_finish_regs.argtypes = [vp, vp, i32, vp, vp, i64, vp, i64, i64, vp, vp, i64, vp, vp, vp]
    L.gb_bsw_alnreg_from_regions.argtypes = [vp, i64, vp, i64, vp]
    L.gb_bsw_finish_regs_timing.argtypes = [vp] * 6
    L._bsw_regs_decl = True
    return L


def reg_opt(**kw):
    """bwa's defaults (bwamem.c:50-86): a 1, b 4, gaps 6 / 1, w 100, max_chain_gap 10000, min_seed_len 19,
    mask_level 0.5, mask_level_redun 0.95, mapQ_coef_len 50, mapQ_coef_fac 3, T 30, primary5 0; keywords
    override."""
    o = RegOpt()
    _decl_regs().gb_bsw_reg_default_opt(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, float(v) if k in _REG_OPT_FLOATS else int(v))
    return o


def alnregs_from_regions(regions, chain_info):
    """gb_bsw_alnreg_from_regions: ALNREG_DTYPE records from gb_bsw_chain2aln's regions and
    gb_bsw_seeds2chains' info (rid and frac_rep through regions["chain"])."""
    regions = np.ascontiguousarray(regions, REGION_DTYPE)
    info = np.ascontiguousarray(chain_info, CHAIN_INFO_DTYPE)
    out = np.zeros(len(regions), ALNREG_DTYPE)
    check(_decl_regs().gb_bsw_alnreg_from_regions(_buf(regions), len(regions), _buf(info), len(info), _buf(out)),
          "gb_bsw_alnreg_from_regions")
    return out


def alnregs_from_chain2aln(c2a_result, chains_result):
    """The output of chain2aln_csr and of seeds2chains as the (reg_off, regs) arguments of finish_regs."""
    n_reg = np.asarray(c2a_result["n_reg"], np.int64)
    reg_off = np.concatenate([[0], np.cumsum(n_reg)]).astype(np.int64)
    return reg_off, alnregs_from_regions(c2a_result["regs"], chains_result["info"])


def finish_regs_raw(ref, qbuf, idq, l_query, reg_off, regs, opt=None, params=None, stage=1, id0=0, contig_is_alt=None,
                    n_contigs=None):
    """gb_bsw_finish_regs without the status check: (status, regs, n_out); regs is a copy the call worked on
    in place (a refused call leaves it equal to the input)."""
    opt = opt if opt is not None else reg_opt()
    params = params if params is not None else default_params()
    qbuf = np.ascontiguousarray(qbuf, np.uint8)
    idq = np.ascontiguousarray(idq, np.int64)
    l_query = np.ascontiguousarray(l_query, np.int32)
    reg_off = np.ascontiguousarray(reg_off, np.int64)
    regs = np.array(regs, ALNREG_DTYPE, copy=True, order="C")
    n = len(idq)
    alt = None if contig_is_alt is None else np.ascontiguousarray(contig_is_alt, np.uint8)
    nc = (len(alt) if alt is not None else 1) if n_contigs is None else int(n_contigs)
    n_out = np.full(max(n, 1), -1, np.int32)
    st = _decl_regs().gb_bsw_finish_regs(
        ctypes.byref(params), ctypes.byref(opt), int(stage), ref.h, None if alt is None else alt.ctypes.data, nc,
        _buf(qbuf), len(qbuf), n, _buf(idq), _buf(l_query), int(id0), _buf(reg_off), _buf(regs), n_out.ctypes.data)
    return st, regs, n_out[:n]


def finish_regs(ref, qbuf, idq, l_query, reg_off, regs, **kw):
    """gb_bsw_finish_regs: per read mem_sort_dedup_patch (stage=0) and then mem_mark_primary_se,
    mem_reorder_primary5 (opt.primary5) and the MAPQ (stage=1, the default). reg_off has one entry per read
    plus one, regs is an ALNREG_DTYPE array. Keywords: opt (reg_opt()), params (mat), stage, id0,
    contig_is_alt, n_contigs. Returns (regs, n_out): read r's survivors are regs[reg_off[r]:reg_off[r] +
    n_out[r]], the rest of its slots zero. The call runs on the host and reads ref's host copy, which a
    device call on the same Ref releases: give it a Ref of its own."""
    st, out, n_out = finish_regs_raw(ref, qbuf, idq, l_query, reg_off, regs, **kw)
    check(st, "gb_bsw_finish_regs")
    return out, n_out


def finish_regs_timing():
    """(dedup_ms, dp_ms, mark_ms, dp_rounds, dp_requests, host_reads) of this thread's last finish_regs: the
    three device times are 0 (the call runs on the host), dp_rounds is the largest number of merge alignments
    one read needed, dp_requests their total."""
    t = [ctypes.c_float() for _ in range(3)]
    r, q, h = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(_decl_regs().gb_bsw_finish_regs_timing(*[ctypes.byref(x) for x in t], ctypes.byref(r), ctypes.byref(q),
                                                ctypes.byref(h)), "gb_bsw_finish_regs_timing")
    return t[0].value, t[1].value, t[2].value, r.value, q.value, h.value


# ---- mate rescue (mem_pestat, and mem_sam_pe's rescue loop around mem_matesw; bwamem_pair.c:23-180, 265-276) ----

# struct gb_bsw_pestat (include/gb_bsw.h): mem_pestat_t
PESTAT_DTYPE = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("_pad", "<i4"), ("avg", "<f8"),
                         ("std", "<f8")])
assert PESTAT_DTYPE.itemsize == 32
PESTAT_FIELDS = ("low", "high", "failed", "avg", "std")


class PeOpt(ctypes.Structure):
    """gb_bsw_pe_opt: the mem_opt_t fields mem_pestat and mem_matesw read."""
    _fields_ = ([(k, ctypes.c_int32) for k in "a b o_del e_del o_ins e_ins min_seed_len max_chain_gap pen_unpaired "
                                              "max_matesw max_ins".split()]
                + [(k, ctypes.c_float) for k in "mask_level mask_level_redun".split()])


_PE_OPT_FLOATS = ("mask_level", "mask_level_redun")


def _decl_matesw():
    L = _decl_regs()
    if getattr(L, "_bsw_matesw_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_bsw_pe_default_opt.argtypes = [vp]
    L.gb_bsw_pe_default_opt.restype = None
    L.gb_bsw_pestat.argtypes = [vp, i64, i64, vp, vp, vp]
    L.gb_bsw_mate_rescue.argtypes = [vp, vp, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.gb_bsw_mate_rescue_timing.argtypes = [vp] * 6
    L._bsw_matesw_decl = True
    return L


def pe_opt(**kw):
    """bwa's defaults (bwamem.c:50-86): a 1, b 4, gaps 6 / 1, min_seed_len 19, max_chain_gap 10000, pen_unpaired 17,
    max_matesw 50, max_ins 10000, mask_level 0.5, mask_level_redun 0.95; keywords override."""
    o = PeOpt()
    _decl_matesw().gb_bsw_pe_default_opt(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, float(v) if k in _PE_OPT_FLOATS else int(v))
    return o


def pestat_raw(l_pac, reg_off, regs, opt=None, pes=None):
    """gb_bsw_pestat without the status check: (status, pes); pes (a PESTAT_DTYPE array of 4) is written only by
    a call that succeeds."""
    opt = opt if opt is not None else pe_opt()
    reg_off = np.ascontiguousarray(reg_off, np.int64)
    regs = np.ascontiguousarray(regs, ALNREG_DTYPE)
    pes = np.zeros(4, PESTAT_DTYPE) if pes is None else pes
    st = _decl_matesw().gb_bsw_pestat(ctypes.byref(opt), int(l_pac), len(reg_off) - 1, _buf(reg_off), _buf(regs),
                                      pes.ctypes.data)
    return st, pes


def pestat(l_pac, reg_off, regs, opt=None):
    """gb_bsw_pestat: mem_pestat over the stage-0 regions of an even number of reads (reads 2p and 2p + 1 are
    pair p). Returns a PESTAT_DTYPE array of 4, one record per orientation FF, FR, RF, RR. Runs on the host."""
    st, pes = pestat_raw(l_pac, reg_off, regs, opt)
    check(st, "gb_bsw_pestat")
    return pes


def mate_rescue_raw(ref, pes, qbuf, idq, l_query, reg_off, regs, opt=None, params=None, contig_end=None,
                    n_contigs=None, out_cap=None, want_n_sw=True):
    """gb_bsw_mate_rescue without the status check: a dict with status, regs (out_cap records, zero where the
    call wrote nothing), out_off, n_out, n_sw, out_used. out_cap defaults to the bound that always suffices."""
    opt = opt if opt is not None else pe_opt()
    params = params if params is not None else default_params()
    pes = np.ascontiguousarray(pes, PESTAT_DTYPE)
    qbuf = np.ascontiguousarray(qbuf, np.uint8)
    idq = np.ascontiguousarray(idq, np.int64)
    l_query = np.ascontiguousarray(l_query, np.int32)
    reg_off = np.ascontiguousarray(reg_off, np.int64)
    regs = np.ascontiguousarray(regs, ALNREG_DTYPE)
    n = len(idq)
    assert n % 2 == 0 and len(pes) == 4
    ce = None if contig_end is None else np.ascontiguousarray(contig_end, np.int64)
    nc = (len(ce) if ce is not None else 1) if n_contigs is None else int(n_contigs)
    if out_cap is None:
        n_reg = np.diff(reg_off)  # every region of the mate can be an anchor, each adds at most four
        out_cap = int(n_reg.sum() + 4 * np.minimum(n_reg, max(int(opt.max_matesw), 0)).sum()) if n else 0
    out = np.zeros(max(int(out_cap), 1), ALNREG_DTYPE)
    out_off = np.full(max(n, 1), -1, np.int64)
    n_out = np.full(max(n, 1), -1, np.int32)
    n_sw = np.full(max(n // 2, 1), -1, np.int32)
    used = ctypes.c_int64(-1)
    st = _decl_matesw().gb_bsw_mate_rescue(
        ctypes.byref(params), ctypes.byref(opt), pes.ctypes.data, ref.h, None if ce is None else ce.ctypes.data, nc,
        _buf(qbuf), len(qbuf), n // 2, _buf(idq), _buf(l_query), _buf(reg_off), _buf(regs), out.ctypes.data,
        int(out_cap), out_off.ctypes.data, n_out.ctypes.data, n_sw.ctypes.data if want_n_sw else None,
        ctypes.byref(used))
    return dict(status=st, regs=out[:int(out_cap)], out_off=out_off[:n], n_out=n_out[:n], n_sw=n_sw[:n // 2],
                out_used=used.value)


def mate_rescue(ref, pes, qbuf, idq, l_query, reg_off, regs, **kw):
    """gb_bsw_mate_rescue: the rescue loop of mem_sam_pe around mem_matesw for pairs of reads (2p, 2p + 1). regs
    (never written) holds the reads' stage-0 regions, reg_off one entry per read plus one, pes is pestat()'s
    result. Keywords: opt (pe_opt()), params (mat), contig_end, n_contigs, out_cap. Returns a dict: read r's
    final list is regs[out_off[r]:out_off[r] + n_out[r]]; n_sw[p] counts the alignments pair p performed."""
    res = mate_rescue_raw(ref, pes, qbuf, idq, l_query, reg_off, regs, **kw)
    check(res["status"], "gb_bsw_mate_rescue")
    return res


def mate_rescue_timing():
    """(fetch_ms, dp_ms, region_ms, host_ms, rounds, requests) of this thread's last mate_rescue: the device time
    of the window and fetch kernels, of the local DP and of the region kernel, the host time of the bookkeeping
    between the rounds, the rounds that had a request, and the requests."""
    t = [ctypes.c_float() for _ in range(4)]
    r, q = ctypes.c_int32(0), ctypes.c_int64(0)
    check(_decl_matesw().gb_bsw_mate_rescue_timing(*[ctypes.byref(x) for x in t], ctypes.byref(r), ctypes.byref(q)),
          "gb_bsw_mate_rescue_timing")
    return t[0].value, t[1].value, t[2].value, t[3].value, r.value, q.value
