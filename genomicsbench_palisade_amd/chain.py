"""Host mirror of the reference chaining interface (host_chain_kernel, benchmarks/chain/src/
host_kernel.cpp:481-501) over CSR call sets (gen.ChainCalls), executed by csrc/chain.hip.

Below it, the mirror of gb_chain_extd2 (include/gb_chain_extd2.h): base-level alignment between and beyond a
chain's anchors, the batch form of minimap2's ksw_extd2_sse (tools/minimap2/ksw2_extd2_sse.c), executed by
csrc/chain_extd2.hip over gen.Extd2Items."""
from __future__ import annotations

import ctypes

import numpy as np

from . import check, lib
from .gen import EXTD2_ITEM_DTYPE, EXTD2_PARAMS_DTYPE, extd2_params  # noqa: F401


def _decl():
    L = lib()
    if getattr(L, "_chain_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_chain_batch_create.argtypes = [i64, vp, vp, vp, vp, vp, ctypes.POINTER(vp)]
    L.gb_chain_batch_run.argtypes = [vp]
    L.gb_chain_batch_sync.argtypes = [vp]
    L.gb_chain_batch_results.argtypes = [vp, vp, vp, vp, vp, vp]
    L.gb_chain_batch_timing.argtypes = [vp, vp]
    L.gb_chain_batch_split_stats.argtypes = [vp, vp, vp, vp]
    L.gb_chain_batch_destroy.argtypes = [vp]
    L.gb_chain_batch_backtrack.argtypes = [vp, ctypes.c_int32, ctypes.c_int32]
    L.gb_chain_batch_chains.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.gb_chain_batch_backtrack_timing.argtypes = [vp, vp]
    L._chain_decl = True
    return L


class ChainBatch:
    def __init__(self, calls):
        L = _decl()
        self.calls = calls
        self.h = ctypes.c_void_p()
        check(L.gb_chain_batch_create(calls.ncalls, calls.offsets.ctypes.data, calls.avg_qspan.ctypes.data,
                                      calls.params4.ctypes.data, calls.x.ctypes.data, calls.y.ctypes.data,
                                      ctypes.byref(self.h)), "gb_chain_batch_create")

    def run(self):
        check(_decl().gb_chain_batch_run(self.h), "gb_chain_batch_run")

    def sync(self):
        check(_decl().gb_chain_batch_sync(self.h), "gb_chain_batch_sync")

    def results(self):
        n = self.calls.nanchors
        out = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        v = ctypes.c_int64()
        check(_decl().gb_chain_batch_results(self.h, *[o.ctypes.data for o in out], ctypes.byref(v)),
              "gb_chain_batch_results")
        return [o[:n] for o in out] + [v.value]

    def timing(self):
        ms = ctypes.c_float()
        check(_decl().gb_chain_batch_timing(self.h, ctypes.byref(ms)), "gb_chain_batch_timing")
        return ms.value

    def split_stats(self):
        """-> (calls run as speculative segments, guess/verify rounds, fix-up blocks) of the last run."""
        v = [ctypes.c_int64() for _ in range(3)]
        check(_decl().gb_chain_batch_split_stats(self.h, *[ctypes.byref(x) for x in v]), "gb_chain_batch_split_stats")
        return tuple(x.value for x in v)

    def backtrack(self, min_cnt: int = 3, min_sc: int = 40):
        """minimap2's chain backtrack on this batch's chain_dp outputs (asynchronous)."""
        check(_decl().gb_chain_batch_backtrack(self.h, min_cnt, min_sc), "gb_chain_batch_backtrack")

    def chains(self):
        """-> (n_chains [ncalls], u [CSR at offsets], n_anchors [ncalls], ax, ay [CSR at 2*offsets],
        total chains, total anchors)."""
        c = self.calls
        n = max(c.nanchors, 1)
        nch = np.zeros(max(c.ncalls, 1), np.int64)
        nan = np.zeros(max(c.ncalls, 1), np.int64)
        u = np.zeros(n, np.uint64)
        ax = np.zeros(2 * n, np.uint64)
        ay = np.zeros(2 * n, np.uint64)
        tc, ta = ctypes.c_int64(), ctypes.c_int64()
        check(_decl().gb_chain_batch_chains(self.h, nch.ctypes.data, u.ctypes.data, nan.ctypes.data, ax.ctypes.data,
                                            ay.ctypes.data, ctypes.byref(tc), ctypes.byref(ta)),
              "gb_chain_batch_chains")
        return nch[:c.ncalls], u, nan[:c.ncalls], ax, ay, tc.value, ta.value

    def backtrack_timing(self):
        ms = ctypes.c_float()
        check(_decl().gb_chain_batch_backtrack_timing(self.h, ctypes.byref(ms)), "gb_chain_batch_backtrack_timing")
        return ms.value

    def close(self):
        if self.h:
            _decl().gb_chain_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- gb_chain_extd2 ----

EXTD2_MAX_LEN = 32768
EXTD2_RIGHT, EXTD2_APPROX_MAX, EXTD2_APPROX_DROP, EXTD2_EXTZ_ONLY, EXTD2_REV_CIGAR = 0x02, 0x08, 0x10, 0x40, 0x80
EXTD2_FLAGS = 0xda
EXTD2_NEG_INF = -0x40000000
EXTD2_RESULT_DTYPE = np.dtype([(f, "<i4") for f in ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q",
                                                    "score", "reach_end", "n_cigar", "pad")])
assert EXTD2_RESULT_DTYPE.itemsize == 48


def _extd2_decl():
    L = lib()
    if getattr(L, "_chain_extd2_decl", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.gb_chain_extd2.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp]
    L.gb_chain_extd2_timing.argtypes = [vp, vp, vp]
    L.gb_chain_extd2_plan.argtypes = [vp, vp]
    L._chain_extd2_decl = True
    return L


def _buf(a):
    return a.ctypes.data if len(a) else None


def extd2_need(items):
    """The cigar_cap the call asks for: qlen + tlen summed over EXTD2_ITEM_DTYPE records."""
    items = np.asarray(items, EXTD2_ITEM_DTYPE)
    return int((items["qlen"].astype(np.int64) + items["tlen"]).sum())


def extd2_raw(params, seqs, items, cigar_cap=None, res=None, cigar=None, cigar_off=None):
    """gb_chain_extd2 as it is: (status, res, cigar buffer, cigar_off, cigar_used). No exception. `res`, `cigar`
    and `cigar_off` are the buffers the call writes (new ones by default: res of -7 in every field, cigar_off of
    -1), so that a refusal can be seen to leave them untouched; cigar_used starts as -1."""
    L = _extd2_decl()
    params = np.ascontiguousarray(params, EXTD2_PARAMS_DTYPE)
    seqs = np.ascontiguousarray(seqs, np.uint8)
    items = np.ascontiguousarray(items, EXTD2_ITEM_DTYPE)
    cap = extd2_need(items) if cigar_cap is None else int(cigar_cap)
    if res is None:
        res = np.full(len(items) * 12, -7, np.int32).view(EXTD2_RESULT_DTYPE)
    if cigar is None:
        cigar = np.zeros(max(cap, 0), np.uint32)
    if cigar_off is None:
        cigar_off = np.full(len(items) + 1, -1, np.int64)
    used = ctypes.c_int64(-1)
    st = L.gb_chain_extd2(params.ctypes.data, _buf(seqs), len(seqs), _buf(items), len(items), _buf(res), _buf(cigar), cap,
                          cigar_off.ctypes.data, ctypes.addressof(used))
    return st, res, cigar, cigar_off, used.value


def extd2(x):
    """ksw_extd2_sse of every item of a gen.Extd2Items: (res, cigar words, cigar_off). Item i owns
    cigar[cigar_off[i]:cigar_off[i + 1]], the reference's ez->cigar words."""
    st, res, cigar, off, used = extd2_raw(x.params, x.seqs, x.items)
    check(st, "gb_chain_extd2")
    return res, cigar[:used], off


def extd2_timing():
    """(fill ms, walk ms, in-band cells swept) of this thread's last device call of extd2."""
    f, w, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_int64()
    check(_extd2_decl().gb_chain_extd2_timing(ctypes.addressof(f), ctypes.addressof(w), ctypes.addressof(c)),
          "gb_chain_extd2_timing")
    return f.value, w.value, c.value


def extd2_plan():
    """(chunks, largest chunk's workspace bytes) of this thread's last device call of extd2."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(_extd2_decl().gb_chain_extd2_plan(ctypes.addressof(a), ctypes.addressof(b)), "gb_chain_extd2_plan")
    return a.value, b.value
