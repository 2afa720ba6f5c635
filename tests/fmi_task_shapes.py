"""Builders and witnesses for the per-call SMEM kernels (csrc/fmi_tasks.hip, csrc/fmi_wave.h), CPU only.

nested_reference builds a read and a reference on which one getSMEMsOnePosOneThread call has a `prev`
list as long as the read allows and emits one record per backward step; one_pos_trace restates that
call in plain Python over brute-force occurrence counts and records what each backward step did, so a
test can prove from the oracle and the trace alone that an input reaches a given branch of the kernels
(a second 64-entry chunk, a dedupe across a chunk boundary, a slot overflow). The expected values of
every GPU comparison come from the oracle (oracle/fmi_oracle.c) through the wrappers at the end."""
from __future__ import annotations

import bisect
import ctypes

import numpy as np

import fmi_util
import oracle_lib

FIELDS = ("rid", "m", "n", "k", "l", "s")


def revcomp(a):
    return (3 - np.asarray(a, np.uint8)[::-1]).astype(np.uint8)


def nested_reference(rng, L, x0, g=None, d=None):
    """A random read R of L bases and a reference on which the forward extension from x0 changes s at
    every step (a `prev` list of L - x0 entries) and the copies of R[x0..j] carry d_j bases of R's left
    context: after 3000 random bases, for every j in x0..L-1 one record
        [a base != R[x0-d_j-1]] R[x0-d_j .. x0-1] R[x0 .. j] [a base != R[j+1]] [5 random bases].
    d_j = min(x0, (L-1-j) // g): each backward step kills the g longest survivors; g=None draws d_j at
    random in 0..x0; d (a sequence of L - x0 values, for j = x0..L-1) sets them. Returns (R, ref)."""
    R = rng.integers(0, 4, L, dtype=np.uint8)
    parts = [rng.integers(0, 4, 3000, dtype=np.uint8)]

    def other(b):
        return np.array([(int(b) + 1 + int(rng.integers(0, 3))) % 4], np.uint8)

    for j in range(x0, L):
        if d is not None:
            dj = int(d[j - x0])
        elif g is not None:
            dj = min(x0, (L - 1 - j) // g)
        else:
            dj = int(rng.integers(0, x0 + 1))
        assert 0 <= dj <= x0
        lo = x0 - dj
        parts.append(other(R[lo - 1]) if lo > 0 else rng.integers(0, 4, 1, dtype=np.uint8))
        parts.append(R[lo:j + 1])
        parts.append(other(R[j + 1]) if j + 1 < L else rng.integers(0, 4, 1, dtype=np.uint8))
        parts.append(rng.integers(0, 4, 5, dtype=np.uint8))
    return R, np.concatenate(parts).astype(np.uint8)


class CountIndex:
    """Bi-intervals (k, l, s) of patterns of up to `window` bases over ref + revcomp(ref) (+ '$'), by
    bisection in the sorted list of the text's suffixes cut to `window` bases: k = suffixes smaller than
    P (the empty '$' suffix is row 0), s = suffixes that start with P, l = the k of revcomp(P) -- the row
    numbering of the bwa-mem2 index, as BruteIndex of test_fmi_getsmems_pin.py, for references too long
    for whole suffixes."""

    def __init__(self, ref, window):
        ref = np.asarray(ref, np.uint8)
        t = np.concatenate([ref, revcomp(ref)]).tobytes()
        self.window = window
        self.keys = sorted(t[i:i + window] for i in range(len(t) + 1))

    def interval(self, p):
        p = bytes(bytearray(int(b) for b in p))
        assert 0 < len(p) <= self.window
        k = bisect.bisect_left(self.keys, p)
        e = bisect.bisect_left(self.keys, p + b"\xff")
        rc = bytes(3 - b for b in reversed(p))
        return k, bisect.bisect_left(self.keys, rc), e - k


_index_cache = {}


def _count_index(ref, window):
    ref = np.ascontiguousarray(ref, np.uint8)
    key = (hash(ref.tobytes()), len(ref))
    ix = _index_cache.get(key)
    if ix is None or ix.window < window:
        ix = _index_cache[key] = CountIndex(ref, window)
    return ix


def one_pos_trace(ref, q, x, min_intv, min_seed_len):
    """One getSMEMsOnePosOneThread call (FMI_search.cpp:1004-1178) for position x of read q, restated
    over brute-force counts in ref + revcomp(ref). Returns (records, next_x, trace): records are
    (m, n, k, l, s) in emission order; trace has one entry per backward step j:
      n_list  entries of the `prev` list the step extends
      s_ext   the extended entries' s', in list order
      f       list position at which the first loop stops (None: it ran off the list)
      kind    "push" or "emit" for that stop
      pushed  list positions whose extension went into the next list.
    A witness of what the kernels' inputs reach, not the reference of any comparison."""
    q = [int(b) for b in q]
    L = len(q)
    ix = _count_index(ref, L + 1)
    memo = {}

    def iv(m, n):
        r = memo.get((m, n))
        if r is None:
            r = memo[(m, n)] = ix.interval(q[m:n + 1])
        return r

    def i32(v):
        return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)

    records, trace = [], []
    next_x = x + 1
    if q[x] >= 4:
        return records, next_x, trace
    sm = (x, x) + iv(x, x)  # (m, n, k, l, s)
    prev = []
    for j in range(x + 1, L):
        next_x = j + 1
        if q[j] >= 4:
            break
        ns = (x, j) + iv(x, j)
        if ns[4] != sm[4]:
            prev.append(sm)
        if ns[4] < min_intv:
            next_x = j
            break
        sm = ns
    if sm[4] >= min_intv:
        prev.append(sm)
    prev.reverse()
    for j in range(x - 1, -1, -1):
        if q[j] > 3:
            break
        ext = [(j, e[1]) + iv(j, e[1]) for e in prev]
        step = {"j": j, "n_list": len(prev), "s_ext": [e[4] for e in ext], "f": None, "kind": None, "pushed": []}
        curr, curr_s, p = [], -1, 0
        while p < len(prev):
            s0, ns = prev[p], ext[p]
            if ns[4] < min_intv and s0[1] - s0[0] + 1 >= min_seed_len:
                records.append(s0)
                step["f"], step["kind"] = p, "emit"
                break
            if ns[4] >= min_intv and ns[4] != curr_s:
                curr_s = i32(ns[4])
                curr.append(ns)
                step["f"], step["kind"] = p, "push"
                step["pushed"].append(p)
                break
            p += 1
        p += 1
        while p < len(prev):
            ns = ext[p]
            if ns[4] >= min_intv and ns[4] != curr_s:
                curr_s = i32(ns[4])
                curr.append(ns)
                step["pushed"].append(p)
            p += 1
        trace.append(step)
        prev = curr
        if not prev:
            break
    if prev and prev[0][1] - prev[0][0] + 1 >= min_seed_len:
        records.append(prev[0])
    return records, next_x, trace


# ------------------------------------------------------------------ read sets and the oracle's answers
class ReadSet:
    """Reads of any lengths as the class API takes them: flat codes, lens[r], offs[r]."""

    def __init__(self, reads):
        self.reads = [np.ascontiguousarray(r, np.uint8) for r in reads]
        self.n = len(self.reads)
        self.lens = np.array([len(r) for r in self.reads], np.int32)
        self.offs = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.int32) if self.n else np.zeros(0, np.int32)
        self.flat = np.concatenate(self.reads + [np.zeros(1, np.uint8)]).astype(np.uint8)  # never empty
        self.maxlen = int(self.lens.max()) if self.n else 0


def fields(a):
    """SMEM array -> int64[n, 6] of (rid, m, n, k, l, s)."""
    if len(a) == 0:
        return np.zeros((0, 6), np.int64)
    return np.stack([a[f].astype(np.int64) for f in FIELDS], axis=1)


def _phase(oi):
    L = oracle_lib.oracle()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.fmi_oracle_phase.restype = ctypes.c_int64
    L.fmi_oracle_phase.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    return L.fmi_oracle_phase


def _cap(rs, rid):
    # OnePos emits at most one record per backward step and one at the end; LAST one per two bases
    return int(rs.lens[np.asarray(rid, np.int64)].astype(np.int64).sum()) + len(rid) + 64 if len(rid) else 64


def oracle_onepos(oi, rs, qpos, intv, rid, min_seed_len):
    """-> (records int64[n, 6], next_pos int16[ntasks], backwardExt calls) of one OnePos call."""
    qpos = np.array(qpos, np.int16)
    intv = np.array(intv, np.int32)
    rid = np.array(rid, np.int32)
    out = np.zeros(_cap(rs, rid), fmi_util.SMEM_DTYPE)
    c0 = oi.bwt_calls()
    n = _phase(oi)(oi.h, 1, rs.flat.ctypes.data, rs.lens.ctypes.data, rs.offs.ctypes.data, qpos.ctypes.data,
                   intv.ctypes.data, rid.ctypes.data, len(rid), max(rs.maxlen, 1), min_seed_len, out.ctypes.data)
    return fields(out[:n]), qpos, oi.bwt_calls() - c0


def oracle_allpos(oi, rs, intv, rid, min_seed_len):
    """-> (records in the reference's round-major order, rounds per task, backwardExt calls). rounds
    comes from a plain loop over next_x: OnePos calls from 0 until the read's end, per task."""
    intv0 = np.array(intv, np.int32)
    rid0 = np.array(rid, np.int32)
    nt = len(rid0)
    cap = 64
    if nt:
        ln = rs.lens[rid0].astype(np.int64)
        cap += int((ln * (ln + 3) // 2).clip(max=1 << 20).sum())
    out = np.zeros(min(cap, 1 << 24), fmi_util.SMEM_DTYPE)
    i, r = intv0.copy(), rid0.copy()
    qp = np.zeros(max(nt, 1), np.int16)
    c0 = oi.bwt_calls()
    n = _phase(oi)(oi.h, 0, rs.flat.ctypes.data, rs.lens.ctypes.data, rs.offs.ctypes.data, qp.ctypes.data,
                   i.ctypes.data, r.ctypes.data, nt, max(rs.maxlen, 1), min_seed_len, out.ctypes.data)
    calls = oi.bwt_calls() - c0
    assert n <= len(out)
    rounds = np.zeros(nt, np.int32)
    x = np.zeros(nt, np.int64)
    while True:
        live = np.nonzero(x < rs.lens[rid0])[0] if nt else []
        if len(live) == 0:
            break
        _, nx, _ = oracle_onepos(oi, rs, x[live], intv0[live], rid0[live], min_seed_len)
        x[live] = nx
        rounds[live] += 1
    return fields(out[:n]), rounds, calls


def oracle_last(oi, rs, max_intv, min_seed_len):
    """-> (records, backwardExt calls) of one bwtSeedStrategyAllPosOneThread call over every read."""
    intv = np.array(max_intv, np.int32)
    assert len(intv) == rs.n
    out = np.zeros(_cap(rs, np.arange(rs.n)), fmi_util.SMEM_DTYPE)
    c0 = oi.bwt_calls()
    n = _phase(oi)(oi.h, 2, rs.flat.ctypes.data, rs.lens.ctypes.data, rs.offs.ctypes.data, None, intv.ctypes.data,
                   None, rs.n, max(rs.maxlen, 1), min_seed_len, out.ctypes.data)
    return fields(out[:n]), oi.bwt_calls() - c0


def oracle_get_smems(oi, codes, num_reads, min_seed_len, nthreads=1):
    c0 = oi.bwt_calls()
    out = oi.get_smems(codes, num_reads, min_seed_len, nthreads)
    return fields(out), oi.bwt_calls() - c0


# ------------------------------------------------------------------ the constructed cases
def _ordinary(rng, ref, n, length):
    """Reads sampled from the reference (either strand) with a few substitutions: ordinary tasks."""
    out = []
    for r in range(n):
        p = int(rng.integers(0, len(ref) - length))
        s = ref[p:p + length].copy()
        if r % 2:
            s = revcomp(s)
        sub = rng.random(length) < 0.03
        s[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
        out.append(s)
    return out


class Case:
    """Nested reads over one reference (their references concatenated) plus ordinary reads."""

    def __init__(self, seed, specs, ordinary=(), extra=()):
        rng = np.random.default_rng(seed)
        reads, refs = [], []
        for L, x0, g, d in specs:
            R, ref = nested_reference(rng, L, x0, g=g, d=d)
            reads.append(R)
            refs.append(ref)
        self.ref = np.concatenate(refs)
        self.specs = list(specs)
        self.nested = len(reads)
        for n, length in ordinary:
            reads += _ordinary(rng, self.ref, n, length)
        for length in extra:  # random reads: LAST emits len // 2 records on them with a huge max_intv
            reads.append(rng.integers(0, 4, length, dtype=np.uint8))
        self.rs = ReadSet(reads)
        self._oi = None

    @property
    def oi(self):
        if self._oi is None:
            self._oi = fmi_util.OracleIndex(self.ref)
        return self._oi


def _d_dead_head(L, x0, head):
    """The `head` longest entries lack any left context, the others have all of it."""
    n = L - x0
    return [0 if j >= n - head else x0 for j in range(n)]


def _d_runs(L, x0, at):
    """Full left context only under the entries at list positions `at` (0 = the longest): after one
    backward step every entry survives, with s' = the number of those at or before it -- runs of equal s'."""
    n = L - x0
    return [x0 if (n - 1 - j) in at else 0 for j in range(n)]


RUNS_AT = (0, 30, 100, 150, 200)

_SPECS = {
    # name: (seed, [(L, x0, g, d)], ordinary [(count, length)], extra random read lengths)
    "L151": (151, [(151, 31, 3, None), (151, 32, 3, None), (151, 40, 2, None), (151, 100, 1, None)], [(6, 151), (3, 77)],
             (96, 98)),
    "L255": (255, [(255, 1, None, None), (255, 60, 3, None)], [(3, 255), (2, 100)], ()),
    "L256": (256, [(256, 60, 3, None), (256, 100, 1, None), (256, 1, None, None),
                   (256, 50, None, _d_dead_head(256, 50, 100)), (256, 10, None, _d_runs(256, 10, RUNS_AT))],
             [(4, 256), (3, 151)], ()),
    # both sides of the OnePos / AllPos slot (32 records), of LAST's (48) and tasks above twice either
    "SLOT": (32, [(151, 31, 3, None), (151, 32, 3, None), (256, 100, 1, None)], [(5, 151), (3, 77)], (96, 98, 256)),
    # fixed-stride reads for getSMEMs: both sides of its 64-record slot and a task above twice it
    "G256": (64, [(256, 63, 3, None), (256, 64, 3, None), (256, 140, 1, None)], [(3, 256)], ()),
    "L257": (257, [(257, 1, None, None), (257, 60, 3, None), (257, 10, None, _d_runs(257, 10, RUNS_AT))], [(3, 257), (2, 64)],
             ()),
}
_cases = {}


def case(name):
    """The named case, built once per process (its oracle index too)."""
    if name not in _cases:
        seed, specs, ordinary, extra = _SPECS[name]
        _cases[name] = Case(seed, specs, ordinary, extra)
    return _cases[name]
