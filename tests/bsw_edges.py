"""Edge inputs and parameter sets for the banded-SW extension kernels (tests/test_bsw_edges.py,
tests/golden/make_bsw_edges_golden.py).

gen.bsw_pairs is the workload generator: symmetric scoring, tlen >= qlen, h0 in {0, 10..70}, random
lengths. The sets here are cross products over the values at which csrc/bsw.hip changes shape:
query lengths around 8 * NCH (the pair-per-lane kernel's variants, 160 handing over to the
wave-per-pair kernel) and 64 * K (the wave kernel's columns per lane), target lengths around the
256-base refill of the wave kernel's target word and the 4096 clamp of the sort key, targets shorter
than the query and empty, and h0 around o_ins + e_ins (an all-zero first row) and at the limit of
the lane kernel's 16-bit packing.

A set is described by lists only; an entry of a tlen or h0 list is an int or a function of qlen."""
from __future__ import annotations

import os

import numpy as np

from genomicsbench_palisade_amd import bsw, gen

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bsw_edges_golden.npz")
INPUT_KEYS = ("tgt", "toff", "tlen", "qry", "qoff", "qlen", "h0")


def edge_pairs(qlens, tlens, h0s, seed, sub=0.04, n_rate=0.01):
    """The cross product qlens x tlens x h0s (in that nesting) as one gen.BswPairs. Each pair has its
    own random query over 0..3; its target is the query truncated, or extended with random bases, to
    tlen, with one indel of 1..4 bases in about 30 % of the pairs whose lengths both exceed 8, and
    substitutions at rate `sub`; code 4 then goes into both at rate `n_rate`. One rng(seed)."""
    rng = np.random.default_rng(seed)

    def val(v, q):
        return int(v(q)) if callable(v) else int(v)
    Q, T, ql, tl, h0 = [], [], [], [], []
    for q in qlens:
        for tv in tlens:
            for hv in h0s:
                t = val(tv, q)
                qs = rng.integers(0, 4, q).astype(np.uint8)
                # 4 spare bases: a deletion of up to 4 still leaves t
                ts = np.concatenate([qs, rng.integers(0, 4, max(t - q, 0) + 4).astype(np.uint8)])
                if q > 8 and t > 8 and rng.random() < 0.3:
                    d = int(rng.integers(1, 5))
                    at = int(rng.integers(1, min(q, t)))
                    if rng.random() < 0.5:
                        ts = np.delete(ts, np.arange(at, at + d))
                    else:
                        ts = np.insert(ts, at, rng.integers(0, 4, d).astype(np.uint8))
                ts = ts[:t].copy()
                m = rng.random(t) < sub
                ts[m] = rng.integers(0, 4, int(m.sum())).astype(np.uint8)
                qs[rng.random(q) < n_rate] = 4
                ts[rng.random(t) < n_rate] = 4
                Q.append(qs)
                T.append(ts)
                ql.append(q)
                tl.append(t)
                h0.append(val(hv, q))
    ql, tl = np.array(ql, np.int32), np.array(tl, np.int32)
    toff, qoff = np.zeros(len(tl), np.int64), np.zeros(len(ql), np.int64)
    toff[1:] = np.cumsum(tl, dtype=np.int64)[:-1]
    qoff[1:] = np.cumsum(ql, dtype=np.int64)[:-1]
    return gen.BswPairs(np.concatenate(T), toff, tl, np.concatenate(Q), qoff, ql, np.array(h0, np.int32))


MAIN_QLENS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 254,
              255]
MAIN_TLENS = [0, 1, lambda q: q // 2, lambda q: q - 1, lambda q: q, lambda q: q + 1, 255, 256, 257, 511, 512, 513,
              1025]
MAIN_H0S = [0, 1, 6, 7, 8, 40, 200]

LONG_QLENS = [8, 96, 160, 255]
LONG_TLENS = [4095, 4096, 4097]
LONG_H0S = [40]

# the lane kernel takes a pair iff h0 + qlen * mx < 30000 (bsw_batch_plan): d = 0 is the last eligible
# h0, d = 1 the first that goes to the wave kernel
LIMIT_MATCH = [1, 5, 127]
LIMIT_QLENS = [31, 96, 159, 160, 200]
LIMIT_D = [-1, 0, 1, 2000]


def main_set():
    return edge_pairs(MAIN_QLENS, MAIN_TLENS, MAIN_H0S, seed=20240)


def long_set():
    return edge_pairs(LONG_QLENS, LONG_TLENS, LONG_H0S, seed=20241)


def limit_set(mx):
    return edge_pairs(LIMIT_QLENS, [lambda q: q + 20], [lambda q, d=d: 29999 - q * mx + d for d in LIMIT_D],
                      seed=20242 + mx)


def limit_d(p, mx):
    """d of every pair of limit_set(mx)."""
    return p.h0.astype(np.int64) - (29999 - p.qlen.astype(np.int64) * mx)


def input_sets():
    """name -> BswPairs for every set the fixture holds."""
    s = {"main": main_set(), "long": long_set()}
    for mx in LIMIT_MATCH:
        s[f"limit{mx}"] = limit_set(mx)
    return s


ASYM_MAT = [5, -7, -3, -9, -2, -6, 4, -8, -1, -3, -2, -9, 6, -5, -1, -8, -4, -7, 3, -2, -1, -3, -2, -4, -1]
EXT_MAT = [127, -128, -100, -90, -2, -128, 127, -77, -101, -3, -99, -80, 126, -128, -1, -128, -60, -128, 125, -2,
           -1, -3, -2, -4, -5]

# name -> keyword arguments of bsw.default_params
PARAM_SETS = {
    "default": {},
    "w0": {"w": 0},
    "w1": {"w": 1},
    "w2": {"w": 2},
    "zdrop5_asym": {"zdrop": 5, "o_del": 4, "e_del": 2, "o_ins": 7, "e_ins": 3},
    "e_only": {"e_del": 1, "e_ins": 2},
    "o_only": {"o_del": 5, "o_ins": 6},
    "o0": {"o_del": 0, "o_ins": 0},
    "bigext": {"e_del": 9, "e_ins": 7, "end_bonus": 0},
    "bigext_bonus": {"e_del": 9, "e_ins": 7, "end_bonus": 50},
    "asym_mat": {"mat": ASYM_MAT},
    "ext_mat": {"mat": EXT_MAT},
    "m5": {"match": 5},
    "allneg": {"mat": [-1] * 25},
    "ambig_pos": {"match": 2, "mismatch": 3, "ambig": 1},
    "m127": {"match": 127},  # the limit set only
}
MAIN_PARAMS = [k for k in PARAM_SETS if k != "m127"]
LIMIT_PARAMS = {1: "default", 5: "m5", 127: "m127"}
# (input set, parameter set) of every expected output in the fixture
CASES = ([("main", k) for k in MAIN_PARAMS] + [("long", "default"), ("long", "asym_mat")] +
         [(f"limit{mx}", LIMIT_PARAMS[mx]) for mx in LIMIT_MATCH])


def params(name, **override):
    kw = dict(PARAM_SETS[name])
    kw.update(override)
    return bsw.default_params(**kw)


def transposed(mat):
    return np.asarray(mat, np.int8).reshape(5, 5).T.reshape(-1).tolist()


# The inputs discriminate: (what is broken, parameter set whose fixture outputs are the baseline, the
# broken keyword arguments, required fraction of main-set pairs whose outputs change). The broken run
# is the oracle with other *arguments*, so these are properties of the reference and the inputs alone.
BROKEN_RULES = [
    ("asym_mat transposed", "asym_mat", {"mat": transposed(ASYM_MAT)}, 0.10),
    ("ext_mat transposed", "ext_mat", {"mat": transposed(EXT_MAT)}, 0.10),
    ("e_only with e_ins := e_del", "e_only", {"e_ins": 1}, 0.10),
    ("o_only with o_ins := o_del", "o_only", {"o_ins": 5}, 0.05),
    ("zdrop5_asym with ins and del swapped", "zdrop5_asym", {"o_del": 7, "e_del": 3, "o_ins": 4, "e_ins": 2}, 0.05),
    ("w0 vs w1", "w0", {"w": 1}, 0.03),
    ("w1 vs w2", "w1", {"w": 2}, 0.03),
]


def changed_fraction(a, b):
    return float((np.asarray(a) != np.asarray(b)).any(axis=1).mean())


class Fixture:
    """bsw_edges_golden.npz: sets[name] -> BswPairs, params[name] -> bsw.Params, out / cells[(set,
    parameter set)] -> ksw_extend2's six outputs [n, 6] and the oracle's per-pair cell counts [n]."""

    def __init__(self, path=FIXTURE):
        z = np.load(path)
        self.sets = {s: gen.BswPairs(*[z[f"{s}.{k}"] for k in INPUT_KEYS]) for s in dict.fromkeys(c[0] for c in CASES)}
        self.params, self.out, self.cells = {}, {}, {}
        for s, k in CASES:
            if k not in self.params:
                P = bsw.Params(*[int(v) for v in z[f"{k}.params"]])
                for i, v in enumerate(z[f"{k}.mat"]):
                    P.mat[i] = int(v)
                self.params[k] = P
            self.out[s, k] = z[f"{s}.{k}.out"].astype(np.int32)
            self.cells[s, k] = z[f"{s}.{k}.cells"].astype(np.int64)
