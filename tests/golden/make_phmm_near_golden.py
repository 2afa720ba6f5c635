#!/usr/bin/env python3
"""Testcases whose f32 PairHMM result lies next to MIN_ACCEPTED = 1e-28, for the predictor's verify and
redo path (tests/test_phmm_predict.py): found with the oracle by varying one base quality of a
gen.phmm_batch read (seed 97) until the f32 result falls into (0.5e-28, 2e-28); at least 8 on each
side of 1e-28. Writes tests/golden/phmm_near_golden.npz (inputs only: the tests take the expected
outputs from the oracle) and records how long the search took.
    python tests/golden/make_phmm_near_golden.py"""
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PATH = os.path.join(HERE, "phmm_near_golden.npz")
LO, MID, HI = 0.5e-28, 1e-28, 2e-28
PER_SIDE = 10


def load():
    """[(read 5-tuple, hap)] of the fixture."""
    z = np.load(PATH)
    out, ro, ho = [], 0, 0
    for R, C in zip(z["rlen"], z["hlen"]):
        rd = tuple(z[f][ro:ro + R].tobytes() for f in ("rs", "q", "i", "d", "c"))
        out.append((rd, z["hap"][ho:ho + C].tobytes()))
        ro, ho = ro + int(R), ho + int(C)
    return out


def main():
    import oracle_lib
    from genomicsbench_palisade_amd import gen
    from genomicsbench_palisade_amd._tc import TestcaseArray
    o = oracle_lib.oracle()
    def f32(pair):
        ta = TestcaseArray.from_pairs([pair])  # owns the buffers the testcase points into
        return float(o.phmm_oracle_prob_f32(ctypes.addressof(ta.arr[0])))
    rng = np.random.default_rng(97)
    t0 = time.time()
    below, above, evals = [], [], 0
    while len(below) < PER_SIDE or len(above) < PER_SIDE:
        batch = gen.phmm_batch(rng, 24, 6)
        for read in batch.reads:
            for hap in batch.haps:
                base = f32((read, hap))
                evals += 1
                if not (1e-31 < base < 1e-25):
                    continue
                for pos in rng.permutation(len(read[0]))[:40]:
                    hit = None
                    for v in range(2, 64):
                        q = bytearray(read[1])
                        q[pos] = v
                        cand = ((read[0], bytes(q)) + read[2:], hap)
                        p = f32(cand)
                        evals += 1
                        if LO < p < HI and p != MID:
                            hit = (cand, p)
                            break
                    if hit:
                        side = below if hit[1] < MID else above
                        if len(side) < PER_SIDE:
                            side.append(hit[0])
                        break
    pairs = below + above
    took = time.time() - t0
    cat = lambda k: np.frombuffer(b"".join(p[0][k] for p in pairs), np.uint8)
    np.savez_compressed(PATH, rs=cat(0), q=cat(1), i=cat(2), d=cat(3), c=cat(4),
                        hap=np.frombuffer(b"".join(p[1] for p in pairs), np.uint8),
                        rlen=np.array([len(p[0][0]) for p in pairs], np.int32),
                        hlen=np.array([len(p[1]) for p in pairs], np.int32),
                        search_seconds=np.float64(took), search_evals=np.int64(evals))
    print(f"{len(below)} below and {len(above)} above MIN_ACCEPTED, {evals} oracle evaluations, {took:.1f} s")


if __name__ == "__main__":
    main()
