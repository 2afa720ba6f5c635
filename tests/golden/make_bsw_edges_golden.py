"""Regenerate tests/golden/bsw_edges_golden.npz: the edge sets of tests/bsw_edges.py (main, long,
limit per match score), bwa v1 ksw_extend2's six outputs for each under the parameter sets of
bsw_edges.CASES (oracle/_ref/libref_bwa.so, built from the reference tree by `make -C oracle ref`),
the oracle's per-pair cell counts (ksw_extend2 does not count cells) and the parameter vectors and
matrices. Run in the build container only:

    python tests/golden/make_bsw_edges_golden.py

Refuses to write when the restatement (oracle/bsw_oracle.c) and ksw_extend2 disagree anywhere, and
prints the measured discrimination fractions that tests/test_bsw_edges.py puts a floor under."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bsw_edges  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    lib = oracle_lib.ref_bsw()
    if lib is None:
        raise SystemExit("oracle/_ref/libref_bwa.so missing: run `make -C oracle ref` first")
    sets = bsw_edges.input_sets()
    arrs = {}
    for s, p in sets.items():
        for k in bsw_edges.INPUT_KEYS:
            arrs[f"{s}.{k}"] = getattr(p, k)
        print(f"{s}: {p.n} pairs, {len(p.tgt) + len(p.qry)} bases")
    out = {}
    for s, k in bsw_edges.CASES:
        P = bsw_edges.params(k)
        arrs[f"{k}.params"], arrs[f"{k}.mat"] = P.as_array(), P.mat_array()
        ref = oracle_lib.ref_bsw_run(lib, sets[s], P)
        got, cells, tot = oracle_lib.bsw_oracle(sets[s], P, nthreads=8)
        bad = int((got != ref).any(axis=1).sum())
        if bad:
            raise SystemExit(f"{s} / {k}: the oracle differs from ksw_extend2 on {bad} pairs")
        assert tot == cells.sum()
        out[s, k] = ref
        arrs[f"{s}.{k}.out"] = ref
        arrs[f"{s}.{k}.cells"] = cells.astype(np.int32)
    print(f"oracle == ksw_extend2 on all {len(bsw_edges.CASES)} (set, parameter set) cases; top score "
          f"{max(int(o[:, 0].max()) for o in out.values())}")
    main_p = sets["main"]
    for what, base, kw, need in bsw_edges.BROKEN_RULES:
        broken = oracle_lib.ref_bsw_run(lib, main_p, bsw_edges.params(base, **kw))
        print(f"{what}: {bsw_edges.changed_fraction(broken, out['main', base]):.3f} of the main set changes "
              f"(required >= {need})")
    fo = bsw_edges.changed_fraction(out["main", "bigext"], out["main", "bigext_bonus"])
    fc = float((arrs["main.bigext.cells"] != arrs["main.bigext_bonus.cells"]).mean())
    print(f"bigext vs bigext_bonus: outputs {fo:.3f}, cell counts {fc:.3f} (required > 0 in either)")
    np.savez_compressed(bsw_edges.FIXTURE, **arrs)
    print(f"wrote {os.path.relpath(bsw_edges.FIXTURE, ROOT)}: {os.path.getsize(bsw_edges.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
