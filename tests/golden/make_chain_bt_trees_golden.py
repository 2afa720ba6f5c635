#!/usr/bin/env python3
"""Generates tests/golden/chain_bt_trees_golden.npz: the live reference's outputs on the constructed
call sets of tests/chain_shapes.py (far-parent trees, one set per size class of csrc/chain_bt.hip).

Build container only: needs oracle/_ref/libref_chain.so and libref_chain_bt.so (make ref). Recorded
per set, over all its calls (the ordinary ones between the special ones included):

  host_kernel (the scalar chain_dp)   {set}_scores, _dparent, _dtarget, _dpeak (chain_shapes.pack_dp)
  the testbed's mm_chain_dp, per (min_cnt, min_sc) pair k of `thresholds`
                                      {set}_u{k}    chains (score << 32 | count) of all calls
                                      {set}_nch{k}  chains per call
                                      {set}_dai{k}  chain anchors as int32 indices into their call,
                                                    concatenated, as first differences (cumsum restores)
                                      {set}_nan{k}  chain anchors per call

The anchors themselves are not stored: `spec` holds the sets' generator arguments (chain_shapes.SETS
as JSON) and the test rebuilds the calls from it. The file must stay no larger than the largest
fixture committed before it (chain_bt_golden.npz); DROP lists, in the order to take them, the cases
to leave out of the record if it does not (a case on a size-class boundary or one step past it is
never dropped; a dropped case still runs against the oracle)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chain_shapes  # noqa: E402
import oracle_lib  # noqa: E402

OUT = os.path.join(HERE, "chain_bt_trees_golden.npz")
LIMIT = os.path.getsize(os.path.join(HERE, "chain_bt_golden.npz"))
# (set, index among the set's special calls), in the order to drop
DROP = [("ldsw", 0), ("window", 0), ("cloud", 1)]


def anchor_indices(x, y, bx, by):
    """Indices into the call's anchors (x, y) of the chain anchors (bx, by); equal anchors are
    interchangeable, any of their indices serves."""
    where = {}
    for i, k in enumerate(zip(x.tolist(), y.tolist())):
        where.setdefault(k, i)
    return np.array([where[k] for k in zip(bx.tolist(), by.tolist())], np.int32)


def record(n_drop):
    dp_lib, bt_lib = oracle_lib.ref_chain(), oracle_lib.ref_chain_bt()
    dropped = DROP[:n_drop]
    fx = {"spec": np.array(json.dumps(chain_shapes.SETS)), "thresholds": np.array(chain_shapes.THRESHOLDS, np.int32),
          "dropped": np.array(json.dumps(dropped))}
    for name, spec in chain_shapes.SETS.items():
        calls, special = chain_shapes.build_set(spec)
        keep = np.ones(calls.ncalls, bool)
        for s, k in dropped:
            if s == name:
                keep[special[k]] = False
        amask = np.repeat(keep, np.diff(calls.offsets))
        dp = chain_shapes.pack_dp(calls.offsets, *oracle_lib.ref_chain_run(dp_lib, calls, 8))
        for key, a in zip(("scores", "dparent", "dtarget", "dpeak"), dp):
            fx["%s_%s" % (name, key)] = a[amask]
        for k, (mc, ms) in enumerate(chain_shapes.THRESHOLDS):
            us, an = oracle_lib.ref_chain_bt_run(bt_lib, calls, mc, ms)
            ai = []
            for c in range(calls.ncalls):
                o0, o1 = int(calls.offsets[c]), int(calls.offsets[c + 1])
                ai.append(anchor_indices(calls.x[o0:o1], calls.y[o0:o1], *an[c]) if keep[c] else np.zeros(0, np.int32))
            us = [u if keep[c] else u[:0] for c, u in enumerate(us)]
            fx["%s_u%d" % (name, k)] = np.concatenate(us)
            fx["%s_nch%d" % (name, k)] = np.array([len(u) for u in us], np.int32)
            fx["%s_dai%d" % (name, k)] = np.diff(np.concatenate(ai), prepend=np.int32(0)).astype(np.int32)
            fx["%s_nan%d" % (name, k)] = np.array([len(a) for a in ai], np.int32)
        print("set %-12s %2d calls, %6d anchors, chains %s" % (
            name, calls.ncalls, calls.nanchors, [int(fx["%s_nch%d" % (name, k)].sum()) for k in range(len(chain_shapes.THRESHOLDS))]))
    np.savez_compressed(OUT, **fx)
    return os.path.getsize(OUT)


def main():
    if oracle_lib.ref_chain() is None or oracle_lib.ref_chain_bt() is None:
        print("skipped: needs oracle/_ref/libref_chain.so and libref_chain_bt.so (make ref)")
        return 0
    for n_drop in range(len(DROP) + 1):
        size = record(n_drop)
        print("wrote %s: %d bytes (limit %d), dropped %s" % (OUT, size, LIMIT, DROP[:n_drop]))
        if size <= LIMIT:
            return 0
    raise SystemExit("the record does not fit with every droppable case dropped")


if __name__ == "__main__":
    sys.exit(main())
