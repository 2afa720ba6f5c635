"""Records tests/golden/chain_extd2_edges_golden.npz: the items of tests/chain_extd2_edges.py (piece, class, LDS
and launch-bucket edges of gb_chain_extd2) with the records and CIGARs that minimap2's ksw_extd2_sse returns.

The live reference is make_chain_extd2_golden.py's LiveExtd2: tools/minimap2/ksw2_extd2_sse.c of the reference
tree, compiled unmodified in a temporary directory. Every item is recorded through it. The numpy restatement
(tests/chain_extd2_ref.py) is too slow for the wide items; it runs on the bucket-edge items of at most
chain_extd2_edges.RESTATED_ROWS rows, where it must equal the live result, and on every item that the reference
stops early (zdropped), where it must equal the live result too and tells the row in which the sweep stopped:
the record alone does not, and the labels and the cell count of the timing call need it.

Stored: the parameter set, the bases once per pair, the item records (the items of a pair share q_off and t_off),
the 12-word result records, the CIGAR words and lengths, the rows each item swept, the label names and counts.

Usage: python tests/golden/make_chain_extd2_edges_golden.py [reference root]
"""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import chain_extd2_edges as ee  # noqa: E402
import chain_extd2_ref as ref  # noqa: E402
from make_chain_extd2_golden import REF_TREE, LiveExtd2, equal  # noqa: E402

OUT = os.path.join(HERE, "chain_extd2_edges_golden.npz")


def restated_rows(x, i, want):
    """The rows item i swept, from the restatement's count of in-band cells; the restatement equals `want`."""
    count = collections.defaultdict(int, cells=0)
    got = ref.align_item(x, i, labels=count)
    assert equal(got, want), ("restatement", x.items[i], got[0], want[0])
    R = ee.rows_of(x.items[i])
    k = int(np.searchsorted(R.cells, count["cells"]))
    assert k < R.n and R.cells[k] == count["cells"], (x.items[i], count["cells"])
    return k + 1


def record(ref_root=REF_TREE):
    live = LiveExtd2(ref_root)
    try:
        x = ee.build_items()
        recs, cigs, rows, restated = [], [], [], 0
        for i in range(x.n):
            it = x.items[i]
            want = live.align_item(x, i)
            R = ee.rows_of(it)
            n = int(it["qlen"]) + int(it["tlen"]) - 1
            edge = R.state in ee.BUCKET_STATES and n <= ee.RESTATED_ROWS
            if want[0][1]:
                rows.append(restated_rows(x, i, want))
            else:
                rows.append(n)
                if edge:
                    assert equal(ref.align_item(x, i), want), ("restatement", it)
            restated += edge
            recs.append(want[0]), cigs.append(want[1])
            print(f"{i:3d} {int(it['qlen']):5d} x {int(it['tlen']):5d} w {int(it['w']):5d} flag {int(it['flag']):#04x}: class {R.cls}, "
                  f"span up to {int(R.span.max())}, {int(R.pieces.max())} pieces, state {R.state}, rows {rows[-1]} of {n}, "
                  f"{len(want[1])} words", flush=True)
        assert restated >= 8, restated
    finally:
        live.close()
    res = np.array(recs, np.int32)
    rows = np.array(rows, np.int32)
    counts = ee.count_labels(x, res, rows)
    for k in ee.LABELS:
        print(f"label {k:30s} {counts[k]:4d}")
    ee.check_labels(counts)
    none, of = ee.cigarless(x, res)
    print(f"{none} of {of} items that neither z-drop nor leave the band end without a CIGAR")
    assert 4 * none <= of, (none, of)
    lens = np.array([len(c) for c in cigs], np.int32)
    return dict(params=x.params, seqs=x.seqs, items=x.items, res=res, cigar=np.concatenate(cigs).astype(np.uint32),
                cigar_len=lens, rows_swept=rows, label_names=np.array(list(ee.LABELS)),
                label_counts=np.array([counts[k] for k in ee.LABELS], np.int64))


def main():
    data = record(sys.argv[1] if len(sys.argv) > 1 else REF_TREE)
    ee.save(OUT, **data)
    fx = ee.Fixture(OUT)
    print(f"{OUT}: {fx.size} bytes, {fx.n} items over {len(data['seqs'])} bases, {len(data['cigar'])} CIGAR words")
    print("items per class:", {c: int((fx.cls == c).sum()) for c in range(4)})
    print("items per piece count:", {p: int((fx.pieces == p).sum()) for p in sorted(set(fx.pieces.tolist()))})
    print("launch groups:", sorted(set(fx.group.tolist())))
    assert fx.size <= ee.MAX_BYTES, fx.size


if __name__ == "__main__":
    main()
