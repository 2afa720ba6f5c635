"""Records tests/golden/poa_edges_golden.npz: the items of tests/poa_edges.py (column-split edges, long gaps, odd
scoring, the length limit) with what the reference's spoa returns for them.

The live reference is make_poa_golden.py's: spoa's SISD engine compiled unmodified with poa_live_shim.cpp in a
temporary directory. Every item's view comes from the live graph and its pairs from the live align. The
restatement tests/poa_ref.py must give the same pairs on every item of at most REF_CELLS cells and on the three
square items, and the same consensus, node count and rounds on every odd-scoring window; an item's score is the
restatement's final H value, of the run whose pairs equal the live ones. The length-limit item is too large for
the restatement: it is stored as a checksum of the live pairs, without a score.

Stored: the parameter sets with their subtypes; per item its group, parameter set, kind, window and round, view,
sequence, score, pair count and pairs (node and position columns apart, which compress better); the odd windows'
reads once, and per parameter set and window the consensus, node count, alignments done and cells; the
length-limit item's view, pair count and checksums; the label counts (poa_edges.LABELS).

Usage: python tests/golden/make_poa_edges_golden.py [reference root]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import poa_edges as pe  # noqa: E402
import poa_ref as ref  # noqa: E402
from genomicsbench_palisade_amd import poa  # noqa: E402
from make_poa_golden import REF_CELLS, REF_TREE, LivePoa, cat, offs  # noqa: E402

OUT = os.path.join(HERE, "poa_edges_golden.npz")


def last_round(live, p, reads):
    """(view, sequence, pairs) of the window's last alignment."""
    got = {}
    live.window(p, reads, on_alignment=lambda k, v, r, pr: got.update({k: (v, r, pr.copy())}))
    return got[len(reads) - 1]


def restated(p, view, seq, pairs, what):
    """The restatement's score, of a run whose pairs equal the live ones."""
    rp, score = ref.align(p, ref.View(*view), seq)
    assert rp == [(int(a), int(b)) for a, b in pairs], ("pairs", what)
    return score


def record(ref_root=REF_TREE):
    live = LivePoa(ref_root)
    try:
        for name, (p, sub) in pe.PARAM_SETS.items():
            assert poa.subtype(poa.params(*p)) == sub == ref.subtype(p)[0], name
        items, runs, missed = [], {}, []

        def add(group, ps, kind, win, rnd, view, seq, pairs, score):
            items.append(dict(group=group, ps=ps, kind=kind, win=win, round=rnd, view=view, seq=bytes(seq),
                              pairs=np.asarray(pairs, np.int32).reshape(-1, 2), n_pairs=len(pairs), score=score))

        for ps, L, kind, reads, seq in pe.split_items():
            p = pe.PARAM_SETS[ps][0]
            view, r, pairs = last_round(live, p, reads + [seq])
            assert r == seq and len(view[0]) * L <= REF_CELLS, (ps, L, kind, len(view[0]))
            add("split", ps, kind, -1, 3, view, seq, pairs, restated(p, view, seq, pairs, (ps, L, kind)))
            run = pe.longest_inserted_run(pairs)
            runs[(ps, L, kind)] = (run, len(view[0]))
            if kind == "disjoint" and pe.PARAM_SETS[ps][1] != poa.LINEAR and run < L - pe.CAP_SLACK:
                missed.append((ps, L, run))
            print(f"split {ps} {L} {kind}: {len(view[0])} nodes, {len(pairs)} pairs, longest inserted run {run}", flush=True)
        assert not missed, f"disjoint items whose longest inserted run misses the cap (change the draw in poa_edges.split_items): {missed}"
        for ps, L, reads in pe.square_windows():
            p = pe.PARAM_SETS[ps][0]
            view, r, pairs = last_round(live, p, reads)
            assert len(r) == L
            add("square", ps, "", -1, 2, view, r, pairs, restated(p, view, r, pairs, (ps, L)))
            print(f"square {ps} {L}: {len(view[0])} nodes, {len(pairs)} pairs", flush=True)
        windows, win = pe.odd_windows(), []
        for ps in pe.ODD_SETS:
            p = pe.PARAM_SETS[ps][0]
            for w, reads in enumerate(windows):
                mine, scores = [], {}
                exp = live.window(p, reads, on_alignment=lambda k, v, r, pr: mine.append((k, v, r, pr.copy())))

                def on_restated(k, v, r, pairs, score):
                    scores[k] = (v, pairs, score)

                got = ref.window(p, reads, on_alignment=on_restated)
                assert got == (exp[0], exp[1], exp[2], exp[3], ref.rank_checksum(exp[4])), (ps, w)
                for k, view, r, pairs in mine:
                    v, rp, score = scores[k]
                    for a, b in zip((v.base, v.id, v.out, v.in_end, v.pred), view):
                        assert list(a) == [int(x) for x in b], ("view", ps, w, k)
                    assert rp == [(int(a), int(b)) for a, b in pairs] and len(view[0]) * len(r) <= REF_CELLS, (ps, w, k)
                    add("odd", ps, "", w, k, view, r, pairs, score)
                win.append((ps, w, exp[0], exp[1], exp[2], exp[3]))
            print(f"odd {ps}: {sum(1 for it in items if it['ps'] == ps)} items", flush=True)
        reads, seq = pe.limit_reads()
        lview, r, lpairs = last_round(live, pe.PARAM_SETS["bench"][0], reads + [seq])
        assert r == seq and len(seq) == poa.MAX_LEN and len(lpairs) > 0
        assert pe.longest_inserted_run(lpairs) >= poa.MAX_LEN - pe.CAP_SLACK
        counts = pe.count_labels(items)
        pe.check_labels(counts)
        names = list(pe.PARAM_NAMES)
        all_reads = [r for w in windows for r in w]
        data = dict(
            param_names=np.array(names), params=np.array([pe.PARAM_SETS[k][0] for k in names], np.int8),
            param_sub=np.array([pe.PARAM_SETS[k][1] for k in names], np.int32),
            item_group=np.array([it["group"] for it in items]), item_kind=np.array([it["kind"] for it in items]),
            item_params=np.array([names.index(it["ps"]) for it in items], np.int32),
            item_win=np.array([it["win"] for it in items], np.int32), item_round=np.array([it["round"] for it in items], np.int32),
            item_node_off=offs([it["view"][0] for it in items]), item_edge_off=offs([it["view"][4] for it in items]),
            node_base=cat([it["view"][0] for it in items], np.uint8), node_id=cat([it["view"][1] for it in items], np.int32),
            node_out=cat([it["view"][2] for it in items], np.uint8), in_end=cat([it["view"][3] for it in items], np.int32),
            pred_rank=cat([it["view"][4] for it in items], np.int32),
            item_seq_off=offs([it["seq"] for it in items]),
            item_seq=cat([np.frombuffer(it["seq"], np.uint8) for it in items], np.uint8),
            item_score=np.array([it["score"] for it in items], np.int32),
            item_pairs=np.array([it["n_pairs"] for it in items], np.int64),
            item_whole=np.ones(len(items), np.uint8), item_pair_sum=np.array([pe.checksum(it["pairs"]) for it in items], np.int64),
            item_pair_off=offs([it["pairs"] for it in items]),
            pair_node=cat([it["pairs"][:, 0] for it in items], np.int32), pair_pos=cat([it["pairs"][:, 1] for it in items], np.int32),
            odd_win_read_off=offs(windows), odd_read_off=offs(all_reads),
            odd_read_bytes=cat([np.frombuffer(r, np.uint8) for r in all_reads], np.uint8),
            win_params=np.array([names.index(w[0]) for w in win], np.int32), win_reads=np.array([w[1] for w in win], np.int32),
            win_cons=cat([np.frombuffer(w[2], np.uint8) for w in win], np.uint8), win_cons_off=offs([w[2] for w in win]),
            win_nodes=np.array([w[3] for w in win], np.int32), win_done=np.array([w[4] for w in win], np.int64),
            win_cells=np.array([w[5] for w in win], np.int64),
            limit_node_base=np.asarray(lview[0], np.uint8), limit_node_id=np.asarray(lview[1], np.int32),
            limit_node_out=np.asarray(lview[2], np.uint8), limit_in_end=np.asarray(lview[3], np.int32),
            limit_pred_rank=np.asarray(lview[4], np.int32), limit_seq_sum=np.array(pe.checksum(np.frombuffer(seq, np.uint8)), np.int64),
            limit_pairs=np.array(len(lpairs), np.int64), limit_pair_sum=np.array(pe.checksum(lpairs), np.int64),
            label_names=np.array(list(pe.LABELS)), label_counts=np.array([counts[k] for k in pe.LABELS], np.int64),
            ref_cells=np.array([REF_CELLS], np.int64))
        return data, runs
    finally:
        live.close()


def main():
    data, runs = record(sys.argv[1] if len(sys.argv) > 1 else REF_TREE)
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    groups = [str(g) for g in data["item_group"]]
    print(f"{OUT}: {size} bytes, {len(groups)} items ({ {g: groups.count(g) for g in ('split', 'square', 'odd')} }), "
          f"{len(data['win_params'])} windows, length-limit item of {int(data['limit_pairs'])} pairs")
    short = {k: v for k, v in zip(data["label_names"].tolist(), data["label_counts"].tolist()) if not k.startswith("split/")}
    print(short)
    worst = min((run - L, ps, L) for (ps, L, kind), (run, _) in runs.items() if kind == "disjoint" and ps != "spoa-linear")
    print(f"disjoint items' shortest inserted run: L - {-worst[0]} ({worst[1]}, {worst[2]}); nodes "
          f"{min(n for _, n in runs.values())} .. {max(n for _, n in runs.values())}")
    assert size <= pe.MAX_BYTES, size


if __name__ == "__main__":
    main()
