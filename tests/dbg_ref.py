"""A short restatement of the dbg contract (include/gb_fmi_dbg.h; the reference's benchmarks/dbg/debruijn.cpp) over
Python dicts. tests/golden/make_dbg_golden.py checks it against the live reference on every fixture region."""
import numpy as np

FIELDS = ("src", "off", "colours", "position", "weight", "n_edges", "edge_to", "edge_weight")


def graph(ref, ref_start, reads, k, min_qual=20):
    """ref: bytes; reads: (pool index, sequence bytes, qualities, flag) in pool order. Nodes as a list of dicts in
    order of first visit."""
    ids, nodes = {}, []

    def visit(kmer, src, off, colour, pos, w):
        i = ids.get(kmer)
        if i is None:
            ids[kmer] = i = len(nodes)
            nodes.append({"src": src, "off": off, "colours": colour, "position": pos, "weight": w, "to": [], "ew": []})
        else:
            nodes[i]["colours"] |= colour
            nodes[i]["weight"] += w
        return i

    def add(text, src, i, colour, pos, w):
        a = visit(text[i:i + k], src, i, colour, pos, w)
        b = visit(text[i + 1:i + 1 + k], src, i + 1, colour, pos + 1 if pos >= 0 else -1, w)
        n = nodes[a]
        if b in n["to"]:
            n["ew"][n["to"].index(b)] += w
        elif len(n["to"]) < 4:
            n["to"].append(b)
            n["ew"].append(w)

    for i in range(len(ref) - k - 1):
        add(ref, -1, i, 1, ref_start + i, 1)
    for j, seq, qual, flag in reads:
        if flag & 512:
            continue
        for i in range(len(seq) - k - 1):
            q = int(min(qual[i:i + k + 1]))
            if q >= min_qual and b"N" not in seq[i:i + k + 1]:
                add(seq, j, i, 2, -1, q)
    return nodes


def cyclic(nodes, min_weight=40):
    """A directed cycle among the edges that are not (end node read-only and weight < min_weight)."""
    out = [[t for t, w in zip(n["to"], n["ew"]) if not (nodes[t]["colours"] == 2 and w < min_weight)] for n in nodes]
    indeg = [0] * len(nodes)
    for ts in out:
        for t in ts:
            indeg[t] += 1
    work = [i for i, d in enumerate(indeg) if d == 0]
    removed = 0
    while work:
        i = work.pop()
        removed += 1
        for t in out[i]:
            indeg[t] -= 1
            if indeg[t] == 0:
                work.append(t)
    return int(removed < len(nodes))


def assemble(ref, ref_start, reads, params=(15, 5, 50, 20, 40)):
    """(tried: [(k, cyclic)], nodes of the final graph)"""
    k0, k_step, k_max, min_qual, min_weight = params
    k, tried = k0, []
    while True:
        nodes = graph(ref, ref_start, reads, k, min_qual)
        c = cyclic(nodes, min_weight)
        tried.append((k, c))
        if not c or k > k_max:
            return tried, nodes
        k += k_step


def arrays(nodes):
    """The export's arrays of a node list."""
    n = len(nodes)
    g = {f: np.array([x[f] for x in nodes], np.int64 if f == "weight" else np.int32).reshape(n)
         for f in ("src", "off", "colours", "position", "weight")}
    g["n_edges"] = np.array([len(x["to"]) for x in nodes], np.int32).reshape(n)
    g["edge_to"] = np.full((n, 4), -1, np.int32)
    g["edge_weight"] = np.zeros((n, 4), np.int64)
    for i, x in enumerate(nodes):
        g["edge_to"][i, :len(x["to"])] = x["to"]
        g["edge_weight"][i, :len(x["ew"])] = x["ew"]
    return g


def summary(tried, g):
    return {"k": tried[-1][0], "n_graphs": len(tried), "cyclic": tried[-1][1], "n_nodes": len(g["src"]),
            "n_edges": int(g["n_edges"].sum()), "n_ref_and_read": int((g["colours"] == 3).sum()),
            "node_weight_sum": int(g["weight"].sum()), "edge_weight_sum": int(g["edge_weight"].sum())}
