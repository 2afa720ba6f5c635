"""Records tests/golden/dbg_golden.npz: regions for gb_dbg_assemble with what the reference builds for them.

The live reference: benchmarks/dbg/debruijn.cpp of the reference tree, included unmodified by dbg_live_shim.cpp, and
benchmarks/dbg/common.cpp (setWindowPointers), compiled into a temporary directory outside the repository with
-ffunction-sections -Wl,--gc-sections, so that the reference driver's renamed main and getRead, which nothing calls,
are dropped with their htslib calls. The shim runs the k loop that the reference keeps as a comment in
assembleReadsAndDetectVariants and writes the cycle flag of every k tried and every node and edge of the final graph.

tests/dbg_ref.py restates the contract and must equal the live reference on every region before anything is stored.
The labels (dbg_sets.LABELS) are asserted here and again by tests/test_fmi_dbg.py.

Usage: python tests/golden/make_dbg_golden.py [reference root]
"""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import dbg_ref as ref  # noqa: E402
import dbg_sets  # noqa: E402
from make_abea_golden import REF_TREE  # noqa: E402

OUT = os.path.join(HERE, "dbg_golden.npz")
MAX_BYTES = 400 * 1024


class LiveDbg:
    """The reference's graph code behind dbg_live_shim.cpp, compiled in a temporary directory."""

    def __init__(self, ref_root=REF_TREE):
        src = os.path.join(ref_root, "benchmarks", "dbg")
        for f in ("debruijn.cpp", "common.cpp"):
            if not os.path.exists(os.path.join(src, f)):
                raise FileNotFoundError(os.path.join(src, f))
        self.dir = tempfile.mkdtemp(prefix="gb_dbg_live_")
        self.exe = os.path.join(self.dir, "dbg_live_shim")
        subprocess.check_call(["g++", "-O2", "-fopenmp", "-fpermissive", "-w", "-ffunction-sections",
                               "-Wl,--gc-sections", "-I", src, "-I", os.path.join(ref_root, "tools", "htslib"),
                               os.path.join(HERE, "dbg_live_shim.cpp"), os.path.join(src, "common.cpp"), "-o", self.exe])

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def _run(self, mode, data):
        fin, fout = os.path.join(self.dir, "in.bin"), os.path.join(self.dir, "out.bin")
        with open(fin, "wb") as f:
            f.write(data)
        subprocess.check_call([self.exe, mode, fin, fout])
        return open(fout, "rb").read()

    @staticmethod
    def encode(params, regions, reads):
        """regions: dbg.Regions, reads: dbg.Reads"""
        out = [struct.pack("<7i", len(regions), len(reads), *params)]
        for j in range(len(reads)):
            a, b = reads.read_off[j], reads.read_off[j + 1]
            out += [struct.pack("<iI", b - a, int(reads.flag[j])), reads.seq[a:b].tobytes(), reads.qual[a:b].tobytes()]
        for i in range(len(regions)):
            a, b = regions.ref_off[i], regions.ref_off[i + 1]
            out += [struct.pack("<4i", b - a, int(regions.ref_start[i]), int(regions.read_first[i]),
                                int(regions.read_last[i])), regions.ref_bytes[a:b].tobytes()]
        return b"".join(out)

    def graphs(self, params, regions, reads):
        raw, o, res = self._run("graphs", self.encode(params, regions, reads)), 0, []
        node = np.dtype([("src", "<i4"), ("off", "<i4"), ("colours", "<i4"), ("position", "<i4"), ("weight", "<i8"),
                         ("n_edges", "<i4"), ("edge_to", "<i4", 4), ("edge_weight", "<i8", 4)])
        for _ in range(len(regions)):
            n_tried = struct.unpack_from("<i", raw, o)[0]
            tried = np.frombuffer(raw, "<i4", 2 * n_tried, o + 4).reshape(-1, 2)
            o += 4 + 8 * n_tried
            n = struct.unpack_from("<i", raw, o)[0]
            a = np.frombuffer(raw, node, n, o + 4)
            o += 4 + node.itemsize * n
            res.append(([tuple(int(v) for v in x) for x in tried], {f: np.ascontiguousarray(a[f]) for f in node.names}))
        assert o == len(raw)
        return res

    def seconds(self, params, regions, reads):
        return struct.unpack("<d", self._run("time", self.encode(params, regions, reads)))[0]

    def windows(self, pos, end, longest, queries):
        data = struct.pack("<3i", len(pos), longest, len(queries))
        data += np.stack([pos, end], 1).astype("<u4").tobytes() + np.asarray(queries, "<i4").tobytes()
        return np.frombuffer(self._run("windows", data), "<i4").reshape(-1, 2)


def driver_queries(beg, stop, region):
    shift = max(100, min(1000, region // 2))
    return [(k, min(k + region, stop)) for k in range(beg, stop, shift)]


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REF_TREE
    live = LiveDbg(ref_root)
    try:
        store, names, seen = {}, [], set()
        for s in dbg_sets.fixture_sets():
            regions, reads = dbg_sets.packed(s)
            results = live.graphs(s["params"], regions, reads)
            st = dbg_sets.Stored.__new__(dbg_sets.Stored)
            st.regions, st.reads = regions, reads
            for i, (tried, g) in enumerate(results):
                t2, nodes = ref.assemble(*st.texts(i), s["params"])
                assert t2 == tried, (s["name"], i, t2, tried)
                g2 = ref.arrays(nodes)
                for f in dbg_sets.FIELDS:
                    assert g2[f].dtype == g[f].dtype and np.array_equal(g2[f], g[f]), (s["name"], i, f)
                seen.add(s["regions"][i][0])
                print(f"{s['name']}/{i} {s['regions'][i][0]}: tried {tried}, {len(g['src'])} nodes, "
                      f"{int(g['n_edges'].sum())} edges: equal", flush=True)
            dbg_sets.store_set(store, s, regions, reads, results)
            names.append(s["name"])
        missing = [x for x in dbg_sets.LABELS if x not in seen]
        assert not missing, f"labels without a case: {missing}"
        pos, end, longest, spans = dbg_sets.window_reads()
        expect = []
        for beg, stop, region in spans:
            expect.append(live.windows(pos, end, longest, driver_queries(beg, stop, region)))
        store["win_off"] = np.cumsum([0] + [len(e) for e in expect]).astype(np.int64)
        store["win_expect"] = np.concatenate(expect).astype(np.int32)
        store["win_empty"] = live.windows(pos[:0], end[:0], 0, driver_queries(0, 3000, 1500)).astype(np.int32)
    finally:
        live.close()
    store["set_names"] = np.array(names)
    store["label_names"] = np.array(list(dbg_sets.LABELS))
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, size
    print(f"wrote {OUT}: {size} bytes, {len(names)} sets")


if __name__ == "__main__":
    main()
