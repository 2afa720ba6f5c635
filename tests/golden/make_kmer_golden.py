"""Records tests/golden/kmer_golden.npz: read sets for gb_kmer_count and gb_kmer_index with what the reference's
Flye returns for them.

The live reference: tools/Flye/src/sequence/{vertex_index,sequence_container,sequence}.cpp of the reference tree,
compiled unmodified with lib/libcuckoo and kmer_live_shim.cpp into a temporary directory outside the repository
(-lz -pthread, one thread), beside an empty stand-in for the palisade_header.h that sequence_container.cpp
includes. One process per set, because the reference sizes its flat table once per process. KmerCounter::count(true)
runs for k <= 13 and for the one k = 17 set (8.6 GB of host memory), count(false) for k >= 14 and, as a
cross-check, again for every k <= 13 set; the index sets run VertexIndex::countKmers and
buildIndexUnevenCoverage and are read back through iterKmerPos, kmerFreq and isRepetitive over every canonical
code of the reads.

tests/kmer_ref.py restates the contract and must equal the live reference on every set: the frequency of every
canonical code of the reads, of every non-canonical form and of absent codes, getKmerNum, and for the index sets
every list, the repetitive set and the repetitive frequency. The labels (LABELS) are counted and asserted here and
again by tests/test_fmi_kmer.py on the stored counts.

Stored: small sets whole (reads, parameters, codes, counts, index CSR, repetitive codes, scalars); larger sets as
reads (or the recipe of generated reads), statistics, histogram and a checksum of each array.

Usage: python tests/golden/make_kmer_golden.py [reference root]
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

import kmer_ref as ref  # noqa: E402
import kmer_sets  # noqa: E402
from make_abea_golden import REF_TREE  # noqa: E402

OUT = os.path.join(HERE, "kmer_golden.npz")
MAX_BYTES = 400 * 1024
FLYE_SRCS = ("vertex_index.cpp", "sequence_container.cpp", "sequence.cpp")


class LiveFlye:
    """The reference's k-mer counter and index with kmer_live_shim.cpp, compiled in a temporary directory."""

    def __init__(self, ref_root=REF_TREE):
        flye = os.path.join(ref_root, "tools", "Flye")
        srcs = [os.path.join(flye, "src", "sequence", s) for s in FLYE_SRCS]
        for s in srcs:
            if not os.path.exists(s):
                raise FileNotFoundError(s)
        self.dir = tempfile.mkdtemp(prefix="gb_kmer_live_")
        open(os.path.join(self.dir, "palisade_header.h"), "w").close()
        self.exe = os.path.join(self.dir, "kmer_live_shim")
        inc = ["-I", os.path.join(flye, "lib", "libcuckoo"), "-I", os.path.join(flye, "src"), "-I", self.dir]
        objs = []
        for s in srcs:
            o = os.path.join(self.dir, os.path.basename(s) + ".o")
            subprocess.check_call(["g++", "-std=c++11", "-O2", "-w", *inc, "-c", s, "-o", o])
            objs.append(o)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-w", "-fno-access-control", *inc,
                               os.path.join(HERE, "kmer_live_shim.cpp"), *objs, "-o", self.exe, "-lz", "-pthread"])

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def run(self, k, reads, queries, flat, index=None, n_index=0):
        """getKmerNum, getFreq of each query and, with index = (min_freq, select_rate, tandem_freq, repeat_rate), the
        repetitive frequency and (isRepetitive, positions) of each of the first n_index queries."""
        queries = np.ascontiguousarray(queries, np.uint64)
        mf, sr, tf, rr = index if index else (0, 0.0, 0, 0.0)
        fin, fout = os.path.join(self.dir, "in.bin"), os.path.join(self.dir, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<7q2f", k, int(flat), len(reads), len(queries), n_index if index else 0, mf, tf,
                                np.float32(sr), np.float32(rr)))
            for r in reads:
                f.write(struct.pack("<q", len(r)))
                f.write(np.asarray(r, np.uint8).tobytes())
            f.write(queries.tobytes())
        subprocess.check_call([self.exe, fin, fout], stderr=subprocess.DEVNULL)
        raw = open(fout, "rb").read()
        num, self.count_seconds = struct.unpack_from("<qd", raw, 0)
        freq = np.frombuffer(raw, np.uint64, len(queries), 16).copy()
        if not index:
            return num, freq
        o = 16 + 8 * len(queries)
        rep_freq = struct.unpack_from("<q", raw, o)[0]
        o += 8
        is_rep, lists = [], []
        for _ in range(n_index):
            rep, size = struct.unpack_from("<Bq", raw, o)
            o += 9
            is_rep.append(bool(rep))
            lists.append(np.frombuffer(raw, np.int64, size, o).copy())
            o += 8 * size
        assert o == len(raw)
        return num, freq, rep_freq, np.array(is_rep, bool), lists


def queries_of(k, reads):
    """(all canonical codes of the reads ascending, the non-canonical forms of those that have one, absent codes:
    random ones and the reads' last k-mers)"""
    fwd = [ref.codes_of(r, k) for r in reads]
    f = np.concatenate([x[0] for x in fwd]) if fwd else np.zeros(0, np.uint64)
    rc = np.concatenate([x[1] for x in fwd]) if fwd else np.zeros(0, np.uint64)
    can, other = np.minimum(f, rc), np.maximum(f, rc)
    other = np.unique(other[other != can])
    can = np.unique(can)
    rng = np.random.default_rng(k)
    absent = np.unique(rng.integers(0, 1 << (2 * k), 64, dtype=np.uint64))
    # the k-mer that ends each read, which the reference's walk leaves out: counted only where it occurs elsewhere
    last = [ref.canonical(np.append(r, np.uint8(65)), k)[0][-1:] for r in reads if len(r) >= k]
    absent = np.unique(np.concatenate([absent] + last))
    absent = absent[~np.isin(absent, can) & ~np.isin(absent, other)]
    return can, other, absent


def check_live(live, s):
    """The restatement against the live reference on one set; returns what the restatement gives."""
    k, reads = s["k"], s["reads"]
    codes, counts = ref.count(k, reads)
    can, other, absent = queries_of(k, reads)
    assert (can == codes).all(), s["name"]
    q = np.concatenate([can, other, absent])
    want = ref.freq(codes, counts, q)
    assert (want[:len(can)] == counts).all() and not want[len(can):].any()
    modes = [True, False] if k <= 13 else [bool(s.get("flat"))]
    for flat in modes:
        num, freq = live.run(k, reads, q, flat)
        assert num == len(codes), (s["name"], flat, num, len(codes))
        assert (freq == want).all(), (s["name"], flat, "getFreq differs")
    out = {"codes": codes, "counts": counts, "index": []}
    for p in s.get("index", []):
        num, freq, rep_freq, is_rep, lists = live.run(k, reads, q, True, p, len(can))
        assert num == len(codes) and (freq == want).all(), (s["name"], p)
        e = ref.index(k, reads, codes, counts, *p)
        assert e[4] == rep_freq, (s["name"], p, e[4], rep_freq)
        assert np.array_equal(can[is_rep], e[3]), (s["name"], p, "repetitive set")
        listed = np.array([len(x) > 0 for x in lists], bool)
        assert np.array_equal(can[listed], e[0]), (s["name"], p, "codes")
        live_pos = np.concatenate([x for x in lists if len(x)]) if listed.any() else np.zeros(0, np.int64)
        assert np.array_equal(live_pos, e[2]), (s["name"], p, "positions")
        assert np.array_equal(np.cumsum([len(x) for x in lists if len(x)]), e[1][1:]), (s["name"], p, "offsets")
        out["index"].append(e)
    return out


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REF_TREE
    live = LiveFlye(ref_root)
    try:
        store, labels = {}, {}
        names = []
        for s in kmer_sets.fixture_sets():
            got = check_live(live, s)
            kmer_sets.count_labels(labels, s, got)
            kmer_sets.store_set(store, s, got)
            names.append(s["name"])
            print(f"{s['name']}: k {s['k']}, {len(s['reads'])} reads, {len(got['codes'])} codes, "
                  f"{int(got['counts'].sum())} occurrences, {len(got['index'])} index runs: equal", flush=True)
    finally:
        live.close()
    missing = [name for name in kmer_sets.LABELS if not labels.get(name)]
    assert not missing, f"labels without a case: {missing}"
    store["set_names"] = np.array(names)
    store["label_names"] = np.array(list(kmer_sets.LABELS))
    store["label_counts"] = np.array([labels[name] for name in kmer_sets.LABELS], np.int64)
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, size
    print(f"wrote {OUT}: {size} bytes, {len(names)} sets")


if __name__ == "__main__":
    main()
