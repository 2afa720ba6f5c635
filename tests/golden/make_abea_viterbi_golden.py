"""Records tests/golden/abea_viterbi_golden.npz: items for gb_abea_hmm_align with the paths that f5c's CPU
profile_hmm_align returns for them.

The live reference is benchmarks/abea/src/eventalign.c. profile_hmm_align is `static inline` there, so a small C++
shim written here into a temporary directory outside the tree #includes that file unmodified and exposes one
extern "C" call on plain arrays (g++ -O2 -std=c++11 -ffp-contract=off -w, tools/htslib reached by -I, next to the
stand-in hdf5.h that make_abea_golden.py writes). The file's SAM writers, which nothing here calls, reference
seven htslib functions; abort-stubs written here satisfy the linker. Both string arguments are the item's
string: the reference reads only one of them, and takes the length from the first.

tests/abea_viterbi_ref.py restates the contract in numpy and must equal the live path on every item in every
field and bit. It counts the labels, each with a minimum (abea_viterbi_ref.MINIMA) asserted here and again by
tests/test_abea_viterbi.py on the stored counts; the two tie counts are stored without one. Every stored l_fm is
finite, and is a float32 widened (the reference keeps it in a double).

The two models are seeded (gen.abea_model), put on grids of 1/64 (level_mean) and 1/128 (level_stdv) and stored
as integers; event means are multiples of 1/8 and stored as int16. Per item the fixture stores the path's
length and per record the k-mer, the state and the bits of l_fm; a record's event follows from the states (the
row rises by one at every record but a 'K').

Usage: python tests/golden/make_abea_viterbi_golden.py [reference root]
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import abea_viterbi_ref as ref  # noqa: E402
from genomicsbench_palisade_amd import gen  # noqa: E402
from make_abea_golden import HDF5_STANDIN, REF_TREE  # noqa: E402

QUANTUM = 0.125
KMERS = (1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 256)
ROWS = (2, 3, 10, 63, 64, 65)
LONG_KMERS = (1, 17, 64, 129, 256)
LONG_ROWS = (300, 2000)
MAX_BYTES = 400 * 1024

SHIM = """\
#include "eventalign.c"
#include <cstring>
static std::vector<model_t> g_model;
extern "C" void viterbi_live_model(const float *model, int n) {
  g_model.resize((size_t)n);
  for (int k = 0; k < n; ++k)
    g_model[(size_t)k].level_mean = model[3 * k], g_model[(size_t)k].level_stdv = model[3 * k + 1],
    g_model[(size_t)k].level_log_stdv = model[3 * k + 2];
}
extern "C" int viterbi_live_align(const char *seq, int seq_len, const float *means, int n_events, float scale, float shift,
                                  float var, float log_var, int start, int stop, int rc, double events_per_base, int cap,
                                  int *event_idx, int *kmer_idx, char *state, double *l_fm) {
  std::vector<event_t> ev((size_t)n_events);
  std::memset(ev.data(), 0, sizeof(event_t) * ev.size());
  for (int i = 0; i < n_events; ++i) ev[(size_t)i].mean = means[i];
  scalings_t sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.scale = scale, sc.shift = shift, sc.var = var, sc.log_var = log_var;
  const std::string s(seq, seq + seq_len);
  const std::vector<HMMAlignmentState> a = profile_hmm_align(s, s, ev.data(), sc, g_model.data(), events_per_base, 0,
                                                             (uint8_t)rc, 6, (uint32_t)start, (uint32_t)stop,
                                                             (int8_t)(rc ? -1 : 1));
  const int n = (int)a.size();
  for (int i = 0; i < n && i < cap; ++i)
    event_idx[i] = (int)a[(size_t)i].event_idx, kmer_idx[i] = (int)a[(size_t)i].kmer_idx, state[i] = a[(size_t)i].state,
    l_fm[i] = a[(size_t)i].l_fm;
  return n;
}
"""

STUBS = "#include <stdlib.h>\n" + "".join(
    "void %s(void) { abort(); }\n" % name
    for name in ("bam_aux2i", "bam_aux_append", "bam_aux_get", "bam_destroy1", "bam_init1", "sam_hdr_write", "sam_write1"))


class LiveViterbi:
    """eventalign.c compiled in a temporary directory, called through the shim."""

    def __init__(self, ref_root):
        src = os.path.join(ref_root, "benchmarks", "abea", "src")
        hts = os.path.join(ref_root, "tools", "htslib")
        if not os.path.exists(os.path.join(src, "eventalign.c")):
            raise FileNotFoundError(src)
        self.dir = tempfile.mkdtemp(prefix="gb_abea_viterbi_")
        for name, text in (("hdf5.h", HDF5_STANDIN), ("shim.cpp", SHIM), ("stubs.c", STUBS)):
            with open(os.path.join(self.dir, name), "w") as fh:
                fh.write(text)
        flags = ["-O2", "-ffp-contract=off", "-fPIC", "-w"]
        shim_o, stubs_o = os.path.join(self.dir, "shim.o"), os.path.join(self.dir, "stubs.o")
        subprocess.check_call(["g++", "-std=c++11"] + flags + ["-I" + self.dir, "-I" + hts, "-I" + src, "-c",
                                                               os.path.join(self.dir, "shim.cpp"), "-o", shim_o])
        subprocess.check_call(["gcc"] + flags + ["-c", os.path.join(self.dir, "stubs.c"), "-o", stubs_o])
        so = os.path.join(self.dir, "libabea_viterbi_live.so")
        subprocess.check_call(["g++", "-shared", "-o", so, shim_o, stubs_o, "-lm"])
        self.lib = ctypes.CDLL(so)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        self.lib.viterbi_live_model.argtypes = [vp, ci]
        self.lib.viterbi_live_align.argtypes = [vp, ci, vp, ci, cf, cf, cf, cf, ci, ci, ci, ctypes.c_double, ci, vp, vp, vp, vp]
        self.model = None

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def align(self, x, idx=None):
        """profile_hmm_align of the items idx (all by default) of a gen.AbeaAlignItems: per item (event_idx int32,
        kmer_idx int32, state S1, l_fm float64)."""
        if self.model is not x.model:
            self.model = x.model
            self.lib.viterbi_live_model(x.model.ctypes.data, len(x.model))
        idx = range(x.n) if idx is None else idx
        out = []
        fd = os.dup(2)  # the reference warns on stderr about every byte other than ACGTN
        with open(os.devnull, "w") as dn:
            os.dup2(dn.fileno(), 2)
            try:
                for i in idx:
                    seq, ev, rd, it = x.item(i)
                    seq, ev = np.ascontiguousarray(seq), np.ascontiguousarray(ev)
                    cap = int(x.n_rows[i] + x.n_kmers[i])
                    e, k, s, v = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, "S1"), np.zeros(cap, np.float64)
                    n = self.lib.viterbi_live_align(seq.ctypes.data, len(seq), ev.ctypes.data, len(ev), float(rd["scale"]),
                                                    float(rd["shift"]), float(rd["var"]), float(rd["log_var"]),
                                                    int(it["event_start"]), int(it["event_stop"]), int(it["rc"]),
                                                    float(rd["events_per_base"]), cap, e.ctypes.data, k.ctypes.data,
                                                    s.ctypes.data, v.ctypes.data)
                    assert 0 < n <= cap, (i, n, cap)
                    out.append((e[:n], k[:n], s[:n], v[:n]))
            finally:
                os.dup2(fd, 2)
                os.close(fd)
        return out


def quantized_model(rng, grid=None):
    m = gen.abea_model(rng, grid)
    m[:, 0] = np.round(m[:, 0] * 64) / 64
    m[:, 1] = np.round(m[:, 1] * 128) / 128
    m[:, 2] = np.log(m[:, 1].astype(np.float64)).astype(np.float32)
    return m


def build_items(rng):
    """(models, [(group, model id, gen.AbeaAlignItems)])."""
    models = [quantized_model(rng), quantized_model(rng, grid=4.0)]
    parts = []

    def add(group, mid, shapes, **kw):
        kw.setdefault("quantum", QUANTUM)
        parts.append((group, mid, gen.abea_align_items(rng, shapes, model=models[mid], **kw)))

    # every size at which the kernel takes another path, crossed with the row counts, on both strands
    shapes = [(nk, rows) for nk in KMERS for rows in ROWS] + [(nk, rows) for rows in LONG_ROWS for nk in LONG_KMERS]
    for nk, rows in shapes:
        for rc in (0, 1):
            add("shape", 0, [(1, nk, rows)], rc=rc, epb=float(np.clip(rows / nk, 1.05, 4.0)))
    add("typical", 0, [(1, int(nk), int(nk * rng.uniform(1.2, 2.5))) for nk in rng.integers(90, 101, 24)])
    add("outlier", 0, [(1, nk, rows) for nk, rows in ((8, 16), (24, 48), (40, 90), (90, 180))], outlier_every=7)
    add("nonacgt", 0, [(1, nk, 2 * nk) for nk in (5, 14, 30, 90)], non_acgt=0.08)
    add("epb_one", 0, [(1, nk, rows) for nk, rows in ((4, 9), (16, 16), (30, 45), (100, 130))], epb=1.0)
    add("scaled", 0, [(1, nk, 2 * nk) for nk in (10, 25, 60)], scale=(0.8, 0.9), shift=(8.0, 12.0), var=(1.6, 2.4))
    add("scaled", 0, [(1, nk, 2 * nk) for nk in (10, 25, 60)], scale=(1.15, 1.25), shift=(-12.0, -8.0), var=(0.45, 0.7))
    grid = dict(quantum=2.0, scale=1.0, shift=0.0, var=1.0, noise=1.0, epb=2.0)
    add("grid", 1, [(1, nk, rows) for nk, rows in ((6, 6), (12, 30), (16, 40), (30, 50), (40, 60), (70, 100))], **grid)
    add("grid", 1, [(1, nk, rows) for nk, rows in ((12, 30), (30, 50), (70, 100))], homopolymer=20, **grid)
    return models, parts


def equal(got, want):
    """A restated or library path (event_idx, kmer_idx, state, l_fm float32) against a live one (l_fm float64)."""
    return (len(got[0]) == len(want[0]) and (got[0] == want[0]).all() and (got[1] == want[1]).all()
            and (got[2] == want[2]).all() and (got[3].astype(np.float64) == want[3]).all())


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REF_TREE
    live = LiveViterbi(ref_root)
    rng = np.random.default_rng(20261022)
    models, parts = build_items(rng)
    labels = dict.fromkeys(ref.LABELS, 0)
    lens, kmer, state, lfm = [], [], [], []
    for group, mid, x in parts:
        want = live.align(x)
        for i in range(x.n):
            got = ref.align_item(x, i, labels)
            assert equal(got, want[i]), (group, i, x.items[i])
            v = want[i][3]
            assert np.isfinite(v).all() and (v.astype(np.float32).astype(np.float64) == v).all(), (group, i)
            lens.append(len(v)), kmer.append(want[i][1]), state.append(want[i][2]), lfm.append(v.astype(np.float32))
        print(f"{group:8s} {x.n:3d} items, k-mers {x.n_kmers[0]:3d} rows {x.n_rows[0]:4d} records {lens[-1]:4d} "
              f"l_fm {lfm[-1][-1]:.3f}", flush=True)
    live.close()
    for k in ref.LABELS:
        print(f"label {k:22s} {labels[k]:9d} (min {ref.MINIMA.get(k, 0)})")
    short = [k for k, v in ref.MINIMA.items() if labels[k] < v]
    assert not short, f"labels below their minimum: {short}"
    allx = gen.AbeaAlignItems.concat([x for _, _, x in parts])
    ev_q = allx.events / QUANTUM
    assert (ev_q == np.round(ev_q)).all() and np.abs(ev_q).max() < 32768
    mq = np.stack(models)
    assert (mq[..., 0] * 64 == np.round(mq[..., 0] * 64)).all() and (mq[..., 1] * 128 == np.round(mq[..., 1] * 128)).all()
    out = os.path.join(HERE, "abea_viterbi_golden.npz")
    np.savez_compressed(
        out, model_mean_q=(mq[..., 0] * 64).astype(np.uint16), model_stdv_q=(mq[..., 1] * 128).astype(np.uint16),
        model_log_stdv=mq[..., 2], seqs=allx.seqs, events_q=ev_q.astype(np.int16), reads=allx.reads, items=allx.items,
        group=np.concatenate([[g] * x.n for g, _, x in parts]),
        model_id=np.concatenate([[m] * x.n for _, m, x in parts]).astype(np.int8),
        path_len=np.array(lens, np.int32), path_kmer=np.concatenate(kmer).astype(np.uint8),
        path_state=np.concatenate(state).view(np.uint8), path_l_fm_bits=np.concatenate(lfm).view(np.uint32),
        label_names=np.array(list(labels)), label_counts=np.array(list(labels.values()), np.int64),
        label_minima=np.array([ref.MINIMA.get(k, 0) for k in labels], np.int64))
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {allx.n} items, {sum(lens)} records")
    assert os.path.getsize(out) <= MAX_BYTES, "thin the long-row shapes first"


if __name__ == "__main__":
    main()
