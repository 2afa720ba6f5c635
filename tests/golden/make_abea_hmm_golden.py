"""Records tests/golden/abea_hmm_golden.npz: items for gb_abea_hmm_score with what f5c's CPU profile_hmm_score
returns for them.

The live reference is benchmarks/abea/src/hmm.c, compiled unmodified in a temporary directory outside the tree
(g++ -O2 -std=c++11 -ffp-contract=off, tools/htslib reached by -I), next to the stand-in hdf5.h that
make_abea_golden.py writes and a small C++ shim written here, which defines flogsum_lookup, calls
p7_FLogsumInit() and calls profile_hmm_score() on plain arrays. Both string arguments are the item's string: the
reference reads only one of them, and takes the length from the first.

tests/abea_hmm_ref.py restates the contract in numpy and must equal the live score in every bit on every item.
It counts the labels, each with a minimum asserted here and again by tests/test_abea_hmm.py on the stored
counts. Every stored score is finite: -infinity or NaN would compare equal to many wrong kernels.

The two models are seeded (gen.abea_cpg_model), put on grids of 1/64 (level_mean) and 1/128 (level_stdv) and
stored as integers; event means are multiples of 1/8 and stored as int16.

Usage: python tests/golden/make_abea_hmm_golden.py [reference root]
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

import abea_hmm_ref as ref  # noqa: E402
from genomicsbench_palisade_amd import gen  # noqa: E402
from make_abea_golden import HDF5_STANDIN, REF_TREE  # noqa: E402

QUANTUM = 0.125
KMERS = (1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 216, 256)
ROWS = (1, 2, 3, 10, 63, 64, 65, 300, 2000)

SHIM = """\
#include "f5c.h"
#include "logsum.h"
#include <cstring>
#include <vector>
float flogsum_lookup[p7_LOGSUM_TBL];
float profile_hmm_score(const char *m_seq, const char *m_rc_seq, event_t *event, scalings_t scaling, model_t *cpgmodel,
                        uint32_t event_start_idx, uint32_t event_stop_idx, uint8_t strand, int8_t event_stride,
                        uint8_t rc, double events_per_base, uint32_t hmm_flags);  // hmm.c:684
static std::vector<model_t> g_model;
extern "C" void hmm_live_init(float *table_out) {
  p7_FLogsumInit();
  std::memcpy(table_out, flogsum_lookup, sizeof(flogsum_lookup));
}
extern "C" void hmm_live_model(const float *model, int n) {
  g_model.resize((size_t)n);
  for (int k = 0; k < n; ++k)
    g_model[(size_t)k].level_mean = model[3 * k], g_model[(size_t)k].level_stdv = model[3 * k + 1],
    g_model[(size_t)k].level_log_stdv = model[3 * k + 2];
}
extern "C" float hmm_live_score(const char *seq, int seq_len, const float *means, int n_events, float scale, float shift,
                                float var, float log_var, int start, int stop, int rc, double events_per_base, int flags) {
  std::vector<event_t> ev((size_t)n_events);
  std::memset(ev.data(), 0, sizeof(event_t) * ev.size());
  for (int i = 0; i < n_events; ++i) ev[(size_t)i].mean = means[i];
  scalings_t sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.scale = scale, sc.shift = shift, sc.var = var, sc.log_var = log_var;
  std::vector<char> s(seq, seq + seq_len);
  s.push_back(0);
  return profile_hmm_score(s.data(), s.data(), ev.data(), sc, g_model.data(), (uint32_t)start, (uint32_t)stop, 0,
                           (int8_t)(rc ? -1 : 1), (uint8_t)rc, events_per_base, (uint32_t)flags);
}
"""


class LiveHmm:
    """hmm.c compiled in a temporary directory, called through the shim."""

    def __init__(self, ref_root):
        src = os.path.join(ref_root, "benchmarks", "abea", "src")
        hts = os.path.join(ref_root, "tools", "htslib")
        if not os.path.exists(os.path.join(src, "hmm.c")):
            raise FileNotFoundError(src)
        self.dir = tempfile.mkdtemp(prefix="gb_abea_hmm_")
        with open(os.path.join(self.dir, "hdf5.h"), "w") as fh:
            fh.write(HDF5_STANDIN)
        with open(os.path.join(self.dir, "shim.cpp"), "w") as fh:
            fh.write(SHIM)
        flags = ["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-fPIC", "-w", "-I" + self.dir, "-I" + hts, "-I" + src]
        objs = []
        for name, path in (("hmm", os.path.join(src, "hmm.c")), ("shim", os.path.join(self.dir, "shim.cpp"))):
            o = os.path.join(self.dir, name + ".o")
            subprocess.check_call(flags + ["-x", "c++", "-c", path, "-o", o])
            objs.append(o)
        so = os.path.join(self.dir, "libabea_hmm_live.so")
        subprocess.check_call(["g++", "-shared", "-o", so] + objs + ["-lm"])
        self.lib = ctypes.CDLL(so)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        self.lib.hmm_live_init.argtypes = [vp]
        self.lib.hmm_live_model.argtypes = [vp, ci]
        self.lib.hmm_live_score.argtypes = [vp, ci, vp, ci, cf, cf, cf, cf, ci, ci, ci, ctypes.c_double, ci]
        self.lib.hmm_live_score.restype = cf
        self.table = np.zeros(ref.TBL, np.float32)
        self.lib.hmm_live_init(self.table.ctypes.data)
        self.model = None

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def scores(self, x, idx=None):
        """profile_hmm_score of the items idx (all by default) of a gen.AbeaHmmItems, float32."""
        if self.model is not x.model:
            self.model = x.model
            self.lib.hmm_live_model(x.model.ctypes.data, len(x.model))
        idx = range(x.n) if idx is None else idx
        out = np.zeros(len(idx), np.float32)
        fd = os.dup(2)  # the reference warns on stderr about every byte other than ACGMT
        with open(os.devnull, "w") as dn:
            os.dup2(dn.fileno(), 2)
            try:
                for k, i in enumerate(idx):
                    seq, ev, rd, it = x.item(i)
                    seq, ev = np.ascontiguousarray(seq), np.ascontiguousarray(ev)
                    out[k] = self.lib.hmm_live_score(seq.ctypes.data, len(seq), ev.ctypes.data, len(ev), float(rd["scale"]),
                                                     float(rd["shift"]), float(rd["var"]), float(rd["log_var"]),
                                                     int(it["event_start"]), int(it["event_stop"]), int(it["rc"]),
                                                     float(rd["events_per_base"]), int(it["flags"]))
            finally:
                os.dup2(fd, 2)
                os.close(fd)
        return out


def quantized_model(rng, grid=None):
    m = gen.abea_cpg_model(rng, grid)
    m[:, 0] = np.round(m[:, 0] * 64) / 64
    m[:, 1] = np.round(m[:, 1] * 128) / 128
    m[:, 2] = np.log(m[:, 1].astype(np.float64)).astype(np.float32)
    return m


def build_items(rng):
    """(models, [(group, model id, gen.AbeaHmmItems)])."""
    models = [quantized_model(rng), quantized_model(rng, grid=4.0)]
    parts = []

    def add(group, mid, shapes, **kw):
        kw.setdefault("quantum", QUANTUM)
        parts.append((group, mid, gen.abea_hmm_items(rng, shapes, model=models[mid], **kw)))

    # every size at which the kernel takes another path, crossed with the row counts, both strands and all flags;
    # the four flag values share a read
    for nk in KMERS:
        for rows in ROWS:
            for rc in (0, 1):
                x = gen.abea_hmm_items(rng, [(1, nk, rows)], model=models[0], rc=rc, flags=0, meth="none", quantum=QUANTUM,
                                       epb=float(np.clip(rows / nk, 1.05, 4.0)))
                it = np.repeat(x.items, 4)
                it["flags"] = np.arange(4)
                parts.append(("shape", 0, gen.AbeaHmmItems(x.model, x.seqs, x.events, x.reads, it)))
    typical = [(1, nk, int(nk * rng.uniform(1.2, 2.5))) for nk in rng.integers(16, 41, 40)]
    add("typical", 0, typical)
    add("meth", 0, [(1, nk, 2 * nk) for nk in (3, 11, 20, 33, 70, 140)], meth="only", cpg=0.3)
    add("nonacgmt", 0, [(1, nk, 2 * nk) for nk in (5, 14, 30, 90)], non_acgmt=0.08)
    add("epb_one", 0, [(1, nk, rows) for nk, rows in ((4, 9), (16, 16), (30, 45), (100, 130))], epb=1.0)
    add("outlier", 0, [(1, nk, 2 * nk) for nk in (8, 24, 40, 80)], outliers=3)
    add("grid", 1, [(1, nk, rows) for nk, rows in ((6, 6), (12, 30), (16, 40), (30, 50), (40, 60), (70, 100))],
        quantum=2.0, scale=1.0, shift=0.0, var=1.0, noise=1.0, epb=2.0)
    add("scaled", 0, [(1, nk, 2 * nk) for nk in (10, 25, 60)], scale=(0.8, 0.9), shift=(8.0, 12.0), var=(1.6, 2.4))
    add("scaled", 0, [(1, nk, 2 * nk) for nk in (10, 25, 60)], scale=(1.15, 1.25), shift=(-12.0, -8.0), var=(0.45, 0.7))
    return models, parts


MINIMA = {"cut_distance": 1000, "cut_neg_inf": 1000, "index_0": 20, "index_15000": 20, "mm_self_neg_inf": 4, "m_kmer": 20,
          "rank0_byte": 4, "one_row": 50, "more_kmers_than_rows": 200, "stride_up": 200, "stride_down": 200}


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REF_TREE
    live = LiveHmm(ref_root)
    assert (live.table.view(np.uint32) == ref.logsum_table().view(np.uint32)).all(), "the restated table differs"
    rng = np.random.default_rng(20261021)
    models, parts = build_items(rng)
    labels = dict.fromkeys(ref.LABELS, 0)
    scores = []
    for group, mid, x in parts:
        want = live.scores(x)
        for i in range(x.n):
            got = ref.score_item(x, i, labels)
            assert got.view(np.uint32) == want[i].view(np.uint32), (group, i, x.items[i], got, want[i])
        assert np.isfinite(want).all(), (group, x.items[~np.isfinite(want)])
        scores.append(want)
        print(f"{group:9s} {x.n:3d} items, k-mers {x.n_kmers[0]:3d} rows {x.n_rows[0]:4d} score {want[0]:.4f}", flush=True)
    live.close()
    for k, v in MINIMA.items():
        print(f"label {k:22s} {labels[k]:9d} (min {v})")
    short = [k for k, v in MINIMA.items() if labels[k] < v]
    assert not short, f"labels below their minimum: {short}"
    allx = gen.AbeaHmmItems.concat([x for _, _, x in parts])
    ev_q = allx.events / QUANTUM
    assert (ev_q == np.round(ev_q)).all() and np.abs(ev_q).max() < 32768
    mq = np.stack(models)
    assert (mq[..., 0] * 64 == np.round(mq[..., 0] * 64)).all() and (mq[..., 1] * 128 == np.round(mq[..., 1] * 128)).all()
    out = os.path.join(HERE, "abea_hmm_golden.npz")
    np.savez_compressed(
        out, model_mean_q=(mq[..., 0] * 64).astype(np.uint16), model_stdv_q=(mq[..., 1] * 128).astype(np.uint16),
        model_log_stdv=mq[..., 2], seqs=allx.seqs, events_q=ev_q.astype(np.int16), reads=allx.reads, items=allx.items,
        group=np.concatenate([[g] * x.n for g, _, x in parts]),
        model_id=np.concatenate([[m] * x.n for _, m, x in parts]).astype(np.int8),
        score_bits=np.concatenate(scores).view(np.uint32), table_bits=ref.logsum_table().view(np.uint32),
        label_names=np.array(list(labels)), label_counts=np.array(list(labels.values()), np.int64),
        label_minima=np.array([MINIMA[k] for k in labels], np.int64))
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {allx.n} items, {len(allx.reads)} reads")
    assert os.path.getsize(out) <= 400 * 1024


if __name__ == "__main__":
    main()
