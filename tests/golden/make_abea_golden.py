"""Records tests/golden/abea_golden.npz: reads for gb_abea_align with what f5c's CPU align() returns for them.

The live reference is benchmarks/abea/src/align.c, compiled unmodified in a temporary directory outside the
tree (g++ -O2 -std=c++11 -ffp-contract=off -DNDEBUG, tools/htslib reached by -I), next to a stand-in hdf5.h
written here that only declares the names fast5lite.h's inline helpers use (align.c calls none of them) and a
small C++ shim written here that calls align() (C++ linkage) on plain arrays. -DNDEBUG only removes align()'s
assert that a walk is shorter than 2 * n_events, which reads with fewer events than k-mers do not meet. The
output buffer is prefilled with a sentinel, so the pre-QC pair count can be read back after a QC failure.

tests/abea_ref.py restates the contract in numpy. For every read sent to the live reference it must equal the
live result in every pair and in the count; it supplies what the reference does not return (max_gap, spanned,
sum_emission, fills, end cell, end score) and would find the no_end_cell reads, which are never sent to the
live reference (undefined behaviour there); no read of this fixture is one, see DESIGN.md. It also counts labels, each with a minimum asserted here and again by
tests/test_abea.py on the stored counts.

Per read the fixture stores the walk as its end cell plus one move byte per step, not as pairs. Event means
are multiples of 1/8 and stored as int16.

Usage: python tests/golden/make_abea_golden.py [reference root]
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

import abea_ref  # noqa: E402
from genomicsbench_palisade_amd import gen  # noqa: E402

REF_TREE = "/root/reference"
QUANTUM = 0.125
SENTINEL = -7

HDF5_STANDIN = """\
/* stand-in for hdf5.h: declarations only, for the inline helpers of fast5lite.h that align.c never calls */
#pragma once
#include <sys/types.h>
typedef long hid_t;
typedef int herr_t;
typedef unsigned long long hsize_t;
enum { H5F_ACC_RDONLY = 0, H5P_DEFAULT = 0, H5T_NATIVE_FLOAT = 0, H5_INDEX_NAME = 0, H5_ITER_INC = 0, H5S_ALL = 0 };
hid_t H5Fopen(...); herr_t H5Fclose(...); hid_t H5Aopen(...); herr_t H5Aread(...); herr_t H5Aclose(...);
ssize_t H5Lget_name_by_idx(...); hid_t H5Dopen(...); hid_t H5Dget_space(...); herr_t H5Dclose(...);
int H5Sget_simple_extent_dims(...); herr_t H5Sclose(...); herr_t H5Dread(...); hid_t H5Gopen(...);
herr_t H5Gclose(...); int H5Lexists(...); int H5Aexists(...); hid_t H5Aget_type(...); int H5Tis_variable_str(...);
hsize_t H5Aget_storage_size(...); herr_t H5Tclose(...);
"""

SHIM = """\
#include "f5c.h"
#include <cstring>
#include <vector>
int32_t align(AlignedPair *, char *, int32_t, event_table, model_t *, scalings_t, float);  // align.c:169
extern "C" int abea_live_align(int *out, const char *seq, int seq_len, const float *means, int n_events,
                               const float *model, float scale, float shift) {
  std::vector<event_t> ev((size_t)n_events);
  std::memset(ev.data(), 0, sizeof(event_t) * ev.size());
  for (int i = 0; i < n_events; ++i) ev[(size_t)i].mean = means[i];
  event_table et;
  et.n = (size_t)n_events, et.start = 0, et.end = (size_t)n_events, et.event = ev.data();
  std::vector<model_t> m(4096);
  for (int k = 0; k < 4096; ++k)
    m[(size_t)k].level_mean = model[3 * k], m[(size_t)k].level_stdv = model[3 * k + 1],
    m[(size_t)k].level_log_stdv = model[3 * k + 2];
  scalings_t sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.scale = scale, sc.shift = shift, sc.var = 1.0f;
  std::vector<char> s(seq, seq + seq_len);
  s.push_back(0);
  return align((AlignedPair *)out, s.data(), seq_len, et, m.data(), sc, 4000.0f);
}
"""


class LiveAbea:
    """align.c compiled in a temporary directory, called through the shim."""

    def __init__(self, ref_root):
        src = os.path.join(ref_root, "benchmarks", "abea", "src")
        hts = os.path.join(ref_root, "tools", "htslib")
        if not os.path.exists(os.path.join(src, "align.c")):
            raise FileNotFoundError(src)
        self.dir = tempfile.mkdtemp(prefix="gb_abea_")
        with open(os.path.join(self.dir, "hdf5.h"), "w") as fh:
            fh.write(HDF5_STANDIN)
        with open(os.path.join(self.dir, "shim.cpp"), "w") as fh:
            fh.write(SHIM)
        flags = ["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-DNDEBUG", "-fPIC", "-w", "-I" + self.dir, "-I" + hts,
                 "-I" + src]
        objs = []
        for name, path in (("align", os.path.join(src, "align.c")), ("shim", os.path.join(self.dir, "shim.cpp"))):
            o = os.path.join(self.dir, name + ".o")
            subprocess.check_call(flags + ["-x", "c++", "-c", path, "-o", o])
            objs.append(o)
        so = os.path.join(self.dir, "libabea_live.so")
        subprocess.check_call(["g++", "-shared", "-o", so] + objs + ["-lm"])
        self.lib = ctypes.CDLL(so)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        self.lib.abea_live_align.argtypes = [vp, vp, ci, vp, ci, vp, cf, cf]

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def align(self, model, bases, events, scale, shift):
        """(align()'s return value, the pairs it left in the buffer before the QC)."""
        bases = np.ascontiguousarray(bases, np.uint8)
        events = np.ascontiguousarray(events, np.float32)
        model = np.ascontiguousarray(model, np.float32)
        cap = len(events) + len(bases) + 8
        out = np.full((cap, 2), SENTINEL, np.int32)
        fd = os.dup(2)  # the reference warns on stderr about every base other than ACGT
        with open(os.devnull, "w") as dn:
            os.dup2(dn.fileno(), 2)
            try:
                n = self.lib.abea_live_align(out.ctypes.data, bases.ctypes.data, len(bases), events.ctypes.data,
                                             len(events), model.ctypes.data, float(scale), float(shift))
            finally:
                os.dup2(fd, 2)
                os.close(fd)
        n_raw = int(np.count_nonzero(out[:, 0] != SENTINEL))
        assert (out[n_raw:] == SENTINEL).all()
        return n, out[:n_raw].copy()


def build_reads(rng):
    """[(group, model id, bases, events, scale, shift)] over two models: 0 random, 1 on a coarse grid."""
    models = [gen.abea_model(rng), gen.abea_model(rng, grid=4.0)]
    R = []

    def add(group, mid, **kw):
        scale, shift = kw.get("scale", 1.0), kw.get("shift", 0.0)
        q = kw.pop("quantum", QUANTUM)
        b, e = gen.abea_read(rng, models[mid], quantum=q, **kw)
        R.append((group, mid, b, e, np.float32(scale), np.float32(shift)))

    for seq_len in range(6, 13):       # tiny: seq_len 6..12 crossed with n_events 1..8, events spread over the k-mers
        for n_events in range(1, 9):
            b = gen.BASES[rng.integers(0, 4, seq_len)].copy()
            ranks = abea_ref.kmer_ranks(b)
            k = np.arange(n_events) * len(ranks) // n_events
            e = models[0][ranks[k], 0] + 0.3 * models[0][ranks[k], 1] * rng.standard_normal(n_events)
            R.append(("tiny", 0, b, (np.round(e / QUANTUM) * QUANTUM).astype(np.float32), np.float32(1), np.float32(0)))
    for seq_len in np.linspace(20, 120, 30).astype(int):
        add("short", 0, seq_len=int(seq_len), noise=0.6)
    for seq_len in (150, 400, 900):
        add("ratio", 0, seq_len=seq_len, events_per_kmer=0.4, noise=0.5)
    for seq_len, epk in ((60, 5.0), (150, 7.0), (300, 10.0)):
        add("ratio", 0, seq_len=seq_len, events_per_kmer=epk, noise=0.5)
    for i in range(20):
        add("typical", 0, seq_len=int(rng.integers(200, 2001)), noise=float(rng.uniform(0.5, 1.0)),
            missing=float(rng.uniform(0.0, 0.02)))
    for seq_len in (8000, 9100, 10000):
        add("long", 0, seq_len=seq_len, noise=0.6, missing=0.005)
    for scale, shift in ((1.08, -6.5), (0.93, 11.25), (1.2, 3.0)):
        add("scaled", 0, seq_len=int(rng.integers(150, 500)), noise=0.6, scale=scale, shift=shift)
    for seq_len in (40, 120, 300, 500):
        add("ties", 1, seq_len=seq_len, noise=1.0, quantum=2.0)
    for seq_len in (60, 250):
        add("nonacgt", 0, seq_len=seq_len, noise=0.6, non_acgt=0.05)
    for seq_len in (200, 500):
        add("qc_emission", 0, seq_len=seq_len, noise=4.0)
    for seq_len in (200, 400):
        add("qc_span", 0, seq_len=seq_len, noise=0.3, skip_lead=130)
    # a run of more than 50 k-mers without events. Over random bases every skipped k-mer adds a mismatched
    # emission to the walk's sum, so the emission test fails with the gap test; in a homopolymer the skipped
    # k-mers share the level of the event they are skipped at, and the gap test fails alone
    add("qc_gap", 0, seq_len=300, events_per_kmer=1.0, noise=0.2, skip_run=120)
    add("qc_gap", 0, seq_len=400, noise=0.5, poly_a=60)
    add("qc_gap", 0, seq_len=600, noise=0.5, poly_a=80)
    # far more k-mers than events: the nearest a read comes to having no end cell (none has one)
    for seq_len, n_events in ((120, 1), (200, 3), (400, 20), (300, 2)):
        b, e = gen.abea_read(rng, models[0], seq_len, events_per_kmer=1.0, noise=0.5, quantum=QUANTUM)
        R.append(("few_events", 0, b, e[:n_events], np.float32(1), np.float32(0)))
    return models, R


MINIMA = {"tie_u": 1, "tie_l": 1, "alternate": 50, "move_right": 1000, "move_down": 1000, "clamp_kmer_min": 50,
          "clamp_event_min": 50, "clamp_kmer_max": 50, "clamp_event_max": 50, "trim_cell": 50, "trim_past_events": 1,
          "qc_emission_only": 1, "qc_gap_only": 1, "walk_ends_kmer": 1, "walk_ends_event": 1}


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REF_TREE
    live = LiveAbea(ref_root)
    rng = np.random.default_rng(20261020)
    models, R = build_reads(rng)
    labels = dict.fromkeys(abea_ref.LABELS, 0)
    stats = {k: [] for k in ("n_pairs", "n_raw", "max_gap", "spanned", "end_event", "no_end_cell", "fills")}
    end_bits, sum_bits, moves, live_checked = [], [], [], []
    for i, (group, mid, b, e, scale, shift) in enumerate(R):
        r = abea_ref.align(models[mid], b, e, scale, shift)
        if r["no_end_cell"]:
            live_checked.append(0)  # undefined behaviour in the reference: never sent there
        else:
            n, raw = live.align(models[mid], b, e, scale, shift)
            assert n == r["n_pairs"], (i, group, n, r["n_pairs"])
            assert raw.shape == r["pairs"].shape and (raw == r["pairs"]).all(), (i, group, "pairs differ")
            live_checked.append(1)
        if r["n_raw"]:
            nk = len(b) - abea_ref.K + 1
            assert (abea_ref.pairs_from_moves(nk, r["end_event"], r["moves"]) == r["pairs"]).all()
        for k in stats:
            stats[k].append(r[k])
        end_bits.append(np.float32(r["end_score"]).view(np.uint32))
        sum_bits.append(np.float64(r["sum_emission"]).view(np.uint64))
        moves.append(r["moves"])
        for k, v in r["labels"].items():
            labels[k] += v
        print(f"{i:3d} {group:12s} len {len(b):5d} events {len(e):5d} raw {r['n_raw']:5d} pairs {r['n_pairs']:5d} "
              f"gap {r['max_gap']:3d} no_end {r['no_end_cell']}", flush=True)
    live.close()
    groups = [g for g, *_ in R]
    for k, v in MINIMA.items():
        print(f"label {k:18s} {labels[k]:8d} (min {v})")
    short = [k for k, v in MINIMA.items() if labels[k] < v]
    assert not short, f"labels below their minimum: {short}"
    plain = [i for i, g in enumerate(groups) if not g.startswith("qc_") and g != "no_end_cell"]
    failed = [i for i in plain if stats["n_pairs"][i] == 0]
    print(f"QC failures outside the qc_* and no_end_cell groups: {len(failed)} of {len(plain)}")
    assert 4 * len(failed) <= len(plain)
    for g in ("qc_emission", "qc_span", "qc_gap"):
        assert all(stats["n_pairs"][i] == 0 and stats["n_raw"][i] > 0 for i, x in enumerate(groups) if x == g), g
    ev_q = np.concatenate([e for _, _, _, e, _, _ in R]) / QUANTUM
    assert (ev_q == np.round(ev_q)).all() and np.abs(ev_q).max() < 32768
    out = os.path.join(HERE, "abea_golden.npz")
    np.savez_compressed(
        out, models=np.stack(models), group=np.array(groups), model_id=np.array([m for _, m, *_ in R], np.int8),
        seqs=np.concatenate([b for _, _, b, *_ in R]), events_q=ev_q.astype(np.int16),
        seq_len=np.array([len(b) for _, _, b, *_ in R], np.int32), n_events=np.array([len(e) for *_, e, _, _ in R], np.int32),
        scale=np.array([s for *_, s, _ in R], np.float32), shift=np.array([s for *_, s in R], np.float32),
        end_score_bits=np.array(end_bits, np.uint32), sum_emission_bits=np.array(sum_bits, np.uint64),
        moves=np.concatenate(moves), live_checked=np.array(live_checked, np.int8),
        label_names=np.array(list(labels)), label_counts=np.array(list(labels.values()), np.int64),
        label_minima=np.array([MINIMA[k] for k in labels], np.int64),
        **{k: np.array(v, np.int32) for k, v in stats.items()})
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(R)} reads")
    assert os.path.getsize(out) <= 600 * 1024


if __name__ == "__main__":
    main()
