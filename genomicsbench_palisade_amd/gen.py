"""Seeded synthetic inputs shaped like the reference's 'small'/'large' datasets.

The real input-datasets tarball (README.md:26 of the reference) is not available, so every benchmark
and parity test runs on these generators. Shapes follow the comments/logs recovered in SURVEY.md:
  phmm  small: batches <=110 reads x <=37 haps, reads <=250 bp, haps <=302 bp
        large: batches <=1193 reads x <=128 haps, reads <=250 bp, haps <=473 bp
        (PairHMMUnitTest.cpp:1,9-10,30; <=50000 testcases per batch, :69,558)
"""
from __future__ import annotations

import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


class PhmmBatch:
    """One read_batch() worth of data (PairHMMUnitTest.cpp:118-210,461-474): R reads x H haps.

    reads[r] = (bases, q, i, d, c) as bytes, already normalized (phred-33, q>=6) like normalize()
    (PairHMMUnitTest.cpp:107-113); haps[h] = bases. Testcases are r-major: tc[r*H+h].
    """

    def __init__(self, reads, haps):
        self.reads = reads
        self.haps = haps

    @property
    def num_testcases(self):
        return len(self.reads) * len(self.haps)

    def cells(self):
        return sum(len(r[0]) for r in self.reads) * sum(len(h) for h in self.haps)


def _mutate(rng, seq: np.ndarray, sub_rate: float, n_rate: float) -> np.ndarray:
    out = seq.copy()
    m = rng.random(len(out)) < sub_rate
    out[m] = BASES[rng.integers(0, 4, m.sum())]
    nm = rng.random(len(out)) < n_rate
    out[nm] = ord("N")
    return out


def phmm_batch(rng, num_reads, num_haps, read_len=(100, 250), hap_max=473, sub_rate=0.10,
               n_rate=0.01, q_range=(6, 40)):
    """Reads ~ U[read_len], haps ~ U[rl, hap_max] built around a common source; reads are sampled
    from the first haplotype with sub_rate substitutions and n_rate N's."""
    hap_lens = []
    rl_lo, rl_hi = read_len
    max_rl = rl_hi
    src = BASES[rng.integers(0, 4, hap_max + 64)]
    haps = []
    for _ in range(num_haps):
        hl = int(rng.integers(min(max_rl, hap_max), hap_max + 1)) if hap_max > max_rl else hap_max
        off = int(rng.integers(0, 32))
        h = _mutate(rng, src[off:off + hl], 0.02, 0.002)
        haps.append(h.tobytes())
        hap_lens.append(hl)
    reads = []
    for _ in range(num_reads):
        rl = int(rng.integers(rl_lo, rl_hi + 1))
        hl = len(haps[0])
        st = int(rng.integers(0, max(1, hl - rl + 1)))
        b = _mutate(rng, np.frombuffer(haps[0], dtype=np.uint8)[st:st + rl], sub_rate, n_rate)
        if len(b) < rl:
            b = np.concatenate([b, BASES[rng.integers(0, 4, rl - len(b))]])
        q = rng.integers(q_range[0], q_range[1] + 1, rl).astype(np.uint8)
        i = rng.integers(40, 46, rl).astype(np.uint8)
        d = rng.integers(40, 46, rl).astype(np.uint8)
        c = np.full(rl, 10, dtype=np.uint8)
        reads.append((b.tobytes(), q.tobytes(), i.tobytes(), d.tobytes(), c.tobytes()))
    return PhmmBatch(reads, haps)


def phmm_dataset(kind: str, num_batches: int, seed: int = 1):
    """'small' / 'large' shaped batches (seed 1 by default)."""
    rng = np.random.default_rng(seed)
    if kind == "large":
        max_r, max_h, hap_max = 1193, 128, 473
    elif kind == "small":
        max_r, max_h, hap_max = 110, 37, 302
    else:
        raise ValueError(kind)
    out = []
    for _ in range(num_batches):
        # skewed batch sizes: most batches small, a few near the maximum
        R = max(1, int(max_r * rng.random() ** 2))
        H = max(1, int(max_h * rng.random() ** 1.5))
        while R * H > 50000:  # MAX_BATCH_SIZE, PairHMMUnitTest.cpp:69,558
            R = max(1, R // 2)
        out.append(phmm_batch(rng, R, H, hap_max=hap_max))
    return out


def write_phmm_file(path, batches):
    """Write the reference's .in text format (read_batch, PairHMMUnitTest.cpp:137,157,464):
    'R H' then R lines 'bases q i d c' (quals stored +33 raw) then H lines 'bases'."""
    with open(path, "w") as f:
        for b in batches:
            f.write(f"{len(b.reads)} {len(b.haps)}\n")
            for bases, q, i, d, c in b.reads:
                enc = lambda s: bytes(x + 33 for x in s).decode("latin-1")
                f.write(f"{bases.decode()} {enc(q)} {enc(i)} {enc(d)} {enc(c)}\n")
            for h in b.haps:
                f.write(h.decode() + "\n")


# ---------------------------------------------------------------------------------------------
# fmi: synthetic reference + reads ('large' = 10 M x 151 bp reads over a 512 Mbp
# reference (+RC); 1% substitutions, 0.1% indels, 0.05% N; seed 7)
# ---------------------------------------------------------------------------------------------
def fmi_reference(length: int, seed: int = 7, repeat_frac: float = 0.08):
    """Random A/C/G/T codes (0..3) with genome-like structure: ~repeat_frac of the sequence is
    overwritten by mutated copies of earlier segments (interspersed repeats) and short tandem
    repeats, so the SMEM search sees multi-copy intervals and reseeding, not only unique hits."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, length, dtype=np.uint8)
    budget = int(length * repeat_frac)
    while budget > 0 and length > 1000:
        if rng.random() < 0.85:  # interspersed copy, 1-15% divergence
            L = int(min(length // 4, max(50, rng.geometric(1 / 800))))
            src = int(rng.integers(0, length - L))
            dst = int(rng.integers(0, length - L))
            seg = ref[src:src + L].copy()
            mut = rng.random(L) < rng.uniform(0.0, 0.15)
            seg[mut] = rng.integers(0, 4, int(mut.sum()), dtype=np.uint8)
            if rng.random() < 0.5:
                seg = (3 - seg[::-1]).astype(np.uint8)
        else:  # tandem repeat of a short unit
            unit = rng.integers(0, 4, int(rng.integers(1, 7)), dtype=np.uint8)
            L = int(rng.integers(20, 300))
            seg = np.resize(unit, L)
            dst = int(rng.integers(0, length - L))
        ref[dst:dst + len(seg)] = seg
        budget -= len(seg)
    return ref


def fmi_reads(ref: np.ndarray, num_reads: int, read_len: int = 151, seed: int = 7, sub_rate=0.01,
              indel_rate=0.001, n_rate=0.0005, chunk: int = 250_000):
    """Reads sampled uniformly from both strands; returns (codes[num_reads, read_len] uint8 with
    4 = N, lens int32). Codes follow fmi.cpp:141-177 (A0 C1 G2 T3, anything else 4). Generated in
    chunks so 10 M-read sets stay within a few GB of host memory."""
    rng = np.random.default_rng(seed)
    G = len(ref)
    out = np.empty((num_reads, read_len), np.uint8)
    span = read_len + 8
    for c0 in range(0, num_reads, chunk):
        nr = min(chunk, num_reads - c0)
        starts = rng.integers(0, G - span, nr)
        strand = rng.random(nr) < 0.5
        frag = ref[starts[:, None] + np.arange(span)[None, :]]
        # indels: at most one per read, applied on the fragment before trimming (vectorized)
        R = np.nonzero(rng.random(nr) < indel_rate * read_len)[0]
        if len(R):
            p = rng.integers(1, read_len - 1, len(R))[:, None]
            dele = (rng.random(len(R)) < 0.5)[:, None]
            col = np.arange(span)[None, :]
            src = np.where(dele, np.minimum(col + (col >= p), span - 1), col - (col > p))
            sub_frag = np.take_along_axis(frag[R], src, axis=1)
            ins_rows = np.nonzero(~dele[:, 0])[0]
            sub_frag[ins_rows, p[ins_rows, 0]] = rng.integers(0, 4, len(ins_rows))
            frag[R] = sub_frag
        frag = np.ascontiguousarray(frag[:, :read_len])
        frag[strand] = (3 - frag[strand, ::-1])
        flat = frag.reshape(-1)
        si = rng.integers(0, flat.size, rng.binomial(flat.size, sub_rate))
        flat[si] = (flat[si] + rng.integers(1, 4, len(si))) % 4
        flat[rng.integers(0, flat.size, rng.binomial(flat.size, n_rate))] = 4
        out[c0:c0 + nr] = frag
    return out, np.full(num_reads, read_len, np.int32)


def write_fasta(path, ref: np.ndarray, name="chr1", width=80):
    s = np.frombuffer(b"ACGT", np.uint8)[ref].tobytes()
    with open(path, "wb") as f:
        f.write(b">" + name.encode() + b"\n")
        for i in range(0, len(s), width):
            f.write(s[i:i + width] + b"\n")


def write_fastq(path, codes: np.ndarray, lens: np.ndarray):
    lut = np.frombuffer(b"ACGTN", np.uint8)
    with open(path, "wb") as f:
        for r in range(len(lens)):
            s = lut[codes[r, :lens[r]]].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (r, s, b"I" * len(s)))


def read_pac(path):
    """pac2nt (FMI_search.cpp:93-169): forward-strand codes from a bwa .pac file."""
    raw = np.fromfile(path, np.uint8)
    seq_len = (len(raw) - 2) * 4 + int(raw[-1])  # pac_seq_len: (ftell(-1) - 1) * 4 + last byte
    b = raw[: (seq_len + 3) // 4]
    codes = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)
    return codes[:seq_len].astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# chain: minimap2-style anchor sets (n ~ lognormal, max 87 271 anchors per call,
# anchors sorted by x, ~85% forward strand, spans {15,19,28}, max_dist 5000, bw 500, n_segs 1;
# 'large' = 10 000 calls, 'small' = 1 000; seed 5)
# ---------------------------------------------------------------------------------------------
class ChainCalls:
    """CSR anchor sets: anchors of call c are x[offsets[c]:offsets[c+1]] (call_t, host_data.h:19-39)."""

    def __init__(self, offsets, x, y, avg_qspan, params4):
        self.offsets = np.asarray(offsets, np.int64)
        self.x = np.asarray(x, np.uint64)
        self.y = np.asarray(y, np.uint64)
        self.avg_qspan = np.asarray(avg_qspan, np.float32)
        self.params4 = np.asarray(params4, np.int32).reshape(-1, 4)  # max_dist_x, max_dist_y, bw, n_segs

    @property
    def ncalls(self):
        return len(self.offsets) - 1

    @property
    def nanchors(self):
        return int(self.offsets[-1])

    def slice(self, lo: int, hi: int) -> "ChainCalls":
        """Calls lo..hi-1 as their own CSR set (anchors copied, offsets rebased)."""
        o0, o1 = int(self.offsets[lo]), int(self.offsets[hi])
        return ChainCalls(self.offsets[lo:hi + 1] - o0, self.x[o0:o1].copy(), self.y[o0:o1].copy(),
                          self.avg_qspan[lo:hi].copy(), self.params4[lo:hi].copy())


def chain_call(rng, n: int):
    """One read's anchors: a collinear true locus (~85% of anchors, with small indel drift) plus
    spurious hits at other loci (repeats), mixed strands, sorted by x like minimap2's dumps."""
    n_true = max(1, int(n * rng.uniform(0.75, 0.95)))
    n_sp = n - n_true
    spans = rng.choice(np.array([15, 19, 28]), size=n)
    Lq = int(n_true * rng.uniform(6, 14)) + 100
    rid0, rev0 = int(rng.integers(0, 24)), int(rng.random() < 0.15)
    r0 = int(rng.integers(1_000_000, 200_000_000))
    qpos = np.sort(rng.integers(0, Lq, n_true))
    drift = np.cumsum(rng.choice(np.array([-2, -1, 0, 0, 0, 0, 1, 2]), size=n_true) *
                      (rng.random(n_true) < 0.1))
    rpos = r0 + qpos + drift
    xs = [(rev0 << 63) | (rid0 << 32) | rpos.astype(np.uint64)]
    ys = [qpos]
    if n_sp:
        nl = max(1, n_sp // int(rng.integers(5, 60)))
        loc = rng.integers(0, nl, n_sp)
        lrid = rng.integers(0, 24, nl)
        lrev = (rng.random(nl) < 0.3).astype(np.uint64)
        lr0 = rng.integers(1_000_000, 200_000_000, nl)
        q = rng.integers(0, Lq, n_sp)
        rp = lr0[loc] + q + rng.integers(-50, 50, n_sp)
        xs.append((lrev[loc] << np.uint64(63)) | (lrid[loc].astype(np.uint64) << np.uint64(32)) | rp.astype(np.uint64))
        ys.append(q)
    x = np.concatenate([np.asarray(a, np.uint64) for a in xs])
    q = np.concatenate(ys).astype(np.uint64)
    y = (spans.astype(np.uint64) << np.uint64(32)) | q  # seg id 0
    order = np.lexsort((y, x))
    return x[order], y[order], float(spans.mean())


def chain_dataset(kind: str = "large", num_calls: int | None = None, seed: int = 5,
                  median_n: int = 1500, max_n: int = 87271):
    rng = np.random.default_rng(seed)
    if num_calls is None:
        num_calls = 10_000 if kind == "large" else 1_000
    ns = np.minimum(max_n, np.maximum(2, rng.lognormal(np.log(median_n), 1.0, num_calls).astype(np.int64)))
    ns[int(rng.integers(0, num_calls))] = max_n  # the logged maximum (scripts/chain_small_outt:3938)
    offs = np.zeros(num_calls + 1, np.int64)
    xs, ys, aq = [], [], []
    for c in range(num_calls):
        x, y, a = chain_call(rng, int(ns[c]))
        xs.append(x)
        ys.append(y)
        aq.append(a)
        offs[c + 1] = offs[c] + len(x)
    params = np.tile(np.array([5000, 5000, 500, 1], np.int32), (num_calls, 1))
    return ChainCalls(offs, np.concatenate(xs), np.concatenate(ys), np.array(aq, np.float32), params)


def write_chain_file(path, calls: ChainCalls):
    """read_call format (benchmarks/chain/src/host_data_io.cpp:40-80)."""
    with open(path, "w") as f:
        for c in range(calls.ncalls):
            o0, o1 = calls.offsets[c], calls.offsets[c + 1]
            p = calls.params4[c]
            f.write(f"{o1 - o0}\t{calls.avg_qspan[c]:f}\t{p[0]}\t{p[1]}\t{p[2]}\t{p[3]}\n")
            for xx, yy in zip(calls.x[o0:o1].tolist(), calls.y[o0:o1].tolist()):
                f.write(f"{xx}\t{yy}\n")
            f.write("EOR\n")


class BswPairs:
    """Flattened bsw pairs: pair p has target (ref) tgt[toff[p]:toff[p]+tlen[p]] and query
    qry[qoff[p]:qoff[p]+qlen[p]], codes 0..4 (loadPairs subtracts '0', main_banded.cpp:190-195)."""

    def __init__(self, tgt, toff, tlen, qry, qoff, qlen, h0):
        self.tgt, self.toff, self.tlen = tgt, toff, tlen
        self.qry, self.qoff, self.qlen = qry, qoff, qlen
        self.h0 = h0

    @property
    def n(self):
        return len(self.h0)

    def subset(self, idx):
        idx = np.asarray(idx, np.int64)
        tl, ql = self.tlen[idx], self.qlen[idx]
        toff = np.zeros(len(idx), np.int64)
        qoff = np.zeros(len(idx), np.int64)
        toff[1:] = np.cumsum(tl)[:-1]
        qoff[1:] = np.cumsum(ql)[:-1]
        tgt = np.concatenate([self.tgt[self.toff[p]:self.toff[p] + self.tlen[p]] for p in idx.tolist()]) \
            if len(idx) else np.zeros(0, np.uint8)
        qry = np.concatenate([self.qry[self.qoff[p]:self.qoff[p] + self.qlen[p]] for p in idx.tolist()]) \
            if len(idx) else np.zeros(0, np.uint8)
        return BswPairs(tgt, toff, tl.copy(), qry, qoff, ql.copy(), self.h0[idx].copy())

    def slice(self, lo: int, hi: int) -> "BswPairs":
        """Pairs lo..hi-1 (contiguous, so the sequence pools are sliced, not gathered)."""
        if hi <= lo:
            return self.subset(np.zeros(0, np.int64))
        t0, t1 = int(self.toff[lo]), int(self.toff[hi - 1] + self.tlen[hi - 1])
        q0, q1 = int(self.qoff[lo]), int(self.qoff[hi - 1] + self.qlen[hi - 1])
        return BswPairs(self.tgt[t0:t1].copy(), (self.toff[lo:hi] - t0).astype(np.int64), self.tlen[lo:hi].copy(),
                        self.qry[q0:q1].copy(), (self.qoff[lo:hi] - q0).astype(np.int64), self.qlen[lo:hi].copy(),
                        self.h0[lo:hi].copy())


def _ragged_local(lens):
    """(pair index, position within pair) for every element of a ragged concatenation."""
    offs = np.zeros(len(lens), np.int64)
    offs[1:] = np.cumsum(lens)[:-1]
    tot = int(np.sum(lens))
    pid = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    return offs, pid, np.arange(tot, dtype=np.int64) - offs[pid]


def bsw_pairs(num_pairs: int, seed: int = 11, qlen=(10, 150), extra=(0, 100), n_rate=0.002):
    """bwa-mem-like extension pairs: query ~ U[10,150], target = query
    mutated (per-pair substitution rate 0-12 %, one indel of +-1..6 bp in 30 % of pairs, 8 % of
    targets unrelated) followed by U[0,100] extra bases; h0 = 0 for 20 %, else U[10,70]."""
    rng = np.random.default_rng(seed)
    n = int(num_pairs)
    ql = rng.integers(qlen[0], qlen[1] + 1, n).astype(np.int32)
    tl = (ql + rng.integers(extra[0], extra[1] + 1, n)).astype(np.int32)
    h0 = np.where(rng.random(n) < 0.2, 0, rng.integers(10, 71, n)).astype(np.int32)
    qoff, qpid, _ = _ragged_local(ql)
    qry = rng.integers(0, 4, int(ql.sum())).astype(np.uint8)
    qry[rng.random(len(qry)) < n_rate] = 4
    toff, tpid, k = _ragged_local(tl)
    brk = (rng.random(n) * ql).astype(np.int64)
    dlt = rng.integers(1, 7, n) * np.where(rng.random(n) < 0.5, -1, 1)
    dlt[rng.random(n) >= 0.3] = 0
    src = k + np.where(k >= brk[tpid], dlt[tpid], 0)
    ok = (src >= 0) & (src < ql[tpid]) & (rng.random(n) >= 0.08)[tpid]
    tgt = rng.integers(0, 4, len(k)).astype(np.uint8)
    tgt[ok] = qry[qoff[tpid[ok]] + src[ok]]
    sub = rng.random(n) * 0.12
    m = rng.random(len(tgt)) < sub[tpid]
    tgt[m] = rng.integers(0, 4, int(m.sum())).astype(np.uint8)
    tgt[rng.random(len(tgt)) < n_rate] = 4
    return BswPairs(tgt, toff, tl, qry, qoff, ql, h0)


def write_bsw_file(path, pairs: BswPairs):
    """loadPairs format (main_banded.cpp:160-202): per pair 'h0', target, query lines of '0'..'4'."""
    with open(path, "wb") as f:
        for p in range(pairs.n):
            t = (pairs.tgt[pairs.toff[p]:pairs.toff[p] + pairs.tlen[p]] + 48).tobytes()
            q = (pairs.qry[pairs.qoff[p]:pairs.qoff[p] + pairs.qlen[p]] + 48).tobytes()
            f.write(b"%d\n%s\n%s\n" % (int(pairs.h0[p]), t, q))


def concat_bsw(parts):
    """Concatenate BswPairs sets (offsets rebased)."""
    tl = np.concatenate([p.tlen for p in parts])
    ql = np.concatenate([p.qlen for p in parts])
    toff = np.zeros(len(tl), np.int64)
    qoff = np.zeros(len(ql), np.int64)
    toff[1:] = np.cumsum(tl, dtype=np.int64)[:-1]
    qoff[1:] = np.cumsum(ql, dtype=np.int64)[:-1]
    return BswPairs(np.concatenate([p.tgt for p in parts]), toff, tl, np.concatenate([p.qry for p in parts]),
                    qoff, ql, np.concatenate([p.h0 for p in parts]))


BSW_LARGE_PAIRS = 10_606_460  # scripts/bsw_large:6
BSW_SMALL_PAIRS = 100_000     # scripts/bsw_outt:33


def bsw_dataset(num_pairs: int = BSW_LARGE_PAIRS, seed: int = 11, threads: int = 16, chunk: int = 1 << 18):
    """bsw_pairs at dataset scale: chunk c is bsw_pairs(chunk, seed=(seed, c)), generated on a thread
    pool (numpy releases the GIL) and concatenated."""
    from concurrent.futures import ThreadPoolExecutor
    sizes = [min(chunk, num_pairs - o) for o in range(0, num_pairs, chunk)]
    with ThreadPoolExecutor(max(1, threads)) as ex:
        parts = list(ex.map(lambda a: bsw_pairs(a[1], seed=[seed, a[0]]), enumerate(sizes)))
    return concat_bsw(parts) if parts else bsw_pairs(0, seed)


# ---- abea: adaptive banded event alignment (benchmarks/abea) ----

ABEA_K = 6


class AbeaReads:
    """Reads for abea.align: `model` is float32 [4096, 3] (level_mean, level_stdv, level_log_stdv by k-mer
    rank), `seqs` the concatenated ASCII bases (uint8), `events` the concatenated event means (float32); read
    r is seqs[seq_off[r]:][:seq_len[r]] and events[event_off[r]:][:n_events[r]] with scale[r], shift[r]."""

    def __init__(self, model, seqs, events, seq_len, n_events, scale, shift):
        self.model = np.ascontiguousarray(model, np.float32).reshape(4096, 3)
        self.seqs = np.ascontiguousarray(seqs, np.uint8)
        self.events = np.ascontiguousarray(events, np.float32)
        self.seq_len = np.asarray(seq_len, np.int32)
        self.n_events = np.asarray(n_events, np.int32)
        self.scale = np.asarray(scale, np.float32)
        self.shift = np.asarray(shift, np.float32)
        self.seq_off = np.concatenate([[0], np.cumsum(self.seq_len[:-1], dtype=np.int64)]).astype(np.int64)[:len(self.seq_len)]
        self.event_off = np.concatenate([[0], np.cumsum(self.n_events[:-1], dtype=np.int64)]).astype(np.int64)[:len(self.seq_len)]

    @property
    def n(self):
        return len(self.seq_len)

    def pair_cap(self):
        """n_events + n_kmers over the reads: always enough for the pairs."""
        return int(self.n_events.sum(dtype=np.int64) + (self.seq_len.astype(np.int64) - ABEA_K + 1).sum())

    def read(self, r):
        """(bases, event means) of read r."""
        return (self.seqs[self.seq_off[r]:self.seq_off[r] + self.seq_len[r]],
                self.events[self.event_off[r]:self.event_off[r] + self.n_events[r]])

    def subset(self, idx):
        idx = list(idx)
        rs = [self.read(r) for r in idx]
        return AbeaReads(self.model, np.concatenate([s for s, _ in rs]) if rs else np.zeros(0, np.uint8),
                         np.concatenate([e for _, e in rs]) if rs else np.zeros(0, np.float32),
                         self.seq_len[idx], self.n_events[idx], self.scale[idx], self.shift[idx])


def abea_model(rng, grid=None):
    """A pore model shaped like r9.4 (levels 55..130 pA, stdv 1..3.5). With `grid`, levels are multiples of
    it and every stdv is 2, so that equal scores are common."""
    m = np.zeros((4096, 3), np.float32)
    if grid:
        m[:, 0] = (np.round(rng.uniform(55, 130, 4096) / grid) * grid).astype(np.float32)
        m[:, 1] = 2.0
    else:
        m[:, 0] = rng.uniform(55, 130, 4096).astype(np.float32)
        m[:, 1] = rng.uniform(1.0, 3.5, 4096).astype(np.float32)
    m[:, 2] = np.log(m[:, 1].astype(np.float64)).astype(np.float32)
    return m


def abea_kmer_ranks(bases):
    """Rank of every k-mer of an ASCII sequence; a base other than ACGT counts as A (align.c:10-38)."""
    code = np.zeros(256, np.int64)
    code[ord("C")], code[ord("G")], code[ord("T")] = 1, 2, 3
    c = code[np.asarray(bases, np.uint8)]
    n = len(c) - ABEA_K + 1
    r = np.zeros(n, np.int64)
    for i in range(ABEA_K):
        r = r * 4 + c[i:i + n]
    return r


def abea_read(rng, model, seq_len, events_per_kmer=1.6, noise=0.7, missing=0.0, scale=1.0, shift=0.0, non_acgt=0.0,
              skip_lead=0, skip_run=0, poly_a=0, quantum=0.125):
    """One synthetic read: random bases, then for every k-mer a number of events (mean events_per_kmer; none
    with probability `missing` for inner k-mers, none for the first `skip_lead` k-mers and for a run of
    `skip_run` in the middle; with `poly_a` the middle holds that many AAAAAA k-mers in a row and only the first
    has events), each the k-mer's scaled level plus `noise` stdv of Gaussian noise, rounded to
    a multiple of `quantum`. Returns (bases uint8, event means float32)."""
    bases = BASES[rng.integers(0, 4, seq_len)].copy()
    if non_acgt:
        bases[rng.random(seq_len) < non_acgt] = ord("N")
    nk = seq_len - ABEA_K + 1
    if poly_a:
        bases[nk // 2:nk // 2 + poly_a + ABEA_K - 1] = ord("A")
    ranks = abea_kmer_ranks(bases)
    if events_per_kmer >= 1:
        cnt = 1 + rng.poisson(events_per_kmer - 1, nk)
    else:
        cnt = (rng.random(nk) < events_per_kmer).astype(np.int64)
    drop = rng.random(nk) < missing
    drop[:1], drop[-1:] = False, False
    cnt[drop] = 0
    cnt[:skip_lead] = 0
    if skip_run:
        cnt[nk // 2:nk // 2 + skip_run] = 0
    if poly_a:
        cnt[nk // 2 + 1:nk // 2 + poly_a] = 0
    if cnt.sum() == 0:
        cnt[-1] = 1
    k = np.repeat(np.arange(nk), cnt)
    lv = np.float32(scale) * model[ranks[k], 0] + np.float32(shift)
    ev = lv + noise * model[ranks[k], 1] * rng.standard_normal(len(k))
    ev = (np.round(ev / quantum) * quantum).astype(np.float32)
    return bases, ev


def abea_set(rng, n, lo=500, hi=10000, model=None, events_per_kmer=1.6, noise=0.7, missing=0.01):
    """n reads with seq_len log-uniform in lo..hi over one model."""
    model = abea_model(rng) if model is None else model
    lens = np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.int64)
    rs = [abea_read(rng, model, int(l), events_per_kmer, noise, missing) for l in lens]
    return AbeaReads(model, np.concatenate([b for b, _ in rs]), np.concatenate([e for _, e in rs]),
                     [len(b) for b, _ in rs], [len(e) for _, e in rs], np.ones(n, np.float32), np.zeros(n, np.float32))


# ---- abea: methylation profile-HMM scores (benchmarks/abea, profile_hmm_score) ----

ABEA_HMM_MODEL_SIZE = 15625
ABEA_HMM_READ_DTYPE = np.dtype([("event_off", "<i8"), ("n_events", "<i4"), ("scale", "<f4"), ("shift", "<f4"),
                                ("var", "<f4"), ("log_var", "<f4"), ("pad", "<i4"), ("events_per_base", "<f8")])
ABEA_HMM_ITEM_DTYPE = np.dtype([("seq_off", "<i8"), ("seq_len", "<i4"), ("read", "<i4"), ("event_start", "<i4"),
                                ("event_stop", "<i4"), ("rc", "u1"), ("flags", "u1"), ("pad", "u1", (2,)), ("tail", "<i4")])  # tail: the C struct's padding to 8 bytes
assert ABEA_HMM_READ_DTYPE.itemsize == 40 and ABEA_HMM_ITEM_DTYPE.itemsize == 32


class AbeaHmmItems:
    """Items for abea.hmm_score: `model` is float32 [15625, 3] by k-mer rank over ACGMT, `seqs` the concatenated
    ASCII strings, `events` the concatenated event means, `reads` ABEA_HMM_READ_DTYPE records and `items`
    ABEA_HMM_ITEM_DTYPE records (include/gb_bsw_abea_hmm.h)."""

    MODEL_SIZE = ABEA_HMM_MODEL_SIZE

    def __init__(self, model, seqs, events, reads, items):
        self.model = np.ascontiguousarray(model, np.float32).reshape(self.MODEL_SIZE, 3)
        self.seqs = np.ascontiguousarray(seqs, np.uint8)
        self.events = np.ascontiguousarray(events, np.float32)
        self.reads = np.ascontiguousarray(reads, ABEA_HMM_READ_DTYPE)
        self.items = np.ascontiguousarray(items, ABEA_HMM_ITEM_DTYPE)

    @property
    def n(self):
        return len(self.items)

    @property
    def n_kmers(self):
        return self.items["seq_len"].astype(np.int64) - ABEA_K + 1

    @property
    def n_rows(self):
        return np.abs(self.items["event_stop"].astype(np.int64) - self.items["event_start"]) + 1

    def cells(self):
        return int((self.n_kmers * self.n_rows).sum())

    def subset(self, idx):
        """The same buffers and reads with items[idx]."""
        return type(self)(self.model, self.seqs, self.events, self.reads, self.items[np.asarray(idx, np.int64)])

    @classmethod
    def concat(cls, parts, model=None):
        """The items of several sets over one model (the first part's unless given), offsets and read indices
        shifted."""
        reads, items = [], []
        seq_pos = ev_pos = n_reads = 0
        for p in parts:
            rd, it = p.reads.copy(), p.items.copy()
            rd["event_off"] += ev_pos
            it["seq_off"] += seq_pos
            it["read"] += n_reads
            reads.append(rd)
            items.append(it)
            seq_pos, ev_pos, n_reads = seq_pos + len(p.seqs), ev_pos + len(p.events), n_reads + len(p.reads)
        return cls(parts[0].model if model is None else model, np.concatenate([p.seqs for p in parts]),
                   np.concatenate([p.events for p in parts]), np.concatenate(reads), np.concatenate(items))

    def item(self, i):
        """(string, the read's event means, read record, item record) of item i."""
        it = self.items[i]
        rd = self.reads[it["read"]]
        return (self.seqs[it["seq_off"]:it["seq_off"] + it["seq_len"]],
                self.events[rd["event_off"]:rd["event_off"] + rd["n_events"]], rd, it)


def abea_cpg_model(rng, grid=None):
    """A seeded pore model over ACGMT shaped like abea_model (levels 55..130 pA, stdv 1..3.5). With `grid`, levels
    are multiples of it and every stdv is 2."""
    m = np.zeros((ABEA_HMM_MODEL_SIZE, 3), np.float32)
    if grid:
        m[:, 0] = (np.round(rng.uniform(55, 130, len(m)) / grid) * grid).astype(np.float32)
        m[:, 1] = 2.0
    else:
        m[:, 0] = rng.uniform(55, 130, len(m)).astype(np.float32)
        m[:, 1] = rng.uniform(1.0, 3.5, len(m)).astype(np.float32)
    m[:, 2] = np.log(m[:, 1].astype(np.float64)).astype(np.float32)
    return m


def abea_hmm_kmer_ranks(strings, rc):
    """Ranks [..., n_kmers] of the k-mers of ASCII strings [..., len] in the order profile_hmm_score visits
    them: k-mer ki starts at ki for rc == 0 and at len - ki - 6 for rc == 1 (rc is a scalar or one value per
    string); base 5 with A C G M T = 0..4 and any other byte 0 (hmm.c:21-52, 382-393)."""
    code = np.zeros(256, np.int64)
    for i, ch in enumerate(b"ACGMT"):
        code[ch] = i
    c = code[np.asarray(strings, np.uint8)]
    n = c.shape[-1] - ABEA_K + 1
    r = np.zeros(c.shape[:-1] + (n,), np.int64)
    for i in range(ABEA_K):
        r = r * 5 + c[..., i:i + n]
    return np.where(np.asarray(rc)[..., None].astype(bool), r[..., ::-1], r)


def abea_hmm_items(rng, shapes, model=None, rc=None, flags=3, meth="pair", noise=0.7, cpg=0.08, non_acgmt=0.0,
                   outliers=0, quantum=None, scale=(0.95, 1.05), shift=(-4.0, 4.0), var=(0.9, 1.2), epb=(1.1, 3.0),
                   lead=2):
    """Synthetic site groups for abea.hmm_score. `shapes` is a list of (count, n_kmers, n_rows): `count` reads,
    each with one CG-bearing string of n_kmers + 5 bases (CG planted with probability `cpg` per position and
    always in the middle), on the strand `rc` (0, 1, or None for a random one per read), and n_rows events
    drawn from the levels of the string's k-mers in the order the strand visits them (row r from k-mer
    r * n_kmers // n_rows, `noise` stdv of Gaussian noise; `outliers` rows per read lie 40 stdv off), between
    `lead` other events on either side. `meth`: "pair" gives two items per read, the string and its methylated
    copy (CG turned into MG) over the same events; "none" and "only" give one of them. scale, shift, var and
    epb are a value or a (lo, hi) range per read; with `quantum` events are rounded to its multiples. `flags`
    is a value or a list to draw from."""
    model = abea_cpg_model(rng) if model is None else model
    C, G, M, N = (ord(x) for x in "CGMN")

    def draw(v, n):
        return rng.uniform(v[0], v[1], n) if isinstance(v, tuple) else np.full(n, float(v))

    seqs, events, reads, items = [], [], [], []
    seq_pos = ev_pos = n_reads = 0
    for count, nk, rows in shapes:
        L = nk + ABEA_K - 1
        b = BASES[rng.integers(0, 4, (count, L))].copy()
        cg = rng.random((count, L - 1)) < cpg
        cg[:, (L - 1) // 2] = True
        ii = np.nonzero(cg)
        b[ii[0], ii[1]] = C
        b[ii[0], ii[1] + 1] = G
        if non_acgmt:
            b[rng.random(b.shape) < non_acgmt] = N
        m = b.copy()
        m[:, :-1][(b[:, :-1] == C) & (b[:, 1:] == G)] = M
        strand = rng.integers(0, 2, count) if rc is None else np.full(count, int(rc))
        ranks = abea_hmm_kmer_ranks(b, strand)
        lv = model[ranks[:, (np.arange(rows) * nk) // rows]]  # [count, rows, 3]
        sc, sh, vr = (draw(v, count).astype(np.float32) for v in (scale, shift, var))
        ev = (sc[:, None] * lv[..., 0] + sh[:, None]
              + noise * lv[..., 1] * vr[:, None] * rng.standard_normal((count, rows)))
        for _ in range(outliers):
            at = rng.integers(0, rows, count)
            ev[np.arange(count), at] += 40.0 * lv[np.arange(count), at, 1] * vr
        n_ev = rows + 2 * lead
        arr = rng.uniform(60, 120, (count, n_ev))
        first = np.where(strand == 1, lead + rows - 1, lead)  # row 1's event
        pos = first[:, None] + np.where(strand == 1, -1, 1)[:, None] * np.arange(rows)[None, :]
        arr[np.arange(count)[:, None], pos] = ev
        if quantum:
            arr = np.round(arr / quantum) * quantum
        rd = np.zeros(count, ABEA_HMM_READ_DTYPE)
        rd["event_off"] = ev_pos + n_ev * np.arange(count, dtype=np.int64)
        rd["n_events"] = n_ev
        rd["scale"], rd["shift"], rd["var"] = sc, sh, vr
        rd["log_var"] = np.log(vr.astype(np.float64)).astype(np.float32)
        rd["events_per_base"] = draw(epb, count)
        strings = {"pair": (b, m), "none": (b,), "only": (m,)}[meth]
        it = np.zeros((count, len(strings)), ABEA_HMM_ITEM_DTYPE)
        it["seq_off"] = seq_pos + L * (len(strings) * np.arange(count, dtype=np.int64)[:, None] + np.arange(len(strings)))
        it["seq_len"] = L
        it["read"] = (n_reads + np.arange(count))[:, None]
        it["event_start"] = first[:, None]
        it["event_stop"] = (first + np.where(strand == 1, -1, 1) * (rows - 1))[:, None]
        it["rc"] = strand[:, None]
        it["flags"] = (rng.choice(np.asarray(flags), count) if np.ndim(flags) else np.full(count, flags))[:, None]
        seqs.append(np.stack(strings, 1).reshape(-1))
        events.append(arr.astype(np.float32).reshape(-1))
        reads.append(rd)
        items.append(it.reshape(-1))
        seq_pos += L * len(strings) * count
        ev_pos += n_ev * count
        n_reads += count
    return AbeaHmmItems(model, np.concatenate(seqs), np.concatenate(events), np.concatenate(reads),
                        np.concatenate(items))


# ---- abea: Viterbi event alignment with traceback (benchmarks/abea, profile_hmm_align) ----


class AbeaAlignItems(AbeaHmmItems):
    """Items for abea.hmm_align: AbeaHmmItems over the nucleotide model, float32 [4096, 3] by k-mer rank over ACGT
    (gen.abea_model); flags are 0 and every item has at least two rows (include/gb_bsw_abea_viterbi.h)."""

    MODEL_SIZE = 4096


def abea_align_kmer_ranks(strings, rc):
    """Ranks [..., n_kmers] of the k-mers of ASCII strings [..., len] in the order profile_hmm_align visits them:
    k-mer ki starts at ki for rc == 0 and at len - ki - 6 for rc == 1; two bits per base with A C G T = 0..3 and
    any other byte 0 (eventalign.c:244-291, 434-446)."""
    code = np.zeros(256, np.int64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    c = code[np.asarray(strings, np.uint8)]
    n = c.shape[-1] - ABEA_K + 1
    r = np.zeros(c.shape[:-1] + (n,), np.int64)
    for i in range(ABEA_K):
        r = r * 4 + c[..., i:i + n]
    return np.where(np.asarray(rc)[..., None].astype(bool), r[..., ::-1], r)


def abea_align_items(rng, shapes, model=None, rc=None, noise=0.7, non_acgt=0.0, outliers=0, outlier_every=0,
                     homopolymer=0, quantum=None, scale=(0.95, 1.05), shift=(-4.0, 4.0), var=(0.9, 1.2), epb=(1.1, 3.0),
                     lead=2):
    """Synthetic windows for abea.hmm_align. `shapes` is a list of (count, n_kmers, n_rows): `count` reads, each
    with one item, a random ACGT string of n_kmers + 5 bases (bytes turned into N with probability `non_acgt`, the
    middle one always;
    with `homopolymer` a run of that many equal bases in the middle) on the strand `rc` (0, 1, or None for a
    random one per read), and n_rows >= 2 events drawn from the levels of the string's k-mers in the order the
    strand visits them (row r from k-mer r * n_kmers // n_rows, `noise` stdv of Gaussian noise; `outliers` rows
    per read, and every `outlier_every`-th row, lie 40 pA off), between `lead` other events on either side.
    scale, shift, var and epb are a value or a (lo, hi) range per read; with `quantum` events are rounded to its
    multiples."""
    model = abea_model(rng) if model is None else model
    N = ord("N")

    def draw(v, n):
        return rng.uniform(v[0], v[1], n) if isinstance(v, tuple) else np.full(n, float(v))

    seqs, events, reads, items = [], [], [], []
    seq_pos = ev_pos = n_reads = 0
    for count, nk, rows in shapes:
        L = nk + ABEA_K - 1
        b = BASES[rng.integers(0, 4, (count, L))].copy()
        if homopolymer:
            h = min(int(homopolymer), L)
            b[:, (L - h) // 2:(L - h) // 2 + h] = b[:, (L - h) // 2][:, None]
        if non_acgt:
            b[rng.random(b.shape) < non_acgt] = N
            b[:, L // 2] = N
        strand = rng.integers(0, 2, count) if rc is None else np.full(count, int(rc))
        ranks = abea_align_kmer_ranks(b, strand)
        lv = model[ranks[:, (np.arange(rows) * nk) // rows]]  # [count, rows, 3]
        sc, sh, vr = (draw(v, count).astype(np.float32) for v in (scale, shift, var))
        ev = (sc[:, None] * lv[..., 0] + sh[:, None]
              + noise * lv[..., 1] * vr[:, None] * rng.standard_normal((count, rows)))
        for _ in range(outliers):
            at = rng.integers(0, rows, count)
            ev[np.arange(count), at] += 40.0
        if outlier_every:
            ev[:, outlier_every - 1::outlier_every] += 40.0
        n_ev = rows + 2 * lead
        arr = rng.uniform(60, 120, (count, n_ev))
        first = np.where(strand == 1, lead + rows - 1, lead)  # row 1's event
        pos = first[:, None] + np.where(strand == 1, -1, 1)[:, None] * np.arange(rows)[None, :]
        arr[np.arange(count)[:, None], pos] = ev
        if quantum:
            arr = np.round(arr / quantum) * quantum
        rd = np.zeros(count, ABEA_HMM_READ_DTYPE)
        rd["event_off"] = ev_pos + n_ev * np.arange(count, dtype=np.int64)
        rd["n_events"] = n_ev
        rd["scale"], rd["shift"], rd["var"] = sc, sh, vr
        rd["log_var"] = np.log(vr.astype(np.float64)).astype(np.float32)
        rd["events_per_base"] = draw(epb, count)
        it = np.zeros(count, ABEA_HMM_ITEM_DTYPE)
        it["seq_off"] = seq_pos + L * np.arange(count, dtype=np.int64)
        it["seq_len"] = L
        it["read"] = n_reads + np.arange(count)
        it["event_start"] = first
        it["event_stop"] = first + np.where(strand == 1, -1, 1) * (rows - 1)
        it["rc"] = strand
        seqs.append(b.reshape(-1))
        events.append(arr.astype(np.float32).reshape(-1))
        reads.append(rd)
        items.append(it)
        seq_pos += L * count
        ev_pos += n_ev * count
        n_reads += count
    return AbeaAlignItems(model, np.concatenate(seqs), np.concatenate(events), np.concatenate(reads),
                          np.concatenate(items))


# ---- chain: base-level alignment items (gb_chain_extd2, minimap2's ksw_extd2_sse) ----

EXTD2_PARAMS_DTYPE = np.dtype([(f, "i1") for f in ("a", "b", "sc_ambi", "q", "e", "q2", "e2", "pad")])
EXTD2_ITEM_DTYPE = np.dtype([("q_off", "<i8"), ("t_off", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"), ("w", "<i4"),
                             ("zdrop", "<i4"), ("end_bonus", "<i4"), ("flag", "<i4")])
assert EXTD2_PARAMS_DTYPE.itemsize == 8 and EXTD2_ITEM_DTYPE.itemsize == 40
# (a, b, sc_ambi, q, e, q2, e2) of minimap2's presets (options.c) that write CIGARs
EXTD2_PRESETS = {"map-ont": (2, 4, 1, 4, 2, 24, 1), "asm5": (1, 19, 1, 39, 3, 81, 1), "asm20": (1, 4, 1, 6, 2, 26, 1),
                 "sr": (2, 8, 1, 12, 2, 24, 1)}
# mm_align1's four uses of ksw_extd2_sse: left extension, the two passes of a gap fill, right extension
EXTD2_USES = (0x40 | 0x02 | 0x80, 0x08, 0, 0x40)


class Extd2Items:
    """Items for chain.extd2: `params` one EXTD2_PARAMS_DTYPE record, `seqs` the concatenated base codes (0..3,
    4 for N) and `items` EXTD2_ITEM_DTYPE records (include/gb_chain_extd2.h)."""

    def __init__(self, params, seqs, items):
        self.params = np.ascontiguousarray(params, EXTD2_PARAMS_DTYPE).reshape(1)
        self.seqs = np.ascontiguousarray(seqs, np.uint8)
        self.items = np.ascontiguousarray(items, EXTD2_ITEM_DTYPE)

    @property
    def n(self):
        return len(self.items)

    def subset(self, idx):
        """The same parameters and bases with items[idx]."""
        return type(self)(self.params, self.seqs, self.items[np.asarray(idx, np.int64)])

    @classmethod
    def concat(cls, parts):
        """The items of several sets over the first part's parameters, offsets shifted."""
        items, pos = [], 0
        for p in parts:
            it = p.items.copy()
            it["q_off"] += pos
            it["t_off"] += pos
            items.append(it)
            pos += len(p.seqs)
        return cls(parts[0].params, np.concatenate([p.seqs for p in parts]), np.concatenate(items))

    def item(self, i):
        """(query codes, target codes, item record) of item i."""
        it = self.items[i]
        return (self.seqs[it["q_off"]:it["q_off"] + it["qlen"]], self.seqs[it["t_off"]:it["t_off"] + it["tlen"]], it)


def extd2_params(a, b, sc_ambi, q, e, q2, e2):
    p = np.zeros(1, EXTD2_PARAMS_DTYPE)
    for f, v in zip(("a", "b", "sc_ambi", "q", "e", "q2", "e2"), (a, b, sc_ambi, q, e, q2, e2)):
        p[f] = np.array(v).astype(np.int8)
    return p


def extd2_query(rng, target, qlen, sub=0.06, indel=0.04, long_indel=0.0, repeat=0, n_rate=0.0, tail=0.0):
    """A query of qlen codes derived from `target`: substitutions, indels of 1..3 bases, with rate `long_indel`
    indels of 10..60 bases, the last `tail` part unrelated; `repeat` > 0 first turns the middle of the target (in
    place) into a tandem repeat of that period, which is where left- and right-aligned gaps differ."""
    tlen = len(target)
    if repeat and tlen > 3 * repeat:
        a = tlen // 4
        unit = target[a:a + repeat].copy()
        span = target[a:a + tlen // 2]
        span[:] = np.resize(unit, len(span))
    out, i = [], 0
    while i < tlen and len(out) < qlen:
        u = rng.random()
        if u < long_indel:
            L = int(rng.integers(10, 61))
            if rng.random() < 0.5:
                i += L
            else:
                out.extend(rng.integers(0, 4, L).tolist())
        elif u < long_indel + indel:
            L = int(rng.integers(1, 4))
            if rng.random() < 0.5:
                i += L
            else:
                out.extend(rng.integers(0, 4, L).tolist())
        elif u < long_indel + indel + sub:
            out.append(int((target[i] + rng.integers(1, 4)) % 4) if target[i] < 4 else int(rng.integers(0, 4)))
            i += 1
        else:
            out.append(int(target[i]))
            i += 1
    out = np.array(out[:qlen], np.uint8)
    if len(out) < qlen:
        out = np.concatenate([out, rng.integers(0, 4, qlen - len(out)).astype(np.uint8)])
    if tail > 0:
        k = int(qlen * (1 - tail))
        out[k:] = rng.integers(0, 4, qlen - k)
    if n_rate > 0:
        out[rng.random(qlen) < n_rate] = 4
    return out


def extd2_items(rng, shapes, params="map-ont", w=None, zdrop=None, end_bonus=None, flag=None, **mut):
    """A seeded Extd2Items: `shapes` is a list of (qlen, tlen); per item a target is drawn (with N bases at
    mut['n_rate']) and the query derived from it by extd2_query(**mut). `w`, `zdrop`, `end_bonus` and `flag` are
    a value for every item, a sequence to draw from, or None: then w is drawn from (-1, 10, 50, 200, 751), zdrop
    from (-1, 30, 400), end_bonus from (-1, 10) and flag from EXTD2_USES."""
    if isinstance(params, str):
        params = extd2_params(*EXTD2_PRESETS[params])

    def draw(v, default):
        v = default if v is None else v
        return int(v) if np.isscalar(v) else int(v[rng.integers(0, len(v))])

    seqs, items, pos = [], np.zeros(len(shapes), EXTD2_ITEM_DTYPE), 0
    for k, (qlen, tlen) in enumerate(shapes):
        target = rng.integers(0, 4, tlen).astype(np.uint8)
        if mut.get("n_rate", 0.0) > 0:
            target[rng.random(tlen) < mut["n_rate"]] = 4
        query = extd2_query(rng, target, qlen, **mut) if tlen else rng.integers(0, 4, qlen).astype(np.uint8)
        items[k] = (pos, pos + qlen, qlen, tlen, draw(w, (-1, 10, 50, 200, 751)), draw(zdrop, (-1, 30, 400)),
                    draw(end_bonus, (-1, 10)), draw(flag, EXTD2_USES))
        seqs += [query, target]
        pos += qlen + tlen
    return Extd2Items(params, np.concatenate(seqs) if seqs else np.zeros(0, np.uint8), items)


# ---- poa: windows of noisy reads of a template ----

POA_ALPHABET = b"ACGT"


def poa_template(rng, length, kind="random", alphabet=POA_ALPHABET):
    """A template of `length` bytes: "random" over the alphabet, "homopolymer" (runs of 3..12 of one base) or
    "period" (a random unit of 2..4 bases repeated), the last two for ties."""
    al = np.frombuffer(bytes(alphabet), np.uint8)
    if kind == "random":
        return al[rng.integers(0, len(al), length)].tobytes()
    if kind == "period":
        unit = al[rng.integers(0, len(al), int(rng.integers(2, 5)))]
        return np.resize(unit, length).tobytes()
    assert kind == "homopolymer", kind
    out = []
    while len(out) < length:
        out += [int(al[rng.integers(0, len(al))])] * int(rng.integers(3, 13))
    return bytes(out[:length])


def poa_read(rng, template, sub=0.04, ins=0.04, dele=0.04, long_indel=0.0, long_len=(25, 40), start=0, end=None,
             alphabet=POA_ALPHABET):
    """A read of template[start:end] with substitution, insertion and deletion rates per base, and, at rate
    long_indel per base, an insertion or a deletion of long_len[0] .. long_len[1] bases."""
    al = np.frombuffer(bytes(alphabet), np.uint8)
    t = np.frombuffer(bytes(template), np.uint8)[start:end]
    out, i = [], 0
    while i < len(t):
        u = rng.random()
        if u < long_indel:
            k = int(rng.integers(long_len[0], long_len[1] + 1))
            if rng.random() < 0.5:
                out += [int(x) for x in al[rng.integers(0, len(al), k)]]
            else:
                i += k
        elif u < long_indel + ins:
            out.append(int(al[rng.integers(0, len(al))]))
        elif u < long_indel + ins + dele:
            i += 1
        elif u < long_indel + ins + dele + sub:
            others = al[al != t[i]]
            out.append(int(others[rng.integers(0, len(others))]) if len(others) else int(t[i]))
            i += 1
        else:
            out.append(int(t[i]))
            i += 1
    return bytes(out)


def poa_window(rng, n_reads, length, err=0.12, long_indel=0.0, clip=0.0, kind="random", alphabet=POA_ALPHABET,
               quals=False):
    """A window: a template of `length` bytes and n_reads reads of it at a total error rate `err`, split evenly
    over substitutions, insertions and deletions. With probability `clip` a read starts or ends up to a third of
    the way inside the template. Returns (reads, quals or None); a quality string holds bytes 33 .. 73."""
    t = poa_template(rng, length, kind, alphabet)
    reads = []
    for _ in range(n_reads):
        start, end = 0, len(t)
        if rng.random() < clip:
            if rng.random() < 0.5:
                start = int(rng.integers(0, len(t) // 3 + 1))
            else:
                end = len(t) - int(rng.integers(0, len(t) // 3 + 1))
        reads.append(poa_read(rng, t, err / 3, err / 3, err / 3, long_indel, start=start, end=end, alphabet=alphabet))
    qs = [rng.integers(33, 74, len(r)).astype(np.uint8).tobytes() for r in reads] if quals else None
    return reads, qs


def poa_windows(rng, n_windows, reads=(2, 12), length=(20, 300), err=0.12, long_indel=0.0, clip=0.0, kind="random",
                alphabet=POA_ALPHABET):
    """n_windows windows (lists of reads as bytes) with read counts and template lengths drawn from the closed
    ranges `reads` and `length`."""
    return [poa_window(rng, int(rng.integers(reads[0], reads[1] + 1)), int(rng.integers(length[0], length[1] + 1)),
                       err, long_indel, clip, kind, alphabet)[0] for _ in range(n_windows)]


def write_poa_file(path, windows):
    """The poa benchmark's input: a header line per read, whose second character is '0' for the first read of a
    window, then the read on a line of its own."""
    with open(path, "w") as f:
        for reads in windows:
            for k, r in enumerate(reads):
                f.write(f">{k}\n{bytes(r).decode()}\n")


# ---------------------------------------------------------------------------------------------------- kmer

def kmer_reads(seed, genome_len, coverage, read_len_range=(1000, 20000), error_rate=0.05, repeats=0):
    """Long reads over a random genome for the k-mer leg, as a list of u8 ACGT arrays: `repeats` copies of a 500-base
    family are planted in the genome, reads start uniformly, have lengths drawn from the closed range, come from
    either strand with equal chance and carry substitutions, insertions and deletions at error_rate in all. Reads
    are drawn until their bases reach coverage * genome_len."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, int(genome_len))]
    if repeats and genome_len > 2000:
        family = acgt[rng.integers(0, 4, 500)]
        for _ in range(int(repeats)):
            at = int(rng.integers(0, genome_len - 500))
            genome[at:at + 500] = family
    lo, hi = int(read_len_range[0]), int(min(read_len_range[1], genome_len))
    reads, total = [], 0
    while total < coverage * genome_len:
        n = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, genome_len - n + 1))
        r = genome[at:at + n].copy()
        if rng.random() < 0.5:
            r = acgt[3 - np.searchsorted(acgt, r)][::-1].copy()
        if error_rate > 0:
            u = rng.random(n)
            sub = u < error_rate / 3
            r[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
            dele = (u >= error_rate / 3) & (u < 2 * error_rate / 3)
            ins = (u >= 2 * error_rate / 3) & (u < error_rate)
            keep = np.repeat(np.arange(n), 1 + ins.astype(np.int64) - dele.astype(np.int64))
            r = r[keep]
            r = r[:hi] if len(r) >= lo else np.concatenate([r, acgt[rng.integers(0, 4, lo - len(r))]])
        reads.append(np.ascontiguousarray(r))
        total += len(r)
    return reads


# ----------------------------------------------------------------------------------------------------- dbg

def dbg_regions(seed, n_regions, region=1500, n_reads=300, read_len=150, sub_rate=0.01, n_rate=0.002, low_qual=0.03,
                repeat_every=0, qc_fail=0.01):
    """Overlapping assembly regions over a random genome for the dbg leg, shaped as the reference's driver shapes
    them: region i assembles [a, a + region) with a = region + i * region / 2, its reference is the 3 * region bases
    around it and its reads are those of the sorted pool that overlap it, about n_reads each. Reads of read_len bases
    carry substitutions, a few 'N's, qualities of 30..40 with a fraction low_qual below 20, and the QC-fail flag at
    rate qc_fail. Every repeat_every-th region (0: none) gets a 24-base unit planted twice, 40 bases apart, so that
    its graph is cyclic at k = 15 and 20. Returns (regions, reads) as dbg.pack takes them: regions of
    (reference u8, ref_start, read_first, read_last), reads of (sequence u8, qualities u8, flag)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    shift = region // 2
    length = 3 * region + shift * (int(n_regions) - 1)
    genome = acgt[rng.integers(0, 4, length)]
    starts = [region + i * shift for i in range(int(n_regions))]
    if repeat_every:
        for a in starts[::int(repeat_every)]:
            at = a + int(rng.integers(0, shift - 100))
            genome[at + 40:at + 64] = genome[at:at + 24]
    total = max(1, int(n_reads * length / (region + read_len)))
    pos = np.sort(rng.integers(0, length - read_len + 1, total))
    reads = []
    for p in pos:
        s = genome[p:p + read_len].copy()
        u = rng.random(read_len)
        sub = u < sub_rate
        s[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
        s[(u >= sub_rate) & (u < sub_rate + n_rate)] = ord("N")
        q = rng.integers(30, 41, read_len).astype(np.uint8)
        low = rng.random(read_len) < low_qual
        q[low] = rng.integers(2, 20, int(low.sum()))
        reads.append((s, q, 512 if rng.random() < qc_fail else 0))
    regions = []
    for a in starts:
        first = int(np.searchsorted(pos + read_len, a, side="right"))
        last = int(np.searchsorted(pos, a + region, side="left"))
        regions.append((genome[a - region:a + 2 * region].copy(), a - region, first, max(first, last)))
    return regions, reads
