"""The k-mer contract restated with numpy (include/gb_fmi_kmer.h, DESIGN.md "kmer"): Flye's KmerCounter::count and
VertexIndex::buildIndexUnevenCoverage as sets and sorted lists. Both rate products are np.float32 multiplies.
tests/golden/make_kmer_golden.py asserts that it equals the live reference on every fixture set."""
import hashlib

import numpy as np

_LUT = np.full(256, 255, np.uint8)
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _LUT[ord(_c.lower())] = _i


def codes_of(read, k):
    """(forward codes u64, reverse-complement codes u64) of every k-mer position of one read (u8 ASCII)."""
    b = _LUT[np.asarray(read, np.uint8)]
    assert (b < 4).all(), "a byte that is no base"
    n = len(b) - k  # the reference's walk stops one k-mer before the end of the read (kmer.h:185-200)
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    fwd, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        x = b[j:j + n].astype(np.uint64)
        fwd |= x << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - x) << np.uint64(2 * j)
    return fwd, rc


def canonical(read, k):
    """(canonical codes, strand: True where the reverse complement is strictly smaller)"""
    fwd, rc = codes_of(read, k)
    rev = rc < fwd
    return np.where(rev, rc, fwd), rev


def count(k, reads):
    """(codes ascending u64, counts u32) over all forward reads."""
    parts = [canonical(r, k)[0] for r in reads]
    allc = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    codes, counts = np.unique(allc, return_counts=True)
    return codes.astype(np.uint64), counts.astype(np.uint32)


def stats(codes, counts):
    return {"n_distinct": int(len(codes)), "n_occurrences": int(counts.astype(np.int64).sum()),
            "n_over15": int((counts >= 16).sum()), "max_count": int(counts.max()) if len(counts) else 0}


def hist(counts, n_bins):
    return np.bincount(np.minimum(counts.astype(np.int64), n_bins - 1), minlength=n_bins).astype(np.int64)


def freq(codes, counts, query):
    """getFreq of each query as given: 0 for absent and for non-canonical codes."""
    query = np.asarray(query, np.uint64)
    at = np.searchsorted(codes, query)
    at_c = np.minimum(at, max(len(codes) - 1, 0))
    hit = (at < len(codes)) & (codes[at_c] == query) if len(codes) else np.zeros(len(query), bool)
    return np.where(hit, counts[at_c] if len(codes) else 0, 0).astype(np.uint32)


def kept_positions(k, read, codes, counts, select_rate, tandem_freq):
    """yieldFrequentKmers: (canonical codes, strands, offsets, frequencies) of the kept positions of one read."""
    can, rev = canonical(read, k)
    n = len(can)
    if n == 0:
        return can, rev, np.zeros(0, np.int64), np.zeros(0, np.int64)
    f = counts[np.searchsorted(codes, can)].astype(np.int64)
    max_kmers = int(np.float32(select_rate) * np.float32(n))
    min_freq = np.sort(f)[::-1][max_kmers]
    keep = f >= min_freq
    if tandem_freq > 0:
        _, inv, local = np.unique(can, return_inverse=True, return_counts=True)
        keep &= local[inv] <= tandem_freq
    p = np.nonzero(keep)[0].astype(np.int64)
    return can[p], rev[p], p, f[p]


def index(k, reads, codes, counts, min_freq, select_rate, tandem_freq, repeat_rate):
    """(codes, off, pos, rep_codes, repetitive_frequency) of buildIndexUnevenCoverage."""
    ent_code, ent_pos, ent_freq = [], [], []
    base = 0
    for r in reads:
        length = len(r)
        c, rev, p, f = kept_positions(k, r, codes, counts, select_rate, tandem_freq)
        ok = f >= min_freq
        c, rev, p, f = c[ok], rev[ok], p[ok], f[ok]
        ent_code.append(c)
        ent_freq.append(f)
        ent_pos.append(np.where(rev, 2 * base + length + (length - p - k), 2 * base + p))
        base += length
    cat = (lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt))
    ec, ep, ef = cat(ent_code, np.uint64), cat(ent_pos, np.int64), cat(ent_freq, np.int64)
    # pass 1: capacities
    ucodes, inv, cap = np.unique(ec, return_inverse=True, return_counts=True)
    sel = cap >= min_freq
    total, unique = int(cap[sel].sum()), int(sel.sum())
    mean = np.float32(total) / np.float32(unique + 1)
    rep_freq = int(np.float32(repeat_rate) * mean)
    rep = cap > rep_freq
    # pass 2
    take = (ef <= rep_freq) & ~rep[inv] if len(ec) else np.zeros(0, bool)
    ec, ep = ec[take], ep[take]
    order = np.lexsort((ep, ec))
    ec, ep = ec[order], ep[order]
    out_codes, lens = np.unique(ec, return_counts=True)
    off = np.zeros(len(out_codes) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return out_codes.astype(np.uint64), off, ep, ucodes[rep].astype(np.uint64), rep_freq


def checksum(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + a.tobytes()).hexdigest()
