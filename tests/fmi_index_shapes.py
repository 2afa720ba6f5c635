"""Index-side edge inputs for the fmi path (tests/test_fmi_index_edges.py): references chosen for
where they put the sentinel row, the end of the last 64-row block and the last sampled row, texts
the builder's 21-mer sort cannot resolve (shorter than the key, homopolymers, a text equal to its
own reverse complement, short-period tandems), a brute-force index over them that shares no code
with the oracle's or the product's suffix sort, and read sets whose SMEM intervals start and end at
the sentinel row.

CPU only. The witnesses that these inputs reach the edges they are meant for are the oracle's edge
counters (oracle/fmi_oracle.c, OracleIndex.edges()); tests/test_fmi_index_edges.py asserts them."""
from __future__ import annotations

import numpy as np

import fmi_util

BASES = "ACGT"


def revcomp(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def text_of(ref):
    """The indexed text: forward strand then its reverse complement (pac2nt)."""
    ref = np.asarray(ref, np.uint8)
    return np.concatenate([ref, revcomp(ref)])


# ------------------------------------------------------------------ a. the catalogue
RANDOM_G = (1, 2, 3, 4, 10, 20, 21, 22, 31, 32, 33, 64)
HOMO_G = (1, 5, 40, 300)
PLANTED_G = 600


def random_ref(G):
    return np.random.default_rng(7000 + G).integers(0, 4, G, dtype=np.uint8)


def planted(G, seed):
    """Random text with ref[40] = C whose first 64 bases are copied to G/4, G/2 and 3G/4 with position
    40 of the copies set to A, G and T: the whole forward text, which is the sentinel row's suffix,
    has suffix-order neighbours on both sides that share 40 bases with it."""
    ref = np.random.default_rng(seed).integers(0, 4, G, dtype=np.uint8)
    ref[40] = 1
    head = ref[:64].copy()
    for d, b in ((G // 4, 0), (G // 2, 2), (3 * G // 4, 3)):
        ref[d:d + 64] = head
        ref[d + 40] = b
    return ref


def staggered(G, seed, low):
    """planted() with the three copies diverging from the head of the text at positions 30, 40 and 50
    instead of all at 40. With `low` the copy that diverges at 30 sorts below the whole text and the two
    others above it, so a match of 31 .. 50 bases of the head is an interval of two or three rows that
    starts at the sentinel row z; without, the copy that diverges at 30 sorts above and the others
    below, and the interval ends at z + 1. In planted() the sentinel row is either alone in its
    interval or strictly inside it, and an extension of the one-row interval is always empty, so the
    `k <= z` of backwardExt's sentinel offset decides nothing that survives there."""
    ref = np.random.default_rng(seed).integers(0, 4, G, dtype=np.uint8)
    ref[[30, 40, 50]] = 1
    head = ref[:64].copy()
    first, rest = (0, 3) if low else (2, 0)
    for d, pos, b in ((G // 4, 30, first), (G // 2, 40, rest), (3 * G // 4, 50, rest)):
        ref[d:d + 64] = head
        ref[d + pos] = b
    return ref


STAGGERED = {"staggered_low": (5, True), "staggered_high": (6, False)}

# name -> (seed, class): the sentinel row z of planted(PLANTED_G, seed) has z % 64 (or z % 8) equal
# to the value, or lies in the last 64-row block. Found by scanning seeds upwards with the oracle;
# test_planted_seed_classes holds them in place.
PLANTED = {
    "planted_z64_0": (17, ("mod64", 0)),
    "planted_z64_1": (245, ("mod64", 1)),
    "planted_z64_31": (14, ("mod64", 31)),
    "planted_z64_32": (11, ("mod64", 32)),
    "planted_z64_63": (13, ("mod64", 63)),
    "planted_z8_0": (1, ("mod8", 0)),
    "planted_last_block": (3, ("last_block", None)),
}


def planted_class_holds(cls, n, z):
    kind, v = cls
    if kind == "mod64":
        return z % 64 == v
    if kind == "mod8":
        return z % 8 == v
    return z >> 6 == n >> 6


def _catalogue():
    cat = {}
    for G in RANDOM_G:
        cat[f"random_{G}"] = random_ref(G)
    for b in range(4):
        for G in HOMO_G:
            cat[f"homo_{BASES[b]}_{G}"] = np.full(G, b, np.uint8)
    cat["acgt_x100"] = np.resize(np.array([0, 1, 2, 3], np.uint8), 400)
    x = np.random.default_rng(7777).integers(0, 4, 200, dtype=np.uint8)
    cat["x_revcomp_x"] = np.concatenate([x, revcomp(x)])
    cat["at_x150"] = np.resize(np.array([0, 3], np.uint8), 300)
    cat["cgg_500"] = np.resize(np.array([1, 2, 2], np.uint8), 500)
    for name, (seed, _) in PLANTED.items():
        cat[name] = planted(PLANTED_G, seed)
    for name, (seed, low) in STAGGERED.items():
        cat[name] = staggered(PLANTED_G, seed, low)
    return cat


CATALOGUE = _catalogue()
NAMES = list(CATALOGUE)
SENTINEL_NAMES = list(PLANTED) + list(STAGGERED)  # the references sentinel_reads is run on
WIDE_NAMES = ["random_1", "homo_A_300", "acgt_x100", "x_revcomp_x", "planted_z64_0"]


# ------------------------------------------------------------------ b. brute-force index
class Brute:
    """The .bwt.2bit.64 content of a small reference from Python's own sort of the suffixes' bytes (a
    proper prefix sorts first, which is end-of-text smallest; SA[0] = N is the empty suffix):
    n, count (as loaded, +1), sentinel, bwt (4 at the sentinel row), cp (int64[(n >> 6) + 1, 8] CP_OCC
    lines), sa (every row) and sa_sampled (every 8th)."""

    def __init__(self, ref):
        text = text_of(ref)
        t = text.tobytes()
        N = len(t)
        sa = np.array([N] + sorted(range(N), key=lambda i: t[i:]), np.int64)
        n = N + 1
        bwt = np.where(sa > 0, text[np.maximum(sa - 1, 0)], 4).astype(np.int64)
        c4 = np.bincount(text, minlength=4)[:4]
        self.n = n
        self.count = (np.concatenate([[0], np.cumsum(c4)]) + 1).tolist()
        self.sentinel = int(np.nonzero(sa == 0)[0][0])
        self.sa, self.bwt = sa, bwt
        self.sa_sampled = sa[::8].copy()
        nb = (n >> 6) + 1
        cp = np.zeros((nb, 8), np.uint64)
        for b in range(nb):
            rows = bwt[b * 64:(b + 1) * 64]
            for c in range(4):
                cp[b, c] = int((bwt[:b * 64] == c).sum())
                word = 0
                for j, v in enumerate(rows.tolist()):
                    if v == c:
                        word |= 1 << (63 - j)
                cp[b, 4 + c] = word
        self.cp = cp.view(np.int64)

    def info(self):
        return self.n, self.count, self.sentinel

    def sa_lookup(self, mode):
        """What an LF walk from every row answers: SA[row] (mode 0); in mode 1, 0 where the walk reaches
        the sentinel row after at least one step before it reaches a sampled row."""
        if mode == 0:
            return self.sa.copy()
        isa = np.zeros(self.n, np.int64)
        isa[self.sa] = np.arange(self.n)
        out = self.sa.copy()
        for r in range(self.n):
            p = int(self.sa[r])
            while isa[p] & 7:
                if p == 0:
                    if p != self.sa[r]:
                        out[r] = 0
                    break
                p -= 1
        return out


def largest_prefix_bin(ref, width=8):
    """The most suffixes of the text that share their first `width` symbols, counted the way the
    builder's prefix histogram does (a symbol past the end of the text counts as its own value 0)."""
    t = text_of(ref).astype(np.int64) + 1
    pad = np.concatenate([t, np.zeros(width, np.int64)])
    key = np.zeros(len(t), np.int64)
    for j in range(width):
        key = key * 8 + pad[j:j + len(t)]
    return int(np.unique(key, return_counts=True)[1].max())


# ------------------------------------------------------------------ c. read sets
def sentinel_reads(ref, oracle_index, L=64, max_off=40, seed=0):
    """Reads that end in the suffixes of the sentinel row and its two neighbours: for each of the rows
    z - 1, z, z + 1 with s = SA[row], and each offset o in 1 .. max_off - 1, the L bases of the text
    from s - o (random bases where that lies outside the text), once per substitution position
    p < o, each also reverse-complemented. Returns (codes, lens)."""
    text = text_of(ref)
    N = len(text)
    n, _, z = oracle_index.info()
    rows = np.array([r for r in (z - 1, z, z + 1) if 0 <= r < n], np.int64)
    rng = np.random.default_rng(seed)
    out = []
    for s in oracle_index.sa_lookup(rows, 0).tolist():
        for o in range(1, max_off):
            pos = np.arange(s - o, s - o + L)
            inside = (pos >= 0) & (pos < N)
            base = rng.integers(0, 4, L, dtype=np.uint8)
            base[inside] = text[pos[inside]]
            for p in range(o):
                r = base.copy()
                r[p] = (r[p] + rng.integers(1, 4)) % 4
                out.append(r)
                out.append(revcomp(r))
    codes = np.stack(out)
    return codes, np.full(len(codes), L, np.int32)


def degenerate_reads(ref, L=48, seed=0):
    """40 reads of up to L bases for a tiny or degenerate text: by turns the text tiled past its end
    (np.resize from a random start), a window of the text (followed by random bases where the text is
    shorter than L) and random bases; every seventh has one N, every fifth is cut to a length drawn
    from 1 .. L."""
    text = text_of(ref)
    N = len(text)
    rng = np.random.default_rng(seed + 31 * N)
    codes = np.zeros((40, L), np.uint8)
    lens = np.full(40, L, np.int32)
    for i in range(40):
        r = rng.integers(0, 4, L, dtype=np.uint8)
        if i % 3 == 0:
            r = np.resize(np.roll(text, -int(rng.integers(0, N))), L)
        elif i % 3 == 1:
            s = int(rng.integers(0, max(1, N - L + 1)))
            w = text[s:s + L]
            r[:len(w)] = w
        if i % 7 == 0:
            r[int(rng.integers(0, L))] = 4
        if i % 5 == 0:
            lens[i] = int(rng.integers(1, L + 1))
        codes[i] = r
    return codes, lens


def edge_smems(n, z):
    """Hand-made SMEM intervals for the SA lookup: every row, the sentinel row alone and with either
    neighbour side, and for max_occ in {1, 3, 7} intervals of max_occ, max_occ + 1, 2 max_occ - 1 and
    2 max_occ rows that end at the last row. Returns {max_occ: SMEM array}; the first four intervals
    are in every set."""
    base = [(0, n), (z, 1), (z - 1, 2), (z + 1, n - z - 1)]
    out = {}
    for mo in (1, 3, 7):
        iv = list(base) + [(n - w, w) for w in (mo, mo + 1, 2 * mo - 1, 2 * mo)]
        iv = [(k, s) for k, s in iv if k >= 0 and s >= 0 and k + s <= n]
        sm = np.zeros(len(iv), fmi_util.SMEM_DTYPE)
        sm["k"] = [k for k, _ in iv]
        sm["s"] = [s for _, s in iv]
        out[mo] = sm
    return out
