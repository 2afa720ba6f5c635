"""The read sets of tests/golden/kmer_golden.npz: how they are made, which labels they must show, how they are
stored and loaded. Shared by tests/golden/make_kmer_golden.py and tests/test_fmi_kmer.py."""
import numpy as np

import kmer_ref as ref

TILE = 4096
KS = (1, 4, 8, 11, 12, 13, 16, 17, 21, 31)
FLYE = (1, 0.4, 0, 100.0)  # min_freq, select_rate, tandem_freq, repeat_rate
_B = np.frombuffer(b"ACGT", np.uint8)

# each label names where the code can go wrong; the recorder asserts every count > 0, the tests the stored counts
LABELS = (
    "len_0", "len_k_minus_1", "len_k", "len_k_plus_1", "len_straddles_a_word", "short_reads_3000",
    "palindrome_even_k_forward", "odd_k", "count_14", "count_15", "count_16", "count_17", "count_over_255",
    "count_over_65535", "all_equal_keys", "de_bruijn_2080", "total_tile_minus_1", "total_tile", "total_tile_plus_1",
    "total_two_tiles_minus_1", "total_two_tiles", "total_two_tiles_plus_1", "select_0.4", "select_0.7_n10_f32_7",
    "select_0.7_n90_f32_63", "read_all_equal_freq", "tie_at_threshold", "min_freq_1", "min_freq_2", "tandem_0",
    "tandem_3_code_3_times", "tandem_3_code_4_times", "tandem_100_code_100_times", "tandem_100_code_101_times",
    "repeat_2_removes_codes", "repeat_100", "capacity_passes_frequency_cut", "reverse_offset_1",
    "reverse_offset_L_minus_k",
) + tuple(f"k_{k}" for k in KS)


def rnd(rng, n):
    return _B[rng.integers(0, 4, int(n))]


def revcomp(r):
    return _B[3 - np.searchsorted(_B, r)][::-1].copy()


def text(s):
    return np.frombuffer(s.encode(), np.uint8).copy()


def de_bruijn(k):
    """B(4, k) linearised with k more bases, so that the reference's walk (L - k k-mers) sees each k-mer once."""
    a, seq = [0] * (4 * k), []

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = np.array(seq + seq[:k], np.int64)
    return _B[s]


def edge_reads(rng, k):
    """Lengths 0, k - 1, k, k + 1 and word-straddling ones, both strands of a small genome, a palindrome under even
    k, and planted codes with counts 14..17."""
    genome = rnd(rng, 600)
    reads = [text(""), rnd(rng, k - 1), rnd(rng, k), rnd(rng, k + 1), rnd(rng, 33 + k), rnd(rng, 97 + k)]
    for _ in range(24):
        n = int(rng.integers(k + 2, 200))
        s = int(rng.integers(0, 600 - n))
        r = genome[s:s + n].copy()
        reads.append(revcomp(r) if rng.random() < 0.5 else r)
    if k % 2 == 0:
        reads.append(np.concatenate([text("AT" * (k // 2)), text("CC")]))
    if k >= 8:  # a planted k-mer c times, each in a read of its own with fresh flanks
        for c in (14, 15, 16, 17):
            core = rnd(rng, k)
            for j in range(c):
                r = np.concatenate([rnd(rng, 3 + j % 5), core, rnd(rng, 2 + j % 3)])
                reads.append(revcomp(r) if j % 3 == 0 else r)
    return reads


def index_reads(rng, k):
    """The index cases: reads with exactly 10 and 90 k-mers, a read whose frequencies are all equal, ties, tandem
    multiplicities 3, 4, 100 and 101, a repeat family that the filter removes."""
    genome = rnd(rng, 1500)
    reads = []
    for _ in range(40):
        n = int(rng.integers(60, 400))
        s = int(rng.integers(0, 1500 - n))
        r = genome[s:s + n].copy()
        reads.append(revcomp(r) if rng.random() < 0.5 else r)
    reads.append(genome[100:100 + 10 + k].copy())
    reads.append(genome[700:700 + 90 + k].copy())
    reads.append(rnd(rng, 50 + k))  # fresh: every frequency 1
    unit = rnd(rng, k + 3)
    for times in (3, 4, 100, 101):  # the unit's k-mers occur `times` times in the read
        reads.append(np.concatenate([rnd(rng, 30), np.tile(unit, times), unit[:k], rnd(rng, 30)]))
        unit = rnd(rng, k + 3)
    rep = rnd(rng, 60)
    for _ in range(30):  # a repeat family
        reads.append(np.concatenate([rnd(rng, 10), rep, rnd(rng, 10)]))
    return reads


def fixture_sets():
    """The sets in order. 'store' is 'whole' or 'sums'; 'recipe' sets are regenerated from their seed."""
    out = []
    for k in KS:
        rng = np.random.default_rng(1000 + k)
        s = {"name": f"edges_k{k}", "k": k, "reads": edge_reads(rng, k), "store": "whole", "flat": k == 17}
        if k in (8, 16):
            s["index"] = [FLYE]
        out.append(s)
    for k, params in ((11, [FLYE, (2, 0.7, 3, 2.0), (1, 0.7, 100, 2.0), (2, 0.4, 0, 100.0)]),
                      (4, [(1, 0.4, 3, 2.0)]), (13, [(1, 0.7, 3, 100.0), (2, 0.4, 100, 2.0)])):
        rng = np.random.default_rng(2000 + k)
        out.append({"name": f"index_k{k}", "k": k, "reads": index_reads(rng, k), "store": "sums", "index": params,
                    "recipe": ("index", 2000 + k)})
    rng = np.random.default_rng(3000)
    out.append({"name": "short_3000", "k": 11, "store": "sums", "recipe": ("short", 3000), "index": [FLYE],
                "reads": short_reads(rng, 11)})
    out.append({"name": "homopolymer", "k": 11, "store": "sums", "recipe": ("homopolymer", 0),
                "reads": [np.full(70000, ord("A"), np.uint8)], "index": [(1, 0.4, 0, 100.0)]})
    out.append({"name": "de_bruijn", "k": 6, "store": "sums", "recipe": ("de_bruijn", 6), "reads": [de_bruijn(6)]})
    for total in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        out.append({"name": f"total_{total}", "k": 12, "store": "sums", "recipe": ("total", total),
                    "reads": total_reads(total, 12), "index": [FLYE] if total == TILE + 1 else []})
    return out


def short_reads(rng, k):
    return [rnd(rng, k + 1 + i % 3) for i in range(3000)]


def total_reads(total, k):
    """Two reads with `total` k-mers between them."""
    rng = np.random.default_rng(total)
    first = total // 3
    return [rnd(rng, first + k), rnd(rng, total - first + k)]


def from_recipe(recipe, k):
    kind, arg = recipe
    if kind == "index":
        return index_reads(np.random.default_rng(arg), k)
    if kind == "short":
        return short_reads(np.random.default_rng(arg), k)
    if kind == "homopolymer":
        return [np.full(70000, ord("A"), np.uint8)]
    if kind == "de_bruijn":
        return [de_bruijn(arg)]
    if kind == "total":
        return total_reads(arg, k)
    raise ValueError(kind)


def count_labels(labels, s, got):
    """Adds this set's cases to labels (name -> count)."""
    def add(name, n=1):
        labels[name] = labels.get(name, 0) + int(n)

    k, reads, codes, counts = s["k"], s["reads"], got["codes"], got["counts"]
    add(f"k_{k}")
    if k % 2:
        add("odd_k")
    for r in reads:
        n = len(r)
        add("len_0", n == 0)
        add("len_k_minus_1", n == k - 1)
        add("len_k", n == k)
        add("len_k_plus_1", n == k + 1)
        add("len_straddles_a_word", n >= 33 + k)
    if len(reads) == 3000 and all(k + 1 <= len(r) <= k + 3 for r in reads):
        add("short_reads_3000")
    if k % 2 == 0:
        for r in reads:
            f, rc = ref.codes_of(r, k)
            add("palindrome_even_k_forward", ((f == rc) & ~(rc < f)).sum())
    for c in (14, 15, 16, 17):
        add(f"count_{c}", (counts == c).sum())
    add("count_over_255", (counts > 255).sum())
    add("count_over_65535", (counts > 65535).sum())
    total = int(counts.astype(np.int64).sum())
    add("all_equal_keys", len(codes) == 1 and total > TILE)
    if s["name"] == "de_bruijn":
        assert len(codes) == 2080 and (counts == 2).sum() == 2016 and (counts == 1).sum() == 64
        add("de_bruijn_2080")
    for name, t in (("total_tile_minus_1", TILE - 1), ("total_tile", TILE), ("total_tile_plus_1", TILE + 1),
                    ("total_two_tiles_minus_1", 2 * TILE - 1), ("total_two_tiles", 2 * TILE),
                    ("total_two_tiles_plus_1", 2 * TILE + 1)):
        add(name, total == t)
    for p, e in zip(s.get("index", []), got["index"]):
        min_freq, select_rate, tandem, repeat_rate = p
        add("select_0.4", select_rate == 0.4)
        add(f"min_freq_{min_freq}")
        add("tandem_0", tandem == 0)
        add("repeat_2_removes_codes", repeat_rate == 2.0 and len(e[3]) > 0)
        add("repeat_100", repeat_rate == 100.0)
        rep_freq = e[4]
        cap_codes = {}
        for r in reads:
            can, rev = ref.canonical(r, k)
            n = len(can)
            if n == 0:
                continue
            f = counts[np.searchsorted(codes, can)].astype(np.int64)
            if select_rate == 0.7 and n in (10, 90):
                m32 = int(np.float32(0.7) * np.float32(n))
                m64 = int(float(np.float32(0.7)) * n)
                add(f"select_0.7_n{n}_f32_{m32}", m32 == m64 + 1)
            mk = int(np.float32(select_rate) * np.float32(n))
            srt = np.sort(f)[::-1]
            add("read_all_equal_freq", srt[0] == srt[-1])
            add("tie_at_threshold", mk + 1 < n and srt[mk] == srt[mk + 1] and srt[0] != srt[-1])
            _, local = np.unique(can, return_counts=True)
            if tandem in (3, 100):
                add(f"tandem_{tandem}_code_{tandem}_times", (local == tandem).sum())
                add(f"tandem_{tandem}_code_{tandem + 1}_times", (local == tandem + 1).sum())
            kc, krev, kp, kf = ref.kept_positions(k, r, codes, counts, select_rate, tandem)
            ok = kf >= min_freq
            listed = ok & (kf <= rep_freq) & np.isin(kc, e[0])
            q = len(r) - kp - k
            add("reverse_offset_1", (listed & krev & (q == 1)).sum())
            add("reverse_offset_L_minus_k", (listed & krev & (kp == 0)).sum())
            for c, fr in zip(kc[ok].tolist(), kf[ok].tolist()):
                cap_codes[c] = (cap_codes.get(c, (0, 0))[0] + 1, fr)
        add("capacity_passes_frequency_cut", sum(1 for cap, fr in cap_codes.values() if cap <= rep_freq < fr))


def _pack(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    data = np.concatenate(reads).astype(np.uint8) if reads else np.zeros(0, np.uint8)
    return data, off


def store_set(store, s, got):
    n, codes, counts = s["name"], got["codes"], got["counts"]
    store[f"{n}/k"] = np.int64(s["k"])
    store[f"{n}/params"] = np.array(s.get("index", []), np.float64).reshape(-1, 4)
    st = ref.stats(codes, counts)
    store[f"{n}/stats"] = np.array([st[x] for x in ("n_distinct", "n_occurrences", "n_over15", "max_count")], np.int64)
    store[f"{n}/hist"] = ref.hist(counts, 32)
    data, off = _pack(s["reads"])
    if "recipe" in s:
        store[f"{n}/recipe"] = np.array([s["recipe"][0], str(s["recipe"][1])])
        store[f"{n}/reads_sum"] = np.array(ref.checksum(data) + ref.checksum(off))
    else:
        store[f"{n}/reads"], store[f"{n}/seq_off"] = data, off
    arrays = {"codes": codes, "counts": counts}
    for i, e in enumerate(got["index"]):
        arrays.update({f"idx{i}_codes": e[0], f"idx{i}_off": e[1], f"idx{i}_pos": e[2], f"idx{i}_rep": e[3]})
        store[f"{n}/idx{i}_scalars"] = np.array([len(e[0]), len(e[2]), len(e[3]), e[4]], np.int64)
    for name, a in arrays.items():
        if s["store"] == "whole":
            store[f"{n}/{name}"] = a
        else:
            store[f"{n}/{name}_sum"] = np.array(ref.checksum(a))


class Set:
    """One stored set: k, reads, params, stats, hist and expect(name), which is the stored array or, for a set stored
    as checksums, the restatement's array checked against the stored checksum."""

    def __init__(self, z, name):
        self.z, self.name = z, name
        self.k = int(z[f"{name}/k"])
        self.params = [(int(p[0]), float(p[1]), int(p[2]), float(p[3])) for p in z[f"{name}/params"]]
        self.stats = dict(zip(("n_distinct", "n_occurrences", "n_over15", "max_count"),
                              [int(x) for x in z[f"{name}/stats"]]))
        self.hist = z[f"{name}/hist"]
        if f"{name}/recipe" in z.files:
            kind, arg = z[f"{name}/recipe"]
            self.reads = from_recipe((str(kind), int(arg)), self.k)
            data, off = _pack(self.reads)
            assert ref.checksum(data) + ref.checksum(off) == str(z[f"{name}/reads_sum"]), f"{name}: reads differ"
        else:
            data, off = z[f"{name}/reads"], z[f"{name}/seq_off"]
            self.reads = [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        self.data, self.seq_off = _pack(self.reads)
        self.whole = f"{name}/codes" in z.files
        self._ref = None

    def scalars(self, i):
        return [int(x) for x in self.z[f"{self.name}/idx{i}_scalars"]]

    def restated(self):
        if self._ref is None:
            codes, counts = ref.count(self.k, self.reads)
            arrays = {"codes": codes, "counts": counts}
            for i, p in enumerate(self.params):
                e = ref.index(self.k, self.reads, codes, counts, *p)
                arrays.update({f"idx{i}_codes": e[0], f"idx{i}_off": e[1], f"idx{i}_pos": e[2], f"idx{i}_rep": e[3],
                               f"idx{i}_rep_freq": e[4]})
            self._ref = arrays
        return self._ref

    def expect(self, name):
        if self.whole:
            return self.z[f"{self.name}/{name}"]
        a = self.restated()[name]
        assert ref.checksum(a) == str(self.z[f"{self.name}/{name}_sum"]), f"{self.name}/{name}: restatement differs"
        return a


def load(path):
    z = np.load(path)
    return z, [Set(z, str(n)) for n in z["set_names"]]
