"""Regenerate tests/golden/phmm_exit_golden.npz: PairHMM testcases that pin the f32 pass's early
exit (csrc/phmm.hip phmm_stack, "Early exit") against rows whose probability mass GROWS, with the
outputs of the reference GKL kernels (oracle/_ref/libref_phmm.so, built from the reference tree by
`make ref`; AVX2 and AVX-512 engines must agree bit for bit). Seeds are fixed: a rerun reproduces
the file.

    python tests/golden/make_phmm_exit_golden.py

Every testcase is one read against one haplotype:
  prefix   60-75 rows whose base occurs nowhere in the haplotype, q = 6: the mass falls by about a
           factor 10 a row, to about 1e-32 of the initial 2^120 / haplen
  plateau  70-130 matching rows of ordinary qualities (q = 40, i, d in 40..45, c = 10): the mass stays
           where the prefix left it, far below MIN_ACCEPTED = 1e-28
  tail     trap: rows whose transitions out of a state sum to more than 1, so the mass grows back
           above MIN_ACCEPTED and the reference answers from its f32 result; control: ordinary rows
           (i, d in 40..45, c = 10), the mass stays and the reference falls back to f64
The growth regimes of a tail (GKL clamps pMM = 1 - (10^(-i/10) + 10^(-d/10)) at 0 and does not
renormalise; Y stays with row r's ph2pr[c_r] and leaves with 1 - ph2pr[c_{r+1}]):
  clamp   i, d of 0..3 with pMM = 0: pMM + pMX + pMY up to 2
  dalt    i = 0, d alternating 0 / 45
  yleak0  i = 45, d = 10, c alternating 0 / 40 (ph2pr[0] = 1: the gap mass does not decay along the row)
  yleak1  i = 45, d = 3, c alternating 1 / 40
mixtures of these within one tail, and growth rows interleaved with ordinary rows.

Classification. replay() restates the recurrence in float64 over the f32 table values of
oracle/phmm_oracle.c (phmm_oracle_ph2pr_f / phmm_oracle_m2m_f) and gives the crossing mass after
every row k in the kernel's form, sum_c [M nMM + (X + Y) nGAPM + M nMX + X nXX] with row k+1's
transitions. Thresholds used:
  WINDOW_BELOW = 2.5e-31  the replay is below it (100 x under the kernel's 0.25e-28, so the replay's
                          own rounding is irrelevant) ...
  WINDOW_ROWS  = 72       ... for at least this many consecutive rows (a stripe boundary falls every
                          64 stacked rows, so one lands inside wherever the testcase sits in a stack)
  WINDOW_ABOVE = 1e-35    and never below this inside that run (well clear of the f32 denormals)
  TRAP_F32     = 1e-24    a trap's reference f32 result is at least this (well clear of MIN_ACCEPTED)
A trap holds all four; a control holds the first three and the reference falls back (f32 < 1e-28).
These are conditions: a random draw that misses them is rejected and redrawn. main() asserts them
for the named cases, whose f32 results are given (C and D2 answer 2.6e-26 and 2.9e-26): for those a
trap is a testcase with the window whose reference result does not fall back.

Contents: the eight named cases (haplotype A x 300, prefix 66 x C, plateau 70, tails A, B1, B2, C,
D1, D2, control1, control2), case A against A x 473, 32 random traps and 16 random controls with
haplotypes of 300 or 473 columns: a homopolymer, or for half the draws a random string of two
letters without the prefix base, which the read follows from the haplotype's first column. Against
two letters the mass the prefix leaves sits on one diagonal instead of all of them, some 300 x
lower: such draws hold the control conditions but no trap of them reached TRAP_F32 within the
340-row limit, so every kept trap has a homopolymer and half of the controls have two letters.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "phmm_exit_golden.npz")
WINDOW_BELOW, WINDOW_ROWS, WINDOW_ABOVE, TRAP_F32 = 2.5e-31, 72, 1e-35, 1e-24
MIN_ACCEPTED = np.float32(1e-28)
N_TRAPS, N_CONTROLS = 32, 16
FIELDS = ("bases", "q", "i", "d", "c")

_tabs = None


def tables():
    """(ph2pr[128], m2m[...]) as the f32 values of oracle/phmm_oracle.c, held in float64."""
    global _tabs
    if _tabs is None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
        o = oracle_lib.oracle()
        o.phmm_oracle_ph2pr_f.restype = ctypes.c_float
        o.phmm_oracle_m2m_f.restype = ctypes.c_float
        ph = np.array([o.phmm_oracle_ph2pr_f(x) for x in range(128)], np.float64)
        m2m = np.array([o.phmm_oracle_m2m_f(k) for k in range(((127 * 128) >> 1) + 128)], np.float64)
        _tabs = ph, m2m
    return _tabs


def code(b):
    """ConvertChar: A0 C1 T2 G3 N4, every other byte 0."""
    t = np.zeros(256, np.uint8)
    for ch, v in zip(b"ACTGN", range(5)):
        t[ch] = v
    return t[np.frombuffer(b, np.uint8)]


def replay(read, hap):
    """Crossing mass after rows 0 .. R-2 of (bases, q, i, d, c) against hap, float64."""
    ph, m2m = tables()
    rb, hb = code(read[0]), code(hap)
    q, qi, qd, qc = (np.frombuffer(x, np.uint8).astype(np.int64) & 127 for x in read[1:])
    R, C = len(rb), len(hb)
    mn, mx = np.minimum(qi, qd), np.maximum(qi, qd)
    pMM, pMX, pMY, pXX = m2m[((mx * (mx + 1)) >> 1) + mn], ph[qi], ph[qd], ph[qc]
    pGAPM = np.float32(1.0) - ph[qc].astype(np.float32)  # the f32 one_minus value
    pGAPM = pGAPM.astype(np.float64)
    M, X, Y = np.zeros(C + 1), np.zeros(C + 1), np.full(C + 1, 2.0 ** 120 / C)
    cross = np.zeros(max(R - 1, 0))
    for r in range(R):
        match = (hb == rb[r]) | (hb == 4) | (rb[r] == 4)
        dist = np.where(match, 1.0 - ph[q[r]], ph[q[r]] / 3.0)
        Mn, Xn = np.zeros(C + 1), np.zeros(C + 1)
        Mn[1:] = (M[:-1] * pMM[r] + (X[:-1] + Y[:-1]) * pGAPM[r]) * dist
        Xn[1:] = M[1:] * pMX[r] + X[1:] * pXX[r]
        # Y[c] = M[c-1] pMY + Y[c-1] pYY, Y[0] = 0: a scan by doubling
        Yn = np.zeros(C + 1)
        Yn[1:] = Mn[:-1] * pMY[r]
        p, s = pXX[r], 1
        while s <= C:
            Yn[s:] = Yn[s:] + p * Yn[:-s]
            p, s = p * p, 2 * s
        M, X, Y = Mn, Xn, Yn
        if r + 1 < R:
            n = r + 1
            cross[r] = (M * (pMM[n] + pMX[n]) + (X + Y) * pGAPM[n] + X * pXX[n])[1:].sum()
    return cross


def window(cross):
    """The longest run of rows whose crossing mass is below WINDOW_BELOW: (first row, rows, smallest
    mass inside)."""
    best, k = (0, 0, 0.0), 0
    while k < len(cross):
        if cross[k] < WINDOW_BELOW:
            j = k
            while j < len(cross) and cross[j] < WINDOW_BELOW:
                j += 1
            if j - k > best[1]:
                best = (k, j - k, float(cross[k:j].min()))
            k = j
        else:
            k += 1
    return best


def has_window(cross):
    first, rows, low = window(cross)
    return rows >= WINDOW_ROWS and low >= WINDOW_ABOVE


def classify(read, hap, raw_f, floor=TRAP_F32):
    """'trap', 'control' or None from the replay and the reference's f32 result."""
    if not has_window(replay(read, hap)):
        return None
    if raw_f >= floor:
        return "trap"
    return "control" if raw_f < MIN_ACCEPTED else None


def rows(n, base, q, i, d, c):
    """n read rows; i, d, c a value or a sequence repeated over the rows."""
    cyc = lambda v: np.resize(np.atleast_1d(np.asarray(v, np.uint8)), n)  # noqa: E731
    return [np.full(n, base, np.uint8), cyc(q), cyc(i), cyc(d), cyc(c)]


def join(parts):
    return tuple(np.concatenate([p[k] for p in parts]).tobytes() for k in range(5))


NAMED_TAILS = (("A", 70, 0, 0, 10), ("B1", 90, 1, 1, 10), ("B2", 200, 2, 2, 10), ("C", 160, 0, (0, 45), 10),
               ("D1", 60, 45, 10, (0, 40)), ("D2", 60, 45, 3, (1, 40)), ("control1", 60, 45, 45, 10),
               ("control2", 60, 45, 3, 40))
NAMED_KIND = {"control1": "control", "control2": "control"}


def named_cases():
    out = []
    for name, g, i, d, c in NAMED_TAILS:
        read = join([rows(66, ord("C"), 6, 45, 45, 10), rows(70, ord("A"), 40, 45, 45, 10),
                     rows(g, ord("A"), 40, i, d, c)])
        out.append((name, NAMED_KIND.get(name, "trap"), read, b"A" * 300))
    out.append(("A_473", "trap", out[0][2], b"A" * 473))
    return out


def growth_rows(rng, n, regime):
    """(i, d, c) of n tail rows of one growth regime."""
    i, d, c = np.full(n, 45), np.full(n, 45), np.full(n, 10)
    k = np.arange(n)
    if regime == "clamp":
        lo, hi = [(0, 0), (0, 3), (1, 1), (1, 2), (2, 2), (3, 3), (0, 1)][int(rng.integers(0, 7))]
        i[:], d[:] = (lo, hi) if rng.random() < 0.5 else (hi, lo)
    elif regime == "dalt":
        i[:], d[:] = 0, np.where(k % 2 == 0, 0, 45)
    elif regime == "yleak0":
        d[:], c[:] = int(rng.integers(3, 12)), np.where(k % 2 == 0, 0, 40)
    elif regime == "yleak1":
        d[:], c[:] = int(rng.integers(1, 5)), np.where(k % 2 == 0, 1, int(rng.integers(30, 46)))
    else:
        raise ValueError(regime)
    return i, d, c


def ordinary_rows(rng, n):
    return rng.integers(40, 46, n), rng.integers(40, 46, n), np.full(n, 10)


def random_case(rng, want, two_letters):
    """One draw of the family: (read, hap). want: 'trap' or 'control' (its tail only ordinary rows);
    two_letters: the haplotype is a random string of two letters, else a homopolymer (A x 300, the
    named cases' haplotype, for a third of them)."""
    C = int(rng.choice([300, 473]))
    letters = b"ACGT"
    pre = letters[int(rng.integers(0, 4))]
    rest = [x for x in letters if x != pre]
    a = rest[int(rng.integers(0, 3))]
    if not two_letters and rng.random() < 1 / 3:
        C, a = 300, ord("A")
        pre = b"CGT"[int(rng.integers(0, 3))]
    if not two_letters:
        hap = bytes([a]) * C
        body = np.full(400, a, np.uint8)
    else:  # two letters; the read follows the haplotype from its first column
        b = [x for x in rest if x != a][int(rng.integers(0, 2))]
        hap = np.where(rng.random(C) < 0.5, a, b).astype(np.uint8).tobytes()
        body = np.resize(np.frombuffer(hap, np.uint8), 400)
    n_pre, n_pla = int(rng.integers(60, 76)), int(rng.integers(70, 131))
    n_tail = int(rng.integers(40, 121))
    n_tail = min(n_tail, (C - 10) - n_pre - n_pla, 340 - n_pre - n_pla)
    parts = [rows(n_pre, pre, 6, 45, 45, 10)]
    i, d, c = ordinary_rows(rng, n_pla)
    parts.append(rows(n_pla, 0, 40, i, d, c))
    if want == "control":
        i, d, c = ordinary_rows(rng, n_tail)
    else:
        regimes = ["clamp", "dalt", "yleak0", "yleak1"]
        shape = rng.choice(["one", "mixture", "interleaved"])
        if shape == "mixture":
            cuts = np.sort(rng.integers(1, n_tail, int(rng.integers(1, 3))))
            segs = np.diff(np.concatenate([[0], cuts, [n_tail]]))
            trip = [growth_rows(rng, int(s), regimes[int(rng.integers(0, 4))]) for s in segs if s > 0]
            i, d, c = (np.concatenate([t[k] for t in trip]) for k in range(3))
        else:
            i, d, c = growth_rows(rng, n_tail, regimes[int(rng.integers(0, 4))])
            if shape == "interleaved":  # every 2nd to 4th row (pair of rows for the alternating regimes) ordinary
                oi, od, oc = ordinary_rows(rng, n_tail)
                keep = (np.arange(n_tail) // 2) % int(rng.integers(2, 5)) != 0
                i, d, c = np.where(keep, i, oi), np.where(keep, d, od), np.where(keep, c, oc)
    parts.append(rows(n_tail, 0, int(rng.integers(30, 41)), i, d, c))
    read = list(join(parts))
    bases = np.frombuffer(read[0], np.uint8).copy()
    bases[n_pre:] = body[n_pre:len(bases)]
    read[0] = bases.tobytes()
    return tuple(read), hap


def ref_lib():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    return oracle_lib.ref_phmm()


def ref_run(lib, pairs):
    """(final, raw f32, raw f64) of the reference for [(read, hap)], both engines checked equal."""
    sys.path.insert(0, ROOT)
    from genomicsbench_palisade_amd._tc import TestcaseArray
    ta = TestcaseArray.from_pairs(pairs)
    res = {}
    for eng in (256, 512):
        out, rf, rd = np.zeros(ta.n), np.zeros(ta.n, np.float32), np.zeros(ta.n)
        lib.ref_phmm_batch(ctypes.addressof(ta.arr), ta.n, out.ctypes.data, rf.ctypes.data, rd.ctypes.data, eng, 8)
        res[eng] = (out, rf, rd)
    for a, b in zip(res[256], res[512]):
        assert (a.view(np.uint8) == b.view(np.uint8)).all(), "AVX2 and AVX-512 disagree"
    return res[256]


def load(path=OUT):
    """The fixture as a list of dicts: name, kind, named, read (5 byte strings), hap, final, raw_f, raw_d."""
    z = np.load(path)
    ro = np.concatenate([[0], np.cumsum(z["read_len"])])
    ho = np.concatenate([[0], np.cumsum(z["hap_len"])])
    cases = []
    for k in range(len(z["read_len"])):
        read = tuple(z["read_" + f][ro[k]:ro[k + 1]].tobytes() for f in FIELDS)
        cases.append({"name": str(z["name"][k]), "kind": str(z["kind"][k]), "named": bool(z["named"][k]),
                      "read": read, "hap": z["hap_bases"][ho[k]:ho[k + 1]].tobytes(),
                      "final": z["final"][k], "raw_f": z["raw_f"][k], "raw_d": z["raw_d"][k]})
    return cases


def main():
    lib = ref_lib()
    if lib is None:
        sys.exit("oracle/_ref/libref_phmm.so not built: run `make ref` where the reference tree exists")
    cases = []  # (name, kind, read, hap)
    named = named_cases()
    res = ref_run(lib, [(r, h) for _, _, r, h in named])
    for k, (name, kind, read, hap) in enumerate(named):
        first, nrows, low = window(replay(read, hap))
        print(f"{name:9s} {kind:7s} R {len(read[0])} C {len(hap)} f32 {res[1][k]:.3e} falls back "
              f"{bool(res[1][k] < MIN_ACCEPTED)} window rows {first}-{first + nrows - 1} low {low:.2e}")
        assert classify(read, hap, res[1][k], floor=MIN_ACCEPTED) == kind, name
        cases.append((name, kind, read, hap))
    rng = np.random.default_rng(20261)
    for want, count in (("trap", N_TRAPS), ("control", N_CONTROLS)):
        got = drawn = 0
        while got < count:
            read, hap = random_case(rng, want, two_letters=rng.random() < 0.5)
            drawn += 1
            if len(read[0]) >= len(hap):
                continue
            rf = ref_run(lib, [(read, hap)])[1][0]
            if classify(read, hap, rf) != want:
                continue
            cases.append((f"{want}{got:02d}", want, read, hap))
            got += 1
        print(f"{want}: {count} of {drawn} draws kept")
    res = ref_run(lib, [(r, h) for _, _, r, h in cases])
    out = {"name": np.array([c[0] for c in cases]), "kind": np.array([c[1] for c in cases]),
           "named": np.array([k < len(named) for k in range(len(cases))]),
           "read_len": np.array([len(c[2][0]) for c in cases], np.int32),
           "hap_len": np.array([len(c[3]) for c in cases], np.int32),
           "hap_bases": np.frombuffer(b"".join(c[3] for c in cases), np.uint8),
           "final": res[0], "raw_f": res[1], "raw_d": res[2]}
    for k, f in enumerate(FIELDS):
        out["read_" + f] = np.frombuffer(b"".join(c[2][k] for c in cases), np.uint8)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(cases)} testcases, {os.path.getsize(OUT)} bytes; longest read {out['read_len'].max()}")


if __name__ == "__main__":
    main()
