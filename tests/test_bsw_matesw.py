"""Mate rescue (gb_bsw_pestat, gb_bsw_mate_rescue; csrc/bsw_matesw.hip) against bwa's mem_pestat and the rescue
loop of mem_sam_pe around mem_matesw (tools/bwa/bwamem_pair.c): the results recorded live in
tests/golden/bsw_matesw_golden.npz and, for mem_pestat when the reference tree is present, fresh region sets
through the generator's live helper. Every field of every region is compared bit for bit and in order, avg and
std by their bits; there is no tolerance anywhere."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from genomicsbench_palisade_amd import bsw

sys.path.insert(0, GOLDEN)
import make_bsw_matesw_golden as mg  # noqa: E402  (the fixture's generator: live helper and Python restatement)

GB_ERR_ARG = -1
FIXTURE = os.path.join(GOLDEN, "bsw_matesw_golden.npz")


def regs_array(fields, n):
    """ALNREG_DTYPE records from the fixture's compact fields (re stored as a length)."""
    out = np.zeros(n, bsw.ALNREG_DTYPE)
    for f in mg.FIELDS:
        out[f] = fields[f]
    out["re"] = out["rb"] + fields["re"]
    return out


def pack_pairs(pairs):
    """(qbuf, idq, lens, reg_off, regs) for the generator's pairs ([read1, read2], [list1, list2])."""
    reads = [r for rs, _ in pairs for r in rs]
    lists = [x for _, ls in pairs for x in ls]
    lens = np.array([len(x) for x in reads], np.int32)
    idq = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])[:-1]
    qbuf = np.concatenate(reads).astype(np.uint8)
    reg_off = np.concatenate([[0], np.cumsum([len(x) for x in lists], dtype=np.int64)]).astype(np.int64)
    flat = [g for x in lists for g in x]
    regs = np.zeros(len(flat), bsw.ALNREG_DTYPE)
    for f in mg.FIELDS:
        regs[f] = [g[f] for g in flat]
    return qbuf, idq, lens, reg_off, regs


def pes_array(ints, dbls):
    pes = np.zeros(4, bsw.PESTAT_DTYPE)
    pes["low"], pes["high"], pes["failed"] = ints[:, 0], ints[:, 1], ints[:, 2]
    pes["avg"], pes["std"] = dbls[:, 0], dbls[:, 1]
    return pes


class Group:
    """One group of the fixture: the call's arrays, its pes, and what the live reference returned."""

    def __init__(self, fx, g, opt):
        self.name, self.opt = g, opt
        self.params = bsw.default_params(mat=bsw.fill_scmat(opt.a, opt.b))
        self.lens = fx[g + "_lens"].astype(np.int32)
        self.qbuf = fx[g + "_qbuf"]
        self.idq = np.concatenate([[0], np.cumsum(self.lens, dtype=np.int64)])[:-1]
        pick = lambda p: {f: fx["%s_%s_%s" % (g, p, f)] for f in mg.FIELDS}  # noqa: E731
        self.n_in, self.n_exp = fx[g + "_in_n"].astype(np.int64), fx[g + "_out_n"].astype(np.int64)
        self.reg_off = np.concatenate([[0], np.cumsum(self.n_in)]).astype(np.int64)
        self.exp_off = np.concatenate([[0], np.cumsum(self.n_exp)]).astype(np.int64)
        self.regs = regs_array(pick("in"), int(self.reg_off[-1]))
        self.exp = regs_array(pick("out"), int(self.exp_off[-1]))
        self.n_sw = fx[g + "_n_sw"]
        self.pes = pes_array(fx[g + "_pes_i"], fx[g + "_pes_d"])
        self.pestat = pes_array(fx[g + "_pestat_i"], fx[g + "_pestat_d"])
        self.n_pairs = len(self.lens) // 2

    def call(self, pairs=None):
        """The call's arrays for the pairs given (all by default), in that order."""
        if pairs is None:
            return self.qbuf, self.idq, self.lens, self.reg_off, self.regs
        reads = np.stack([2 * np.asarray(pairs), 2 * np.asarray(pairs) + 1], 1).ravel()
        lens = self.lens[reads]
        idq = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])[:-1]
        qbuf = np.concatenate([self.qbuf[self.idq[r]:self.idq[r] + self.lens[r]] for r in reads])
        idx = np.concatenate([np.arange(self.reg_off[r], self.reg_off[r + 1]) for r in reads]).astype(np.int64)
        return qbuf, idq, lens, np.concatenate([[0], np.cumsum(self.n_in[reads])]).astype(np.int64), self.regs[idx]

    def expected(self, pairs=None):
        """(n_out per read, the regions, n_sw) of the live reference for the pairs given."""
        if pairs is None:
            return self.n_exp, self.exp, self.n_sw
        reads = np.stack([2 * np.asarray(pairs), 2 * np.asarray(pairs) + 1], 1).ravel()
        idx = np.concatenate([np.arange(self.exp_off[r], self.exp_off[r + 1]) for r in reads]).astype(np.int64)
        return self.n_exp[reads], self.exp[idx], self.n_sw[np.asarray(pairs)]


class Golden:
    def __init__(self):
        self.fx = fx = dict(np.load(FIXTURE))
        ref = np.load(os.path.join(GOLDEN, "bsw_mkchain_golden.npz"))
        self.codes, self.contig_end = ref["ref_codes"], ref["contig_end"]
        self.l_pac = len(self.codes)
        self.names = [str(g) for g in fx["group_names"]]
        self._groups = {}

    def opt(self, g):
        row = self.fx["group_opts"][self.names.index(g)]
        return bsw.pe_opt(**{str(k): v for k, v in zip(self.fx["opt_names"], row)})

    def group(self, g):
        """Built once per group and shared; nobody writes to it."""
        if g not in self._groups:
            self._groups[g] = Group(self.fx, g, self.opt(g))
        return self._groups[g]

    def pestat_case(self, c):
        fx = self.fx
        n = fx["ps%d_n" % c].astype(np.int64)
        regs = np.zeros(int(n.sum()), bsw.ALNREG_DTYPE)
        for f in ("rb", "qb", "qe", "score", "rid"):
            regs[f] = fx["ps%d_%s" % (c, f)]
        regs["re"], regs["seedcov"] = regs["rb"] + 100, 50
        return np.concatenate([[0], np.cumsum(n)]).astype(np.int64), regs, \
            pes_array(fx["ps%d_pestat_i" % c], fx["ps%d_pestat_d" % c])


@pytest.fixture(scope="module")
def golden():
    return Golden()


@pytest.fixture(scope="module")
def ref(golden):
    r = bsw.Ref.from_codes(golden.codes)
    yield r
    r.close()


def same_pes(a, b):
    return all((a[f] == b[f]).all() for f in ("low", "high", "failed")) and \
        all((a[f].view(np.uint64) == b[f].view(np.uint64)).all() for f in ("avg", "std"))


def assert_same(res, exp, what):
    n_exp, regs_exp, n_sw = exp
    assert res["status"] == 0
    bad = np.flatnonzero(res["n_out"] != n_exp)
    assert not len(bad), f"{what}: list lengths differ on {len(bad)} reads; first {bad[0]}: {res['n_out'][bad[0]]} != {n_exp[bad[0]]}"
    off = np.concatenate([[0], np.cumsum(n_exp)])[:-1]
    assert (res["out_off"] == off).all() and res["out_used"] == n_exp.sum(), what
    got = res["regs"][:int(n_exp.sum())]
    read_of = np.repeat(np.arange(len(n_exp)), n_exp)
    for f in bsw.ALNREG_FIELDS:
        a, b = got[f], regs_exp[f]
        if f == "frac_rep":
            a, b = a.view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert not len(bad), f"{what}: {f} differs on {len(bad)} regions; first in read {read_of[bad[0]]}: {a[bad[0]]} != {b[bad[0]]}"
    bad = np.flatnonzero(res["n_sw"] != n_sw)
    assert not len(bad), f"{what}: n_sw differs on {len(bad)} pairs; first {bad[0]}: {res['n_sw'][bad[0]]} != {n_sw[bad[0]]}"


def rescue(golden, ref, g, pairs=None, **kw):
    G = golden.group(g)
    return bsw.mate_rescue_raw(ref, G.pes, *G.call(pairs), opt=G.opt, params=G.params, contig_end=golden.contig_end, **kw)


# ---------------------------------------------------------------- CPU

def test_fixture_labels(golden):
    """The live reference alone meets the label minima and the conditions, and the groups are the generator's."""
    fx = golden.fx
    total = dict(zip([str(x) for x in fx["label_names"]], fx["label_counts"].sum(axis=0).tolist()))
    assert list(total) == list(mg.LABELS)
    for k, v in total.items():
        assert v >= max(int(fx["label_min"]), 5), (k, total)
    assert golden.names == list(mg.GROUPS)
    for g, (kw, _, gp) in mg.GROUPS.items():
        o = golden.opt(g)
        for k, v in mg.opts(**kw).items():
            assert getattr(o, k) == (np.float32(v) if isinstance(v, float) else v), (g, k)
        if gp != "live":
            G = golden.group(g)
            assert [(int(p["low"]), int(p["high"]), int(p["failed"])) for p in G.pes] == [tuple(x) for x in gp]
    n_pairs, n_dp, n_gain, rounds = [int(x) for x in fx["conditions"]]
    assert 1400 <= n_pairs <= 1700 and 3 * n_dp >= n_pairs and 10 * n_gain >= n_pairs and rounds >= 3
    w = set(fx["windows"].tolist())
    assert {10, 15, 16, 17, 19, 255, 256, 257} <= w and 16000 < max(w) <= bsw.LOCAL_MAX_TLEN
    assert set(mg.MATE_LENS) <= set(fx["mate_lens_ran"].tolist())  # mates of these lengths went through the DP
    assert os.path.getsize(FIXTURE) <= 600 * 1024


def test_pestat_equals_fixture(golden):
    """low, high, failed equal and avg, std bit-equal: every group's regions and the synthetic cases."""
    for g in golden.names:
        G = golden.group(g)
        assert same_pes(bsw.pestat(golden.l_pac, G.reg_off, G.regs, opt=G.opt), G.pestat), g
    assert int(golden.fx["n_pestat_cases"]) >= 10
    for c in range(int(golden.fx["n_pestat_cases"])):
        reg_off, regs, exp = golden.pestat_case(c)
        assert same_pes(bsw.pestat(golden.l_pac, reg_off, regs), exp), c


def test_pestat_refusals(golden):
    G = golden.group("wide")
    keep = np.full(4, 7, np.int32).repeat(8).view(bsw.PESTAT_DTYPE)
    for args, kw, text in (((golden.l_pac, G.reg_off[:-1], G.regs), {}, "even"),
                           ((golden.l_pac, G.reg_off + 1, G.regs), {}, "reg_off[0]"),
                           ((golden.l_pac, np.array([0, 2, 1], np.int64), G.regs), {}, "read 1: reg_off decreases"),
                           ((0, G.reg_off, G.regs), {}, "l_pac"),
                           ((golden.l_pac, G.reg_off, G.regs), dict(opt=bsw.pe_opt(mask_level=float("nan"))), "mask_level")):
        pes = keep.copy()
        st, _ = bsw.pestat_raw(*args, pes=pes, **kw)
        assert st == GB_ERR_ARG and text in bsw.lib().gb_last_error().decode(), (text, bsw.lib().gb_last_error())
        assert pes.tobytes() == keep.tobytes(), text
    assert (bsw.pestat(golden.l_pac, np.zeros(1, np.int64), np.zeros(0, bsw.ALNREG_DTYPE))["failed"] == 1).all()


def test_default_opt():
    o = bsw.pe_opt()
    got = {k: getattr(o, k) for k, _ in bsw.PeOpt._fields_}
    assert got == {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in mg.DEFAULTS.items()}
    assert list(got.values()) == [1, 4, 6, 1, 6, 1, 19, 10000, 17, 50, 10000, 0.5, float(np.float32(0.95))]
    assert bsw.PESTAT_DTYPE.itemsize == 32 and bsw.PESTAT_DTYPE.fields["avg"][1] == 16


def _one(golden, **kw):
    """A pair whose first read has one region and whose second has none: the base of every refusal."""
    s = 5000
    r1, r2 = golden.codes[s:s + 100].copy(), golden.codes[s + 300:s + 400].copy()
    a = mg.rg.new_reg(rb=s, re=s + 100, qb=0, qe=100, score=100, truesc=100, seedcov=50, seedlen0=19, n_comp=1)
    a.update(kw)
    return pack_pairs([([r1, r2], [[a], []])])


def test_refusals(golden, ref):
    """Every refusal of include/gb_bsw.h: GB_ERR_ARG before any device work, the read or the orientation named,
    nothing written."""
    L = golden.l_pac
    fr = pes_array(np.array([[0, 0, 1], [100, 400, 0], [0, 0, 1], [0, 0, 1]]), np.zeros((4, 2)))
    ok = _one(golden)

    def refused(args, text, pes=fr, **kw):
        kw.setdefault("contig_end", golden.contig_end)
        res = bsw.mate_rescue_raw(ref, pes, *args, **kw)
        assert res["status"] == GB_ERR_ARG, (text, res["status"])
        assert text in bsw.lib().gb_last_error().decode(), (text, bsw.lib().gb_last_error())
        assert not res["regs"].view(np.uint8).any() and (res["n_out"] == -1).all() and (res["out_off"] == -1).all(), text
        assert (res["n_sw"] == -1).all() and res["out_used"] == -1, text

    q, idq, lens, off, regs = ok
    refused((q, idq, lens, np.array([1, 2, 2], np.int64), regs), "reg_off[0]")
    refused((q, idq, lens, np.array([0, 1, 0], np.int64), regs), "read 1: reg_off decreases")
    refused((q, idq, lens, np.array([0, 1, 1 << 31], np.int64), regs), "2^31", out_cap=8)
    refused((q, idq, np.array([0, 100], np.int32), off, regs), "read 0: l_query = 0")
    refused((q, idq, np.array([100, 256], np.int32), off, regs), "read 1: l_query = 256")
    refused((q[:150], idq, lens, off, regs), "read 1 has its query outside")
    for kw, text in ((dict(qb=-1), "[qb, qe)"), (dict(qb=50, qe=50), "[qb, qe)"), (dict(qe=101), "[qb, qe)"),
                     (dict(rb=-1), "[rb, re)"), (dict(rb=5300, re=5300), "[rb, re)"), (dict(re=2 * L + 1), "[rb, re)"),
                     (dict(rb=L - 10, re=L + 10), "[rb, re)"), (dict(rid=-1), "rid"), (dict(rid=3), "rid"),
                     (dict(score=0), "score"), (dict(seedcov=0), "seedcov"), (dict(sub=-1), "sub"), (dict(csub=-1), "csub"),
                     (dict(sub_n=-1), "sub_n"), (dict(w=-1), "w = -1"), (dict(w=1 << 28), "w = ")):
        refused(_one(golden, **kw), "read 0 region 0")
        refused(_one(golden, **kw), text)
    for kw, text in ((dict(min_seed_len=0), "min_seed_len"), (dict(max_matesw=-1), "max_matesw"),
                     (dict(pen_unpaired=-1), "pen_unpaired"), (dict(a=0), "a = 0"), (dict(a=4000), "16 bits"),
                     (dict(max_chain_gap=-1), "max_chain_gap"), (dict(mask_level_redun=float("inf")), "mask_level_redun"),
                     (dict(o_del=-1), "gap penalties"), (dict(o_ins=32768), "gap penalties"),
                     (dict(o_del=300), "read 1 would be aligned with KSW_XBYTE and gap"),
                     (dict(a=2, b=60), "read 1 would be aligned with KSW_XBYTE and l_query")):
        o = bsw.pe_opt(**kw)
        refused(ok, text, opt=o, params=bsw.default_params(mat=bsw.fill_scmat(2, 60)) if "b" in kw else None)
    refused(ok, "scoring matrix", params=bsw.default_params(mat=np.full(25, -1, np.int8)))
    for row, text in (([-1, 400, 0], "orientation 1: low = -1"), ([400, 399, 0], "orientation 1: low = 400, high = 399"),
                      ([100, 100 + bsw.LOCAL_MAX_TLEN - 99, 0], "orientation 1: a window")):
        refused(ok, text, pes=pes_array(np.array([[0, 0, 1], row, [0, 0, 1], [0, 0, 1]]), np.zeros((4, 2))))
    refused(ok, "n_contigs", n_contigs=0)
    refused(ok, "contig_end[1] does not increase", contig_end=np.array([100, 100, L], np.int64))
    refused(ok, "contig_end ends at", contig_end=np.array([100, 200, L - 1], np.int64))
    # a failed orientation's bounds are not read, and a window just inside the bound is accepted by the checks
    bad_failed = pes_array(np.array([[-5, -9, 1]] * 4), np.zeros((4, 2)))
    res = bsw.mate_rescue_raw(ref, bad_failed, *ok, contig_end=golden.contig_end)
    assert res["status"] == 0 and res["n_out"].tolist() == [1, 0] and res["n_sw"].tolist() == [0]


def test_capacity_and_no_device(golden, ref):
    """With every orientation failed nothing is aligned and no device is touched: the lists come back as they
    went in. The short-capacity contract is gb_bsw_chain2aln's."""
    G = golden.group("fr_only")
    none = pes_array(np.array([[0, 0, 1]] * 4), np.zeros((4, 2)))
    args = G.call()
    res = bsw.mate_rescue_raw(ref, none, *args, opt=G.opt, contig_end=golden.contig_end)
    assert res["status"] == 0 and (res["n_out"] == G.n_in).all() and (res["n_sw"] == 0).all()
    assert res["regs"][:len(G.regs)].tobytes() == G.regs.tobytes() and res["out_used"] == len(G.regs)
    assert (res["out_off"] == G.reg_off[:-1]).all()
    assert bsw.mate_rescue_timing() == (0.0, 0.0, 0.0, bsw.mate_rescue_timing()[3], 0, 0)
    short = bsw.mate_rescue_raw(ref, none, *args, opt=G.opt, contig_end=golden.contig_end, out_cap=len(G.regs) - 1)
    assert short["status"] == GB_ERR_ARG and "out_cap" in bsw.lib().gb_last_error().decode()
    assert short["out_used"] == len(G.regs) and (short["n_out"] == G.n_in).all() and (short["out_off"] == G.reg_off[:-1]).all()
    assert not short["regs"].view(np.uint8).any()
    exact = bsw.mate_rescue_raw(ref, none, *args, opt=G.opt, contig_end=golden.contig_end, out_cap=len(G.regs))
    assert exact["status"] == 0 and exact["regs"].tobytes() == G.regs.tobytes()
    # max_matesw = 0: no anchor, whatever pes says
    res = bsw.mate_rescue_raw(ref, G.pes, *args, opt=bsw.pe_opt(max_matesw=0), contig_end=golden.contig_end, want_n_sw=False)
    assert res["status"] == 0 and res["regs"][:len(G.regs)].tobytes() == G.regs.tobytes() and (res["n_sw"] == -1).all()


def test_no_pairs(ref):
    e = np.zeros(0, np.int64)
    res = bsw.mate_rescue_raw(ref, np.zeros(4, bsw.PESTAT_DTYPE), np.zeros(0, np.uint8), e, np.zeros(0, np.int32),
                              np.zeros(1, np.int64), np.zeros(0, bsw.ALNREG_DTYPE))
    assert res["status"] == 0 and res["out_used"] == 0 and len(res["n_out"]) == 0


def test_bad_thread_count(golden, ref, monkeypatch):
    monkeypatch.setenv("GB_BSW_MATESW_THREADS", "0")
    res = rescue(golden, ref, "wide")
    assert res["status"] == GB_ERR_ARG and "GB_BSW_MATESW_THREADS" in bsw.lib().gb_last_error().decode()
    assert not res["regs"].view(np.uint8).any()


@pytest.mark.skipif(not mg.mk.available(), reason="needs the reference tree and oracle/_ref (make ref)")
def test_pestat_live_fuzz(golden):
    """Fresh synthetic region sets through live mem_pestat."""
    contigs, _ = mg.mk.make_reference()
    live = mg.mk.LiveBwa(contigs)
    try:
        lp = mg.LivePair(live)
        rng = np.random.default_rng(20261020)
        for kind in ("normal", "small", "tails", "ratio", "fr_only", "tails"):
            lists = mg.make_pestat_case(rng, golden.l_pac, golden.contig_end, kind, 300)
            exp = lp.pestat(mg.opts(), lists)
            _, _, _, reg_off, regs = pack_pairs([([np.zeros(1, np.uint8)] * 2, [lists[2 * p], lists[2 * p + 1]])
                                                 for p in range(len(lists) // 2)])
            got = bsw.pestat(golden.l_pac, reg_off, regs)
            assert same_pes(got, pes_array(*mg.pes_array(exp))), kind
    finally:
        live.close()


@pytest.mark.skipif(shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc") or os.path.exists("/dev/kfd"),
                    reason="needs make and hipcc, and runs on machines without a GPU only")
def test_matesw_sanitize():
    """`make matesw-sanitize`: the host bookkeeping under the address and undefined-behaviour sanitizers, in a
    stand-alone program on the CPU, its alignments supplied by a table."""
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run(["make", "-s", "matesw-sanitize"], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def results(golden, ref):
    """Every group once through the device path, shared by the tests that compare against it."""
    return {g: rescue(golden, ref, g) for g in golden.names}


@pytest.mark.gpu
def test_equals_fixture(golden, results):
    """Every group: every field of every region in the reference's order, and n_sw."""
    for g in golden.names:
        assert_same(results[g], golden.group(g).expected(), g)


@pytest.mark.gpu
def test_timing(golden, ref):
    G = golden.group("open")
    assert_same(rescue(golden, ref, "open"), G.expected(), "open")
    fetch, dp, region, host, rounds, requests = bsw.mate_rescue_timing()
    assert fetch > 0 and dp > 0 and region > 0 and host > 0 and rounds >= 3 and requests >= G.n_sw.sum()


@pytest.mark.gpu
def test_chunked(golden, ref, results, monkeypatch):
    """Five requests per chunk: many chunks per round, the same results."""
    monkeypatch.setenv("GB_BSW_MATESW_CHUNK", "5")
    for g in ("open", "o_ins0", "wide", "min_seed_len"):
        res = rescue(golden, ref, g)
        assert res["regs"].tobytes() == results[g]["regs"].tobytes() and (res["n_sw"] == results[g]["n_sw"]).all(), g
        assert_same(res, golden.group(g).expected(), g + " chunked")


@pytest.mark.gpu
def test_threads(golden, ref, results, monkeypatch):
    """1 and several host threads give the same arrays (the group has more than 256 tasks per round)."""
    assert (golden.group("open").n_in > 0).sum() > 256
    for n in ("1", "5"):
        monkeypatch.setenv("GB_BSW_MATESW_THREADS", n)
        res = rescue(golden, ref, "open")
        assert res["regs"].tobytes() == results["open"]["regs"].tobytes(), n
        assert (res["n_out"] == results["open"]["n_out"]).all() and (res["n_sw"] == results["open"]["n_sw"]).all(), n


@pytest.mark.gpu
def test_permuted_and_split(golden, ref):
    """The pairs in another order, and the call cut in two: the same per-pair results."""
    G = golden.group("open")
    perm = np.random.default_rng(5).permutation(G.n_pairs)
    assert_same(rescue(golden, ref, "open", perm), G.expected(perm), "permuted")
    for part in (perm[:G.n_pairs // 3], perm[G.n_pairs // 3:]):
        assert_same(rescue(golden, ref, "open", part), G.expected(part), "split")


@pytest.mark.gpu
def test_smaller_call_after_larger(golden, ref):
    """The cached buffers of a large call serve a small one."""
    G = golden.group("open")
    assert_same(rescue(golden, ref, "open"), G.expected(), "large")
    few = np.array([3, 1, 4])
    assert_same(rescue(golden, ref, "open", few), G.expected(few), "small after large")
    assert_same(rescue(golden, ref, "default", few), golden.group("default").expected(few), "another group")


@pytest.mark.gpu
def test_capacity_after_rescue(golden, ref, results):
    """The exact total suffices; one slot less returns the count required, the offsets and the list lengths,
    and leaves the region buffer untouched."""
    G = golden.group("fr_only")
    total = int(G.n_exp.sum())
    assert total > len(G.regs)
    exact = rescue(golden, ref, "fr_only", out_cap=total)
    assert_same(exact, G.expected(), "exact capacity")
    short = rescue(golden, ref, "fr_only", out_cap=total - 1)
    assert short["status"] == GB_ERR_ARG and "out_cap" in bsw.lib().gb_last_error().decode()
    assert short["out_used"] == total and (short["n_out"] == G.n_exp).all() and (short["n_sw"] == G.n_sw).all()
    assert (short["out_off"] == exact["out_off"]).all() and not short["regs"].view(np.uint8).any()
    assert results["fr_only"]["out_used"] == total and len(results["fr_only"]["regs"]) > total


@pytest.mark.gpu
def test_single_contig_default(golden):
    """contig_end == NULL is one contig: a window is clipped at 0 and 2 l_pac only."""
    codes = golden.codes[:3000]
    r = bsw.Ref.from_codes(codes)
    try:
        a = mg.rg.new_reg(rb=1000, re=1100, qb=0, qe=100, score=100, truesc=100, seedcov=50, seedlen0=19, n_comp=1)
        mate = mg.mk._rc(codes[1250:1350])
        fr = pes_array(np.array([[0, 0, 1], [100, 400, 0], [0, 0, 1], [0, 0, 1]]), np.zeros((4, 2)))
        res = bsw.mate_rescue(r, fr, *pack_pairs([([codes[1000:1100], mate], [[a], []])]))
        assert res["n_out"].tolist() == [1, 1] and res["n_sw"].tolist() == [1]
        b = res["regs"][1]
        assert (b["rb"], b["re"], b["qb"], b["qe"], b["score"], b["secondary"], b["rid"]) == (6000 - 1350, 6000 - 1250, 0, 100, 100, -1, 0)
    finally:
        r.close()


def _write_cli_input(golden, tmp_path, g, pes_line):
    G = golden.group(g)
    q, idq, lens, off, regs = G.call()
    pac = tmp_path / "ref.pac"
    pac.write_bytes(bsw.pack_pac(golden.codes).tobytes() + (b"\0" if golden.l_pac % 4 == 0 else b"") + bytes([golden.l_pac % 4]))
    f = tmp_path / "pairs.txt"
    with open(f, "w") as fh:
        fh.write(pes_line + "\n")
        for r in range(len(lens)):
            fh.write("".join(str(int(c)) for c in q[idq[r]:idq[r] + lens[r]]) + f" {off[r + 1] - off[r]}\n")
            for x in regs[off[r]:off[r + 1]]:
                fh.write(" ".join(str(x[k]) for k in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov",
                                                      "seedlen0", "csub", "sub_n")) + " %.9g\n" % x["frac_rep"])
    regs = regs.copy()
    regs["sub"] = regs["n_comp"] = regs["is_alt"] = 0  # the text format has no column for them
    return pac, f, (q, idq, lens, off, regs)


EXE = os.path.join(ROOT, "genomicsbench_palisade_amd", "bin", "bsw")
COLS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary",
        "secondary_all", "seedlen0", "n_comp", "is_alt", "mapq")


def test_cli_refuses(golden, tmp_path):
    """bin/bsw -materescue: what it refuses before any device work."""
    pac, f, _ = _write_cli_input(golden, tmp_path, "wide", "pes auto")
    r = subprocess.run([EXE, "-materescue", str(f)], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"-pac" in r.stderr
    r = subprocess.run([EXE, "-materescue", "-finishregs", "-pac", str(pac), str(f)], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"excludes" in r.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text(open(f).read().split("\n", 1)[1])
    r = subprocess.run([EXE, "-materescue", "-pac", str(pac), str(bad)], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"pes" in r.stderr
    r = subprocess.run([EXE, "-materescue", "-pac", str(pac), str(f), "-maxmatesw", "-1"], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"max_matesw" in r.stderr


@pytest.mark.gpu
def test_cli_materescue(golden, ref, tmp_path):
    """bin/bsw -materescue on pairs written as text, against the library call on the same pairs."""
    contigs = ",".join(str(int(x)) for x in golden.contig_end)
    for g, pes_line, extra, kw in (("fr_only", "pes 0 0 1 100 400 0 0 0 1 0 0 1", [], {}),
                                   ("open", "pes 100 400 0 100 400 0 100 400 0 100 400 0", ["-maxmatesw", "2", "-unpaired", "3"],
                                    dict(max_matesw=2, pen_unpaired=3)),
                                   ("default", "pes auto", [], {})):
        pac, f, args = _write_cli_input(golden, tmp_path, g, pes_line)
        G = golden.group(g)
        pes = G.pes if "auto" not in pes_line else bsw.pestat(golden.l_pac, args[3], args[4])
        res = bsw.mate_rescue(ref, pes, *args, opt=bsw.pe_opt(**kw), contig_end=golden.contig_end)
        lines = ["\t".join([str(r)] + [str(res["regs"][res["out_off"][r] + k][c]) for c in COLS]) + "\n"
                 for r in range(len(args[2])) for k in range(res["n_out"][r])]
        got = subprocess.run([EXE, "-materescue", "-pac", str(pac), str(f), "-contigs", contigs] + extra, check=True,
                             capture_output=True, timeout=120, text=True)
        assert got.stdout == "".join(lines) and len(lines) > 100, g
        assert "Executed mate rescue" in got.stderr


@pytest.mark.gpu
def test_end_to_end_from_reads(golden, ref):
    """From bases to rescued mates through library calls alone: gb_fmi_search, gb_fmi_sa_entries,
    gb_bsw_seeds2chains, gb_bsw_chain2aln, gb_bsw_finish_regs stage 0, gb_bsw_pestat, gb_bsw_mate_rescue. The
    default group's pairs are read pairs whose recorded stage-0 regions are live mem_align1_core's and whose
    recorded result is live mem_pestat's and the rescue loop over live mem_matesw (see the generator)."""
    from genomicsbench_palisade_amd import fmi
    G = golden.group("default")
    mk = np.load(os.path.join(GOLDEN, "bsw_mkchain_golden.npz"))
    is_alt = mk["contig_is_alt"]
    n = len(G.lens)
    reads = np.full((n, int(G.lens.max())), 4, np.uint8)
    for r in range(n):
        reads[r, :G.lens[r]] = G.qbuf[G.idq[r]:G.idq[r] + G.lens[r]]
    idx = fmi.Index.build(golden.codes)
    rd = fmi.Reads(idx, reads, G.lens)
    rd.search(19)
    rd.sync()
    smems = rd.results()[0]
    rd.close()
    coords, counts = idx.sa_entries(smems, max_occ=500, mode=fmi.SA_COMPRESSED)
    idx.close()
    chains = bsw.seeds2chains(golden.l_pac, G.lens, bsw.mems_from_smems(smems, counts), coords,
                              contig_end=golden.contig_end, contig_is_alt=is_alt)
    c2a = bsw.chain2aln_csr(ref, G.qbuf, G.idq, G.lens, chains["read_chain_off"], chains["chain_seed_off"], chains["seeds"],
                            contig_end=golden.contig_end, want_raw=False)
    reg_off, regs = bsw.alnregs_from_chain2aln(c2a, chains)
    host_ref = bsw.Ref.from_codes(golden.codes)  # finish_regs reads a host copy, which chain2aln released on `ref`
    try:
        regs, n_out = bsw.finish_regs(host_ref, G.qbuf, G.idq, G.lens, reg_off, regs, stage=0, contig_is_alt=is_alt)
    finally:
        host_ref.close()
    keep = np.concatenate([np.arange(reg_off[r], reg_off[r] + n_out[r]) for r in range(n)]).astype(np.int64)
    regs0, off0 = regs[keep], np.concatenate([[0], np.cumsum(n_out, dtype=np.int64)])
    assert (n_out == G.n_in).all() and regs0.tobytes() == G.regs.tobytes()
    pes = bsw.pestat(golden.l_pac, off0, regs0)
    assert same_pes(pes, G.pestat)
    res = bsw.mate_rescue_raw(ref, pes, G.qbuf, G.idq, G.lens, off0, regs0, contig_end=golden.contig_end)
    assert_same(res, G.expected(), "end to end")
    assert (res["n_out"] > n_out).sum() > 20
