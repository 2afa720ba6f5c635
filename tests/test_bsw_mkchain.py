"""Chains from seeds (gb_bsw_seeds2chains, csrc/bsw_mkchain.hip) against bwa's mem_chain and mem_chain_flt
(tools/bwa/bwamem.c:251-385): the chains recorded live in tests/golden/bsw_mkchain_golden.npz and, when the
reference tree is present, fresh reads through the generator's live helper. Everything is compared array
by array and bit for bit (frac_rep by its bits); there is no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from genomicsbench_palisade_amd import bsw

sys.path.insert(0, GOLDEN)
import make_bsw_mkchain_golden as mk  # noqa: E402  (the fixture's generator: live helper and Python restatement)

GB_ERR_ARG = -1
MIN_LABELS = {"pos_tie": 200, "gt9": 100, "gt81": 20, "weight_tie3": 200, "kept1": 50, "kept2": 50, "dropped": 50,
              "skipped": 50, "contained": 50, "strand": 20, "alt_ovlp": 20}


class Inputs:
    """What one call takes: lens, mems (MEM_DTYPE), coords and the reference's tables."""

    def __init__(self, fx, lens, mems, coords):
        self.l_pac = len(fx["ref_codes"])
        self.contig_end, self.is_alt = fx["contig_end"], fx["contig_is_alt"]
        self.lens, self.mems, self.coords = np.asarray(lens, np.int32), mems, np.asarray(coords, np.int64)

    def run(self, raw=False, **kw):
        kw.setdefault("contig_end", self.contig_end)
        kw.setdefault("contig_is_alt", self.is_alt)
        l_pac = kw.pop("l_pac", self.l_pac)
        fn = bsw.seeds2chains_raw if raw else bsw.seeds2chains
        return fn(l_pac, kw.pop("lens", self.lens), kw.pop("mems", self.mems), kw.pop("coords", self.coords), **kw)

    def take(self, reads):
        """The same for a subset of the reads (increasing indices)."""
        reads = np.asarray(reads, np.int64)
        new = np.full(len(self.lens), -1, np.int64)
        new[reads] = np.arange(len(reads))
        keep = new[self.mems["read"]] >= 0
        mems = self.mems[keep].copy()
        mems["read"] = new[mems["read"]]
        off = np.concatenate([[0], np.cumsum(self.mems["n_coord"], dtype=np.int64)])
        idx = [np.arange(off[i], off[i + 1]) for i in np.flatnonzero(keep)]
        out = Inputs.__new__(Inputs)
        out.l_pac, out.contig_end, out.is_alt = self.l_pac, self.contig_end, self.is_alt
        out.lens, out.mems = self.lens[reads], mems
        out.coords = self.coords[np.concatenate(idx)] if idx else np.zeros(0, np.int64)
        return out


def _mems(fx, g):
    m = np.zeros(len(fx[g + "_in_m"]), bsw.MEM_DTYPE)
    for f in ("read", "m", "n", "n_coord", "s"):
        m[f] = fx["%s_in_%s" % (g, f)]
    return m


class Golden:
    def __init__(self):
        self.fx = fx = dict(np.load(os.path.join(GOLDEN, "bsw_mkchain_golden.npz")))
        self.groups = [str(g) for g in fx["group_names"]]
        self.all = Inputs(fx, fx["lens"], _mems(fx, "default"), fx["default_in_coords"])
        self.reads = [fx["reads"][r, :n] for r, n in enumerate(fx["lens"])]
        self._exp = {}

    def opt(self, g):
        row = self.fx["group_opts"][self.groups.index(g)]
        return bsw.chain_opt(**{str(k): v for k, v in zip(self.fx["opt_names"], row)})

    def inputs(self, g):
        sel = self.fx[g + "_reads"]
        if g != "default" and g + "_in_m" in self.fx:  # seeds of its own (another max_occ)
            return Inputs(self.fx, self.fx["lens"][sel], _mems(self.fx, g), self.fx[g + "_in_coords"])
        return self.all if g == "default" else self.all.take(sel)

    def expected(self, g, stage):
        """Computed once per (group, stage) and shared; nobody writes to it."""
        if (g, stage) not in self._exp:
            self._exp[g, stage] = mk.expected(self.fx, g, stage)
        return self._exp[g, stage]


@pytest.fixture(scope="module")
def golden():
    return Golden()


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setenv("GB_BSW_MKCHAIN_HOST", "1")


@pytest.fixture
def device(monkeypatch):
    monkeypatch.delenv("GB_BSW_MKCHAIN_HOST", raising=False)


def assert_same(res, exp, what):
    rco, cso, seeds, info = exp
    assert (res["read_chain_off"] == rco).all(), \
        f"{what}: chains per read differ at reads {np.flatnonzero(np.diff(res['read_chain_off']) != np.diff(rco))[:5]}"
    assert len(res["chain_seed_off"]) == len(cso) and (res["chain_seed_off"] == cso).all(), f"{what}: chain_seed_off"
    for f, v in info.items():
        got = res["info"][f]
        if f == "frac_rep":
            got, v = got.view(np.uint32), np.ascontiguousarray(v, np.float32).view(np.uint32)
        bad = np.flatnonzero(got != v)
        assert not len(bad), f"{what}: info.{f} differs on {len(bad)} chains; first {bad[0]}: {got[bad[0]]} != {v[bad[0]]}"
    for f, v in seeds.items():
        bad = np.flatnonzero(res["seeds"][f] != v)
        assert not len(bad), f"{what}: seeds.{f} differs on {len(bad)} seeds; first {bad[0]}"
    assert (res["seeds"]["score"] == res["seeds"]["len"]).all(), what


def check_groups(golden, what):
    for g in golden.groups:
        inp, opt = golden.inputs(g), golden.opt(g)
        for stage in (0, 1):
            assert_same(inp.run(opt=opt, stage=stage), golden.expected(g, stage), f"{what} {g} stage {stage}")


# ---------------------------------------------------------------- CPU

def test_fixture_is_consistent(golden):
    """The live reference alone meets the label counts, and the option groups are the issue's."""
    fx = golden.fx
    names = [str(x) for x in fx["label_names"]]
    counts = dict(zip(names, fx["labels"].sum(axis=0).tolist()))
    for k, v in MIN_LABELS.items():
        assert counts[k] >= v, counts
    assert golden.groups == list(mk.GROUPS)
    for g, kw in mk.GROUPS.items():
        o = golden.opt(g)
        for k, v in mk.opts(**kw).items():
            assert getattr(o, k) == (np.float32(v) if isinstance(v, float) else v), (g, k)
    lens = fx["lens"]
    assert lens.min() < 19 and lens.max() == 250 and len(lens) >= 1500
    nm = np.bincount(fx["default_in_read"], minlength=len(lens))
    assert ((nm == 0) & (lens >= 19)).sum() >= 10  # reads with no SMEM
    s, nc = fx["default_in_s"], fx["default_in_n_coord"]
    assert (s > 1000).any() and (nc[s > 1000] == 500).all()  # s > max_occ with step > 1
    assert os.path.getsize(os.path.join(GOLDEN, "bsw_mkchain_golden.npz")) <= 601912  # the largest fixture so far
    # a three-level tree and sorts that push
    per_read = np.diff(golden.expected("default", 0)[0])
    assert per_read.max() > 81 and (per_read > 34).sum() >= 20


def test_host_equals_fixture(golden, host):
    check_groups(golden, "host")
    # the last call was the last group's: every read took the host path and no kernel ran
    assert bsw.seeds2chains_timing() == (0.0, 0.0, 0.0, len(golden.fx[golden.groups[-1] + "_reads"]))


def test_default_opt():
    o = bsw.chain_opt()
    assert (o.w, o.max_chain_gap, o.max_occ, o.min_seed_len, o.min_chain_weight, o.max_chain_extend, o.mask_level,
            o.drop_ratio) == (100, 10000, 500, 19, 0, 1 << 30, 0.5, 0.5)


def _small(golden):
    """The first 40 reads that have SMEMs, plus two without."""
    nm = np.bincount(golden.fx["default_in_read"], minlength=len(golden.fx["lens"]))
    return golden.all.take(np.sort(np.concatenate([np.flatnonzero(nm > 0)[:40], np.flatnonzero(nm == 0)[:2]])))


def _edit(a, i, **kw):
    a = a.copy()
    for k, v in kw.items():
        a[k][i] = v
    return a


def _set(a, i, v):
    a = a.copy()
    a[i] = v
    return a


def test_refusals(golden, host):
    """Every refusal returns GB_ERR_ARG, names its item and writes nothing."""
    import genomicsbench_palisade_amd as gb
    sm = _small(golden)
    m, c, lens = sm.mems, sm.coords, sm.lens
    nm = np.bincount(m["read"], minlength=len(lens))
    r = int(np.flatnonzero((nm >= 2) & (np.arange(len(lens)) > len(lens) // 2))[0])  # a read in the middle
    k, kl = (int(x) for x in np.flatnonzero(m["read"] == r)[[0, -1]])  # its first and last SMEM
    c0 = int(m["n_coord"][:k].sum())
    long_lens = lens.copy()
    long_lens[r] = 800
    big_s = _edit(m, k, s=int(m["s"][k]) + 1) if m["n_coord"][k] < 500 else _edit(m, k, n_coord=499)
    cases = [
        (dict(mems=_edit(m, kl, read=r - 1)), f"SMEM {kl}"),
        (dict(mems=_edit(m, len(m) - 1, read=len(lens))), f"SMEM {len(m) - 1}"),
        (dict(mems=_edit(m, 0, read=-1)), "SMEM 0"),
        (dict(mems=_edit(m, k, m=-1)), f"SMEM {k} of read {r}"),
        (dict(mems=_edit(m, k, n=int(m["m"][k]) - 1)), f"SMEM {k} of read {r}"),
        (dict(mems=_edit(m, k, n=int(lens[r]))), f"SMEM {k} of read {r}"),
        (dict(mems=_edit(m, k, s=0)), f"SMEM {k} of read {r}"),
        (dict(mems=big_s), f"SMEM {k} of read {r}"),
        (dict(coords=c[:-1]), "n_coords"),
        (dict(coords=np.concatenate([c, [0]])), "n_coords"),
        (dict(coords=_set(c, c0, -1)), f"SMEM {k} of read {r}: coordinate {c0}"),
        (dict(coords=_set(c, c0, 2 * sm.l_pac)), f"SMEM {k} of read {r}: coordinate {c0}"),
        (dict(opt=bsw.chain_opt(max_occ=0)), "max_occ"),
        (dict(opt=bsw.chain_opt(w=-1)), "w = -1"),
        (dict(opt=bsw.chain_opt(max_chain_gap=-1)), "max_chain_gap"),
        (dict(opt=bsw.chain_opt(max_chain_extend=0)), "max_chain_extend"),
        (dict(opt=bsw.chain_opt(mask_level=float("nan"))), "mask_level"),
        (dict(opt=bsw.chain_opt(drop_ratio=float("inf"))), "drop_ratio"),
        (dict(contig_end=sm.contig_end[[0, 0, 2]]), "contig_end[1]"),
        (dict(contig_end=sm.contig_end[:2], contig_is_alt=sm.is_alt[:2]), "l_pac"),
        (dict(stage=2), "stage"),
        (dict(n_coords=1 << 31), f"{1 << 31} coordinates"),  # refused on the count, before coords is read
        (dict(n_coords=(1 << 31) + 5), f"{(1 << 31) + 5} coordinates"),
        (dict(lens=long_lens), f"read {r}"),  # mem_flt_chained_seeds would re-score
    ]
    for kw, name in cases:
        res = sm.run(raw=True, fill=0x5A, **kw)
        msg = gb.lib().gb_last_error().decode()
        assert res["status"] == GB_ERR_ARG, (name, res["status"])
        assert name in msg, (name, msg)
        for f in ("read_chain_off", "chain_seed_off", "seeds", "info"):
            assert (res[f].view(np.uint8) == 0x5A).all(), (name, f)
        assert res["chains_used"] == -1 and res["seeds_used"] == -1, name
    assert sm.run(raw=True)["status"] == 0


def test_mem_flt_chained_seeds_bound(golden, host):
    """min_l > MEM_SEEDSW_COEF * l_query in the reference's types: 5.5f * log(l_query) against
    0.05f * l_query, or 1.1f * min_chain_weight. A read without SMEMs or below min_seed_len is never refused."""
    f32, f64 = np.float32, np.float64
    L = np.arange(19, 2000)
    rhs = (f32(0.05) * L.astype(f32)).astype(f64)
    ok_log = f64(f32(5.5)) * np.log(L.astype(f64)) > rhs
    ok_mcw = f64(f32(1.1) * f32(40)) > rhs
    one = Inputs(golden.fx, [30], np.array([(0, 0, 18, 1, 1)], bsw.MEM_DTYPE), [5])
    for ok, opt in ((ok_log, bsw.chain_opt()), (ok_mcw, bsw.chain_opt(min_chain_weight=40))):
        last = int(L[np.flatnonzero(ok)[-1]])
        assert ok[:last - 19 + 1].all() and 700 < last < 900  # one threshold
        assert one.run(raw=True, lens=[last], opt=opt)["status"] == 0
        assert one.run(raw=True, lens=[last + 1], opt=opt)["status"] == GB_ERR_ARG
    none = Inputs(golden.fx, [5000, 10], np.zeros(0, bsw.MEM_DTYPE), [])
    assert none.run(raw=True)["status"] == 0


def test_cap_protocol(golden, host):
    sm = _small(golden)
    full = sm.run()
    nc, ns = len(full["info"]), len(full["seeds"])
    assert 0 < nc < ns <= len(sm.coords)
    exact = sm.run(raw=True, chain_cap=nc, seed_cap=ns)
    assert exact["status"] == 0 and (exact["seeds"] == full["seeds"]).all() and (exact["info"] == full["info"]).all()
    for ccap, scap in ((nc, ns - 1), (nc - 1, ns), (0, 0)):
        res = sm.run(raw=True, chain_cap=ccap, seed_cap=scap, fill=0x5A)
        assert res["status"] == GB_ERR_ARG
        assert (res["chains_used"], res["seeds_used"]) == (nc, ns)
        assert (res["read_chain_off"] == full["read_chain_off"]).all()
        if ccap >= nc:
            assert (res["chain_seed_off"] == full["chain_seed_off"]).all()
        assert (res["seeds"].view(np.uint8) == 0x5A).all() and (res["info"].view(np.uint8) == 0x5A).all()


def test_no_reads(host):
    res = bsw.seeds2chains_raw(1000, np.zeros(0, np.int32), np.zeros(0, bsw.MEM_DTYPE), np.zeros(0, np.int64))
    assert res["status"] == 0 and res["chains_used"] == 0 and res["seeds_used"] == 0
    assert res["read_chain_off"][0] == 0 and res["chain_seed_off"][0] == 0


def shuffled(inp, seed):
    """Each read's SMEMs in another order, with their coordinates."""
    rng = np.random.default_rng(seed)
    order = np.lexsort((rng.random(len(inp.mems)), inp.mems["read"]))
    off = np.concatenate([[0], np.cumsum(inp.mems["n_coord"], dtype=np.int64)])
    out = inp.take(np.arange(len(inp.lens)))
    out.mems = inp.mems[order]
    out.coords = np.concatenate([inp.coords[off[i]:off[i + 1]] for i in order])
    return out


def test_smem_order_is_free(golden, host):
    sh = shuffled(golden.all, 3)
    assert (sh.mems["m"] != golden.all.mems["m"]).any()
    for stage in (0, 1):
        assert_same(sh.run(stage=stage), golden.expected("default", stage), f"shuffled stage {stage}")


def test_one_contig_without_tables(golden, host):
    """contig_end == NULL is one contig: a seed across a contig boundary is then an ordinary seed."""
    sm = _small(golden)
    a = sm.run(contig_end=None, contig_is_alt=None)
    b = sm.run(contig_end=np.array([sm.l_pac]), contig_is_alt=np.zeros(1, np.uint8))
    assert all((a[k] == b[k]).all() for k in a) and (a["info"]["rid"] == 0).all()


def _cli_case(golden, tmp_path, env):
    """bin/bsw -mkchains on 42 reads written as text, against the library call on the same reads."""
    exe = os.path.join(ROOT, "genomicsbench_palisade_amd", "bin", "bsw")
    sm = _small(golden)
    off = np.concatenate([[0], np.cumsum(sm.mems["n_coord"], dtype=np.int64)])
    first = np.searchsorted(sm.mems["read"], np.arange(len(sm.lens) + 1))
    f = tmp_path / "smems.txt"
    with open(f, "w") as fh:
        for r, n in enumerate(sm.lens):
            fh.write(f"{n} {first[r + 1] - first[r]}\n")
            for i in range(first[r], first[r + 1]):
                m = sm.mems[i]
                fh.write(" ".join(str(int(x)) for x in [m["m"], m["n"], m["s"], *sm.coords[off[i]:off[i + 1]]]) + "\n")
    ce = ",".join(str(int(x)) for x in sm.contig_end)
    alt = ",".join(str(int(x)) for x in sm.is_alt)
    for stage, extra, opt in ((1, [], bsw.chain_opt()), (0, ["-stage", "0"], bsw.chain_opt()),
                              (1, ["-w", "4", "-drop", "0.9", "-maxextend", "2"],
                               bsw.chain_opt(w=4, drop_ratio=0.9, max_chain_extend=2))):
        res = sm.run(stage=stage, opt=opt)
        cso = res["chain_seed_off"]
        lines = []
        for r in range(len(sm.lens)):
            for c in range(res["read_chain_off"][r], res["read_chain_off"][r + 1]):
                x = res["info"][c]
                seeds = "".join(f"\t{s['score']};{s['len']};{s['qbeg']},{s['rbeg']}" for s in res["seeds"][cso[c]:cso[c + 1]])
                lines.append(f"{r}\t{x['pos']}\t{x['rid']}\t{x['is_alt']}\t{x['w']}\t{x['kept']}\t{cso[c + 1] - cso[c]}{seeds}\n")
        out = subprocess.run([exe, "-mkchains", str(f), "-contigs", ce, "-alt", alt] + extra, check=True,
                             capture_output=True, timeout=120, text=True, env=env)
        assert out.stdout == "".join(lines) and len(lines) > 40
    r = subprocess.run([exe, "-mkchains", "-chain2aln", str(f), "-lpac", "5"], capture_output=True, timeout=120, env=env)
    assert r.returncode == 1 and b"excludes" in r.stderr
    r = subprocess.run([exe, "-mkchains", str(f), "-lpac", "5"], capture_output=True, timeout=120, env=env)
    assert r.returncode == 1 and b"coordinate" in r.stderr


def test_cli_long_smem_line(golden, host, tmp_path):
    """An SMEM line of 20 000 coordinates (about 120 KB) is read whole."""
    exe = os.path.join(ROOT, "genomicsbench_palisade_amd", "bin", "bsw")
    rng = np.random.default_rng(4)
    coords = rng.integers(0, int(golden.fx["contig_end"][0]) - 40, 20000)
    mems = np.array([(0, 0, 29, 20000, 20000)], bsw.MEM_DTYPE)
    inp = Inputs(golden.fx, [100], mems, coords)
    res = inp.run(opt=bsw.chain_opt(max_occ=100000), contig_end=None, contig_is_alt=None)
    f = tmp_path / "long.txt"
    f.write_text("100 1\n0 29 20000 " + " ".join(str(int(c)) for c in coords) + "\n")
    out = subprocess.run([exe, "-mkchains", str(f), "-lpac", str(inp.l_pac), "-maxocc", "100000"], check=True,
                         capture_output=True, timeout=120, text=True, env=dict(os.environ, GB_BSW_MKCHAIN_HOST="1"))
    lines = out.stdout.splitlines()
    assert len(lines) == len(res["info"]) > 100
    assert [int(x.split("\t")[1]) for x in lines] == res["info"]["pos"].tolist()
    assert sum(int(x.split("\t")[6]) for x in lines) == len(res["seeds"])
    (tmp_path / "bad.txt").write_text("100 1\n0 29 1 12x\n")
    r = subprocess.run([exe, "-mkchains", str(tmp_path / "bad.txt"), "-lpac", "1000"], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"not a coordinate" in r.stderr


def test_cli_mkchains_host(golden, host, tmp_path):
    _cli_case(golden, tmp_path, dict(os.environ, GB_BSW_MKCHAIN_HOST="1"))


@pytest.mark.skipif(not mk.available(), reason="needs the reference tree and oracle/_ref (make ref)")
def test_live_fuzz(golden, host):
    """500 fresh reads through the live reference: the host path equals mem_chain and mem_chain_flt."""
    contigs, sites = mk.make_reference()
    reads = mk.make_reads(contigs, sites, n_scale=0.32, seed=20261019)[:500]
    assert len(reads) == 500
    live = mk.LiveBwa(contigs)
    try:
        o = mk.opts()
        seeds = [live.seeds(x, o) for x in reads]
        per = [live.chains(x, o) for x in reads]
    finally:
        live.close()
    pin = mk.pack_inputs(seeds)
    mems = np.zeros(len(pin["m"]), bsw.MEM_DTYPE)
    for f in ("read", "m", "n", "n_coord", "s"):
        mems[f] = pin[f]
    inp = Inputs(golden.fx, [len(x) for x in reads], mems, pin["coords"])
    for stage in (0, 1):
        flat = [c for x in per for c in x[stage]]
        rco = np.concatenate([[0], np.cumsum([len(x[stage]) for x in per])])
        cso = np.concatenate([[0], np.cumsum([len(c["seeds"]) for c in flat])])
        sd = np.array([s for c in flat for s in c["seeds"]], np.int64).reshape(-1, 4)
        seeds_e = {"rbeg": sd[:, 0], "qbeg": sd[:, 1], "len": sd[:, 2], "score": sd[:, 3]}
        info = {f: np.array([c[f] for c in flat]) for f in ("pos", "rid", "is_alt", "w", "kept")}
        info["frac_rep"] = np.array([c["frac_rep"] for c in flat], np.float32)
        assert_same(inp.run(stage=stage), (rco, cso, seeds_e, info), f"live stage {stage}")
    assert len(flat) > 1000


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_device_equals_fixture(golden, device):
    check_groups(golden, "device")
    b, f, e, host_reads = bsw.seeds2chains_timing()
    assert host_reads == 0 and b > 0 and f > 0 and e > 0
    # the fixture's largest read stays under the documented bound
    per_read = np.bincount(golden.all.mems["read"], weights=golden.all.mems["n_coord"])
    assert 500 < per_read.max() <= bsw.MKCHAIN_DEV_COORDS


@pytest.mark.gpu
def test_device_host_reads_zero_on_default(golden, device):
    golden.all.run()
    assert bsw.seeds2chains_timing()[3] == 0


@pytest.mark.gpu
def test_device_buffers_are_reused(golden, device):
    """A small call, a large one and the small one again on one thread: the cached buffers grow once and
    the slices are laid out per call."""
    sm = _small(golden)
    first = sm.run()
    assert_same(golden.all.run(), golden.expected("default", 1), "large after small")
    again = sm.run()
    assert all((first[k] == again[k]).all() for k in first)


@pytest.mark.gpu
def test_device_cap_protocol(golden, device):
    sm = _small(golden)
    full = sm.run()
    nc, ns = len(full["info"]), len(full["seeds"])
    for ccap, scap in ((nc, ns - 1), (nc - 1, ns)):
        res = sm.run(raw=True, chain_cap=ccap, seed_cap=scap, fill=0x5A)
        assert res["status"] == GB_ERR_ARG and (res["chains_used"], res["seeds_used"]) == (nc, ns)
        assert (res["read_chain_off"] == full["read_chain_off"]).all()
        assert (res["seeds"].view(np.uint8) == 0x5A).all() and (res["info"].view(np.uint8) == 0x5A).all()


@pytest.mark.gpu
def test_device_output_feeds_chain2aln(golden, device):
    # every read of the fixture lies in chain2aln's domain (1 <= l_query <= GB_BSW_MAX_QLEN = 255)
    sel = np.arange(len(golden.fx["lens"]))[::4]
    inp = golden.all.take(sel)
    ch = inp.run()
    assert len(ch["seeds"]) > 1000
    ref = bsw.Ref.from_codes(golden.fx["ref_codes"])
    reads = [golden.reads[r] for r in sel]
    lens = np.array([len(x) for x in reads], np.int64)
    idq = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    res = bsw.chain2aln_csr(ref, np.concatenate(reads), idq, lens.astype(np.int32), ch["read_chain_off"],
                            ch["chain_seed_off"], ch["seeds"], contig_end=golden.fx["contig_end"], want_raw=False)
    ref.close()
    has = np.diff(ch["read_chain_off"]) > 0
    assert (res["n_reg"][has] > 0).all() and (res["n_reg"][~has] == 0).all()
    assert res["n_reg"].sum() == len(res["regs"]) > 500


def _random_reads(fx, n, seed):
    """n fresh reads of 30 to 250 bases from the fixture's reference, both strands, 0 to 4 substitutions,
    an N now and then: 85 % start in front of the 1 050-copy array (unique sequence, the tandem repeats,
    the ALT copy, the family), 15 % anywhere, so that a few thousand land in the array and bring 500
    coordinates with an SMEM."""
    rng = np.random.default_rng(seed)
    ref = fx["ref_codes"]
    L = len(ref)
    lens = rng.integers(30, 251, n).astype(np.int32)
    front = int(fx["contig_end"][1]) + 9000
    start = np.where(rng.random(n) < 0.85, rng.integers(0, front, n), rng.integers(0, L, n))
    start = np.minimum(start, L - lens)
    col = np.arange(250)[None, :]
    codes = ref[np.minimum(start[:, None] + col, L - 1)]
    sub = (rng.random(codes.shape) < (rng.integers(0, 5, n) / lens)[:, None])
    codes = np.where(sub, (codes + rng.integers(1, 4, codes.shape)) % 4, codes).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.0005] = 4
    rev = rng.random(n) < 0.5
    # reverse complement inside each read's own length
    src = np.where(rev[:, None], lens[:, None] - 1 - col, col)
    flipped = np.take_along_axis(codes, np.clip(src, 0, 249), axis=1)
    codes = np.where(rev[:, None], np.where(flipped < 4, 3 - flipped, 4), codes).astype(np.uint8)
    codes[col >= lens[:, None]] = 4
    return np.ascontiguousarray(codes), lens


@pytest.mark.gpu
def test_device_equals_host_on_random_reads(golden, monkeypatch):
    """20 000 fresh random reads on the fixture's reference, their seeds from the library's own index,
    search and SA lookup: the device and the host path give the same bytes at both stages. A consistency
    check between two paths of ours; the fixture is the yardstick."""
    from genomicsbench_palisade_amd import fmi
    fx = golden.fx
    codes, lens = _random_reads(fx, 20000, 77)
    idx = fmi.Index.build(fx["ref_codes"])
    rd = fmi.Reads(idx, codes, lens)
    rd.search(19)
    rd.sync()
    smems = rd.results()[0]
    rd.close()
    coords, counts = idx.sa_entries(smems, max_occ=500, mode=fmi.SA_COMPRESSED)
    idx.close()
    inp = Inputs(fx, lens, bsw.mems_from_smems(smems, counts), coords)
    per_read = np.bincount(inp.mems["read"], weights=inp.mems["n_coord"], minlength=len(lens))
    monkeypatch.delenv("GB_BSW_MKCHAIN_HOST", raising=False)
    dev = {s: inp.run(stage=s) for s in (0, 1)}
    assert bsw.seeds2chains_timing()[3] == 0
    chains = np.diff(dev[0]["read_chain_off"])
    # the heavy cases are in: three-level trees, sorts that push, s > max_occ
    assert (chains > 81).sum() >= 300 and (chains > 34).sum() >= 1000 and per_read.max() >= 500
    assert len(dev[1]["info"]) > 50000
    monkeypatch.setenv("GB_BSW_MKCHAIN_HOST", "1")
    for s in (0, 1):
        hst = inp.run(stage=s)
        for k in hst:
            assert hst[k].tobytes() == dev[s][k].tobytes(), (s, k)
    assert bsw.seeds2chains_timing()[3] == 20000


@pytest.mark.gpu
def test_device_and_host_reads_in_one_call(golden, device, monkeypatch):
    """With the bound lowered to 100 coordinates the fixture's heavy reads take the host path and the
    others the device, in one call; the spliced result is the fixture's."""
    per_read = np.bincount(golden.all.mems["read"], weights=golden.all.mems["n_coord"], minlength=len(golden.all.lens))
    monkeypatch.setenv("GB_BSW_MKCHAIN_DEV_COORDS", "100")
    for stage in (0, 1):
        assert_same(golden.all.run(stage=stage), golden.expected("default", stage), f"mixed stage {stage}")
        b, f, e, host_reads = bsw.seeds2chains_timing()
        assert host_reads == (per_read > 100).sum() and 100 < host_reads < len(per_read) - 100 and b > 0
    # the cap protocol across the splice
    full = golden.all.run()
    nc, ns = len(full["info"]), len(full["seeds"])
    for ccap, scap in ((nc, ns - 1), (nc - 1, ns)):
        res = golden.all.run(raw=True, chain_cap=ccap, seed_cap=scap, fill=0x5A)
        assert res["status"] == GB_ERR_ARG and (res["chains_used"], res["seeds_used"]) == (nc, ns)
        assert (res["read_chain_off"] == full["read_chain_off"]).all()
        assert (res["seeds"].view(np.uint8) == 0x5A).all() and (res["info"].view(np.uint8) == 0x5A).all()
    # enough host reads for several host threads
    monkeypatch.setenv("GB_BSW_MKCHAIN_DEV_COORDS", "5")
    assert_same(golden.all.run(), golden.expected("default", 1), "mixed, threaded host part")
    assert bsw.seeds2chains_timing()[3] >= 256
    monkeypatch.setenv("GB_BSW_MKCHAIN_DEV_COORDS", "many")
    assert golden.all.run(raw=True)["status"] == GB_ERR_ARG


@pytest.mark.gpu
def test_cli_mkchains_device(golden, device, tmp_path):
    env = dict(os.environ)
    env.pop("GB_BSW_MKCHAIN_HOST", None)
    _cli_case(golden, tmp_path, env)


@pytest.mark.gpu
def test_end_to_end_from_reads(golden, device, tmp_path):
    """reads -> gb_fmi_search -> gb_fmi_sa_entries -> seeds2chains on the fixture's reference: the SMEMs and
    coordinates equal the fixture's (bwa v1's), and the chains equal the live ones."""
    from genomicsbench_palisade_amd import fmi
    fx = golden.fx
    idx = fmi.Index.build(fx["ref_codes"])
    rd = fmi.Reads(idx, fx["reads"], fx["lens"])
    rd.search(19)
    rd.sync()
    smems = rd.results()[0]
    rd.close()
    coords, counts = idx.sa_entries(smems, max_occ=500, mode=fmi.SA_COMPRESSED)
    idx.close()
    assert (np.diff(smems["rid"].astype(np.int64)) >= 0).all()
    mems = bsw.mems_from_smems(smems, counts)
    # step 3: per read the same multiset of (m, n, s, coordinates)
    def per_read(m, c):
        off = np.concatenate([[0], np.cumsum(m["n_coord"], dtype=np.int64)])
        out = [[] for _ in range(len(fx["lens"]))]
        for i in range(len(m)):
            out[m["read"][i]].append((int(m["m"][i]), int(m["n"][i]), int(m["s"][i]), tuple(c[off[i]:off[i + 1]].tolist())))
        return [sorted(x) for x in out]
    got, exp = per_read(mems, coords), per_read(golden.all.mems, golden.all.coords)
    bad = [r for r in range(len(got)) if got[r] != exp[r]]
    assert not bad, f"{len(bad)} reads differ in their SMEMs or coordinates; first {bad[:10]}"
    inp = Inputs(fx, fx["lens"], mems, coords)
    for stage in (0, 1):
        assert_same(inp.run(stage=stage), golden.expected("default", stage), f"end to end stage {stage}")
