"""The per-call SMEM kernels behind the FMI_search class drop-in (csrc/fmi_tasks.hip, csrc/fmi_wave.h:
gb_fmi_smem_onepos / _allpos, gb_fmi_last_seeds, gb_fmi_get_smems) at their list, slot and launch
edges, exact against the oracle (oracle/fmi_oracle.c): record count, all six fields in order, next_pos,
rounds and the backwardExt count.

The first tests need no GPU: from the oracle and one_pos_trace (fmi_task_shapes.py) they prove that the
constructed inputs reach the branches the GPU tests are about -- `prev` lists of more than one, two and
three 64-entry chunks and of the full capacity, a first-loop stop in a later chunk, a dedupe across a
chunk boundary, tasks with exactly a slot's records, one more, and more than twice as many."""
import numpy as np
import pytest

import fmi_task_shapes as S
import fmi_util
from genomicsbench_palisade_amd import gen

gpu = pytest.mark.gpu
BIG = (1 << 31) - 1


def _nested_pairs():
    return [(name, r) for name in S._SPECS for r in range(len(S._SPECS[name][1]))]


def _trace(name, r, min_intv=1, min_seed_len=1):
    """one_pos_trace at the nested read's x0, checked against the oracle (records and next_x)."""
    c = S.case(name)
    x0 = c.specs[r][1]
    rec, nx, tr = S.one_pos_trace(c.ref, c.rs.reads[r], x0, min_intv, min_seed_len)
    exp, enx, _ = S.oracle_onepos(c.oi, c.rs, [x0], [min_intv], [r], min_seed_len)
    assert [(r,) + tuple(int(v) for v in e) for e in rec] == [tuple(e) for e in exp.tolist()]
    assert nx == enx[0]
    return rec, tr


# ------------------------------------------------------------------ witnesses (CPU)
@pytest.mark.parametrize("name,r", _nested_pairs())
def test_trace_equals_oracle(name, r):
    rec, tr = _trace(name, r)
    L, x0 = S.case(name).specs[r][:2]
    assert tr[0]["n_list"] == L - x0  # the forward extension changes s at every step


def test_witness_long_lists():
    longest = {k: max(s["n_list"] for s in _trace(*k)[1]) for k in
               [("L151", 2), ("L256", 1), ("L256", 0), ("L255", 0), ("L256", 2), ("L257", 0)]}
    assert 65 <= longest[("L151", 2)] < 129 <= longest[("L256", 1)] < 193 <= longest[("L256", 0)]
    assert longest[("L255", 0)] == 254
    assert longest[("L256", 2)] == 255   # the LDS lists' capacity less one slot: maxlen + 1 entries
    assert longest[("L257", 0)] == 256   # the lane kernel's rows hold maxlen + 2


def test_witness_first_stop_in_a_later_chunk():
    """min_seed_len above the read length: nothing can be emitted, the 100 longest entries have no left
    context -- the first loop runs through the whole first chunk and stops on a push at entry 100."""
    rec, tr = _trace("L256", 3, min_seed_len=257)
    s = tr[0]["s_ext"]
    assert rec == [] and tr[0]["f"] == 100 and tr[0]["kind"] == "push"
    assert max(s[:64]) < 1 and min(s[100:]) >= 1   # no survivor in the first chunk, some in the next
    # with min_seed_len 1 the same step stops on an emit at entry 0 and the pushes start in chunk two
    rec, tr = _trace("L256", 3)
    assert tr[0]["f"] == 0 and tr[0]["kind"] == "emit" and min(tr[0]["pushed"]) == 100


@pytest.mark.parametrize("name,r", [("L256", 4), ("L257", 2)])
def test_witness_equal_s_across_chunk_boundaries(name, r):
    """Entries 63 and 64, and 127 and 128, survive the first backward step with the same s': the
    second of each pair is the first lane of its chunk and must not be pushed."""
    _, tr = _trace(name, r)
    s, pushed = tr[0]["s_ext"], tr[0]["pushed"]
    assert s[63] == s[64] >= 1 and s[127] == s[128] >= 1 and s[64] != s[127]
    assert pushed[:5] == list(S.RUNS_AT)
    assert 64 not in pushed and 128 not in pushed


def test_witness_slots():
    c = S.case("SLOT")
    one = [len(S.oracle_onepos(c.oi, c.rs, [c.specs[r][1]], [1], [r], 1)[0]) for r in range(3)]
    assert one == [32, 33, 101]          # the slot, one more, above twice the slot
    allp = [len(S.oracle_allpos(c.oi, c.rs, [1], [r], 1)[0]) for r in range(3)]
    assert allp == [32, 33, 101]
    last, _ = S.oracle_last(c.oi, c.rs, [1 << 30] * c.rs.n, 1)
    per = np.bincount(last[:, 0], minlength=c.rs.n)
    assert per[11] == 48 and per[12] == 49 and per[13] == 128 and (per[:11] != 48).all()
    g = S.case("G256")
    rec, _ = S.oracle_get_smems(g.oi, np.stack(g.rs.reads), g.rs.n, 1)
    per = np.bincount(rec[:, 0], minlength=g.rs.n)
    assert per[:3].tolist() == [64, 65, 130] and per[3:].max() < 64


# ------------------------------------------------------------------ GPU: helpers
WAVES = [None, "0"]   # GB_FMI_TASK_WAVE unset (a wave per task up to 256 bases) / "0" (a lane per task)
_expect = {}


def expect(key, fn):
    """The oracle's answer for `key`, computed once and shared by the parametrisations."""
    if key not in _expect:
        _expect[key] = fn()
    return _expect[key]


@pytest.fixture(scope="module")
def dev():
    from genomicsbench_palisade_amd import fmi
    built = {}

    def get(name, ref):
        if name not in built:
            built[name] = fmi.Index.build(ref)
        return built[name]
    yield get
    for i in built.values():
        i.close()


@pytest.fixture
def knobs(monkeypatch):
    def set_(wave=None, tile=None):
        for k, v in (("GB_FMI_TASK_WAVE", wave), ("GB_FMI_TASK_TILE", tile)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
    return set_


def same(got, exp, what):
    g = S.fields(got)
    assert len(g) == len(exp), f"{what}: {len(g)} records, the oracle has {len(exp)}"
    bad = np.nonzero((g != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: record {bad[0]} is {g[bad[0]].tolist()}, the oracle has {exp[bad[0]].tolist()}"


def check_onepos(idx, oi, rs, qpos, intv, rid, msl, key):
    exp, enx, ecalls = expect(("one", key), lambda: S.oracle_onepos(oi, rs, qpos, intv, rid, msl))
    got, nx, calls = idx.smem_onepos(rs.flat, rs.lens, rs.offs, qpos, intv, rid, msl)
    same(got, exp, f"OnePos {key}")
    assert (nx == enx).all(), f"OnePos {key}: next_pos differs at tasks {np.nonzero(nx != enx)[0][:5]}"
    assert calls == ecalls, f"OnePos {key}: {calls} backwardExt calls, the oracle made {ecalls}"
    return exp


def check_allpos(idx, oi, rs, intv, rid, msl, key):
    exp, ernd, ecalls = expect(("all", key), lambda: S.oracle_allpos(oi, rs, intv, rid, msl))
    got, rnd, calls = idx.smem_allpos(rs.flat, rs.lens, rs.offs, intv, rid, msl)
    same(got, exp, f"AllPos {key}")
    assert (rnd == ernd).all(), f"AllPos {key}: rounds {rnd.tolist()} vs {ernd.tolist()}"
    assert calls == ecalls, f"AllPos {key}: {calls} backwardExt calls, the oracle made {ecalls}"
    return exp


def check_last(idx, oi, rs, max_intv, msl, key):
    exp, ecalls = expect(("last", key), lambda: S.oracle_last(oi, rs, max_intv, msl))
    got, calls = idx.last_seeds(rs.flat, rs.lens, rs.offs, max_intv, msl)
    same(got, exp, f"LAST {key}")
    assert calls == ecalls, f"LAST {key}: {calls} backwardExt calls, the oracle made {ecalls}"
    return exp


def check_get_smems(idx, oi, codes, msl, nthreads, key):
    exp, ecalls = expect(("right", key), lambda: S.oracle_get_smems(oi, codes, len(codes), msl, nthreads))
    got, calls = idx.get_smems(codes, len(codes), msl, nthreads)
    same(got, exp, f"getSMEMs {key}")
    assert calls == ecalls, f"getSMEMs {key}: {calls} backwardExt calls, the oracle made {ecalls}"
    return exp


# ------------------------------------------------------------------ a. long lists
LONG = [("L151", w) for w in WAVES] + [("L255", w) for w in WAVES] + [("L256", w) for w in WAVES] + [("L257", None)]
ALL_X_OF = {"L151": 2, "L255": 1, "L256": 1, "L257": 1}   # the nested read whose every x is a task


@gpu
@pytest.mark.parametrize("name,wave", LONG)
def test_long_lists(dev, knobs, name, wave):
    """Nested reads (lists of up to maxlen entries: two to four chunks of the wave kernel, the LDS
    lists' capacity at 256 bases; 257 bases: the lane kernel): OnePos at every nested read's x0 and at
    every x of one of them, AllPos and LAST over the whole set."""
    c = S.case(name)
    rs, oi = c.rs, c.oi
    idx = dev(name, c.ref)
    knobs(wave=wave)
    r_all = ALL_X_OF[name]
    rid = list(range(c.nested)) + [r_all] * int(rs.lens[r_all])
    qpos = [c.specs[r][1] for r in range(c.nested)] + list(range(int(rs.lens[r_all])))
    ones = [1] * len(rid)
    exp = check_onepos(idx, oi, rs, qpos, ones, rid, 1, (name, "x0+allx"))
    assert len(exp) > 100
    # nothing can be emitted: the first loop of every step runs until its first survivor
    check_onepos(idx, oi, rs, qpos, ones, rid, rs.maxlen + 1, (name, "noemit"))
    everyone = np.arange(rs.n)
    check_allpos(idx, oi, rs, [1] * rs.n, everyone, 1, (name, "msl1"))
    check_allpos(idx, oi, rs, [2] * rs.n, everyone, 19, (name, "msl19"))
    check_last(idx, oi, rs, [1 << 30] * rs.n, 1, (name, "huge"))
    check_last(idx, oi, rs, [20] * rs.n, 20, (name, "20"))


# ------------------------------------------------------------------ b. slots
# reads of case SLOT: 0, 1, 2 nested (OnePos / AllPos 32, 33, 101 records), 3-10 ordinary, 11-13 random
# reads of 96, 98 and 256 bases (LAST 48, 49, 128)
ARRANGE = {
    "mixed": list(range(14)),
    "first": [1, 3, 4, 8, 5],          # the task one above the slot first
    "last": [3, 4, 8, 5, 1],
    "alone": [1],
    "first2x": [2, 0, 3, 9, 4],        # the task above twice the slot first (cap = need on the re-run)
    "last_first": [12, 3, 8, 11],      # LAST: 49 records first, 48 last
    "last_last": [11, 3, 8, 12],
    "last_alone": [12],
}


@gpu
@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("tile", [None, "1", "5"])
@pytest.mark.parametrize("arr", list(ARRANGE))
def test_slots(dev, knobs, arr, tile, wave):
    """Tasks with exactly a slot's records, one more and above twice as many, in one call with ordinary
    tasks: the re-run with cap = need, its packing rule and its pass-0-only call count. tile: tasks per
    launch (1: every task alone, 5: the overflowing subset of a tile)."""
    c = S.case("SLOT")
    sub = S.ReadSet([c.rs.reads[r] for r in ARRANGE[arr]])
    idx = dev("SLOT", c.ref)
    knobs(wave=wave, tile=tile)
    x0 = {0: 31, 1: 32, 2: 100}
    rid = np.arange(sub.n)
    qpos = [x0.get(r, int(c.rs.lens[r]) // 2) for r in ARRANGE[arr]]
    one = check_onepos(idx, c.oi, sub, qpos, [1] * sub.n, rid, 1, arr)
    allp = check_allpos(idx, c.oi, sub, [1] * sub.n, rid, 1, arr)
    last = check_last(idx, c.oi, sub, [1 << 30] * sub.n, 1, arr)
    if arr == "mixed":   # the call holds both sides of each slot and a task above twice it
        per = np.bincount(one[:, 0], minlength=sub.n)
        assert per[:3].tolist() == [32, 33, 101]
        assert np.bincount(allp[:, 0], minlength=sub.n)[:3].tolist() == [32, 33, 101]
        assert np.bincount(last[:, 0], minlength=sub.n)[11:].tolist() == [48, 49, 128]


# ------------------------------------------------------------------ c. launch shapes
def _short_reads():
    ref = gen.fmi_reference(60_000, seed=71)
    codes, lens = gen.fmi_reads(ref, 700, read_len=100, seed=171, sub_rate=0.02, n_rate=0.002)
    return ref, S.ReadSet(list(codes)), fmi_util.OracleIndex(ref)


def short_reads():
    return expect("short_reads", _short_reads)


@gpu
@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("tile", [None, "65536", "4096"])
def test_seventy_thousand_tasks(dev, knobs, tile, wave):
    """Every (read, x) of 700 reads of 100 bases in one OnePos call. At the default tile that is one
    launch; the wave kernel's grid is min(n, 65535), so its waves stride over the tasks."""
    ref, rs, oi = short_reads()
    idx = dev("short", ref)
    knobs(wave=wave, tile=tile)
    rid = np.repeat(np.arange(rs.n, dtype=np.int32), 100)
    qpos = np.tile(np.arange(100, dtype=np.int16), rs.n)
    assert len(rid) == 70_000 > 65_535
    # run_tasks' default tile for these reads (256 MiB of (maxlen + 2) 32-byte `prev` entries per task,
    # rounded down to whole waves) holds the whole call
    default_tile = ((256 << 20) // ((rs.maxlen + 2) * 32)) & ~63
    assert default_tile >= len(rid)
    exp = check_onepos(idx, oi, rs, qpos, np.ones(len(rid), np.int32), rid, 19, "70k")
    assert len(exp) > 10_000


@gpu
@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_task_counts(dev, knobs, n, wave):
    ref, rs, oi = short_reads()
    idx = dev("short", ref)
    knobs(wave=wave)
    sub = S.ReadSet(rs.reads[200:200 + n])
    rid = np.arange(n)
    check_onepos(idx, oi, sub, [(7 * i) % 100 for i in range(n)], [1] * n, rid, 12, ("count", n))
    check_allpos(idx, oi, sub, [1] * n, rid, 12, ("count", n))
    check_last(idx, oi, sub, [20] * n, 13, ("count", n))


# ------------------------------------------------------------------ d. mixed and degenerate reads
def _mixed():
    ref, _, oi = short_reads()
    rng = np.random.default_rng(4)

    def cut(length, at=None):
        at = int(rng.integers(0, len(ref) - length)) if at is None else at
        return ref[at:at + length].copy()
    reads = [cut(n) for n in (0, 1, 2, 18, 19, 20, 255, 256)]
    for r in reads[6:]:                                    # a few substitutions: several AllPos rounds
        at = rng.integers(0, len(r), 8)
        r[at] = (r[at] + 1) % 4
    reads.append(np.full(20, 4, np.uint8))                 # 8: all N
    one = np.full(20, 4, np.uint8)
    one[7] = 2
    reads.append(one)                                      # 9: one real base
    for pos in (0, 49, 30):                                # 10, 11, 12: N first, N last, N inside
        r = cut(60 if pos == 30 else 50)
        r[pos] = 4
        reads.append(r)
    return S.ReadSet(reads)


def mixed():
    return expect("mixed", _mixed)


INTVS = [1, 2, 1000, BIG]


def _mixed_onepos_tasks(rs):
    """(rid, x, min_intv): both ends of every read, on an N, next to an N on either side; each with
    every min_intv (2^31 - 1 exceeds every interval, 1000 all but those of one to three bases)."""
    at = []
    for r in range(rs.n):
        n = int(rs.lens[r])
        if n:
            at += [(r, 0), (r, n - 1)]
    at += [(8, 10), (9, 6), (9, 7), (9, 8), (10, 1), (11, 48), (12, 29), (12, 30), (12, 31), (6, 128), (7, 200)]
    return [(r, x, i) for (r, x) in at for i in INTVS]


@gpu
@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_mixed_reads_onepos(dev, knobs, order, wave):
    """Lengths 0 to 256 in one call (maxlen sizes the LDS of every task), each read named by several
    tasks with different min_intv, tasks in either read order."""
    ref, _, oi = short_reads()
    rs = mixed()
    idx = dev("short", ref)
    knobs(wave=wave)
    tasks = _mixed_onepos_tasks(rs)
    if order == "descending":
        tasks = tasks[::-1]
    rid, qpos, intv = (np.array(v) for v in zip(*tasks))
    for msl in (1, 19):
        exp = check_onepos(idx, oi, rs, qpos, intv, rid, msl, ("mixed", order, msl))
        assert len(exp) > 0
    # A min_intv above every interval leaves only the one-base entry that the forward loop stores before
    # it tests s (FMI_search.cpp:1044-1060); min_seed_len 19 drops it: no record, and next_pos as the
    # oracle leaves it. (1000 is above every interval of 19 bases or more in 120 k bases of text.)
    sel = intv >= 1000
    got, nx, _ = idx.smem_onepos(rs.flat, rs.lens, rs.offs, qpos[sel], intv[sel], rid[sel], 19)
    assert len(got) == 0
    _, enx, _ = S.oracle_onepos(oi, rs, qpos[sel], intv[sel], rid[sel], 19)
    assert (nx == enx).all()


@gpu
@pytest.mark.parametrize("wave", WAVES)
def test_mixed_reads_allpos(dev, knobs, wave):
    """AllPos over the same reads (the empty read included: no round), reads named twice with
    different min_intv and in descending order: the output is round-major in task order, as the
    oracle's rid_array loop gives it."""
    ref, _, oi = short_reads()
    rs = mixed()
    idx = dev("short", ref)
    knobs(wave=wave)
    up = list(range(rs.n))
    for name, rid, intv in [("up", up, [1] * rs.n), ("down", up[::-1], [2] * rs.n),
                            ("twice", [6, 7, 6, 12, 7, 0, 12, 5], [1, 1, 3, 1, BIG, 1, 1000, 2]),
                            ("big", up, [BIG] * rs.n)]:
        for msl in (1, 19):
            exp = check_allpos(idx, oi, rs, intv, rid, msl, ("mixed", name, msl))
            if name in ("up", "twice"):
                assert len(exp) > 0
            if name == "big" and msl == 19:   # at min_seed_len 1 the one-base entries remain (see OnePos)
                assert len(exp) == 0
    # round-major: in "twice" at min_seed_len 1 the tasks' records interleave
    exp = _expect[("all", ("mixed", "twice", 1))][0]
    assert (np.diff(exp[:, 0]) != 0).sum() > 8


@gpu
@pytest.mark.parametrize("wave", WAVES)
def test_mixed_reads_last(dev, knobs, wave):
    ref, _, oi = short_reads()
    rs = mixed()
    idx = dev("short", ref)
    knobs(wave=wave)
    total = 0
    for max_intv in (0, 1, 20, 1 << 30):
        for msl in (1, 20, 300):
            total += len(check_last(idx, oi, rs, [max_intv] * rs.n, msl, ("mixed", max_intv, msl)))
    assert total > 0
    per_read = [0, 1, 20, 1 << 30, 5, 2, 20, 1 << 30, 1, 1, 20, 20, 3]
    check_last(idx, oi, rs, per_read, 2, ("mixed", "per-read"))


# ------------------------------------------------------------------ e. the length limit
def _long_read(n):
    ref, _, _ = short_reads()
    rng = np.random.default_rng(5)
    r = rng.integers(0, 4, n, dtype=np.uint8)
    r[:30_000] = ref[10_000:40_000]
    return r


@gpu
def test_longest_read(dev, knobs):
    """One read of 32 767 bases (the phase calls' limit: positions are int16 in the reference), 30 000
    of them one stretch of the reference: m, n and rounds beyond 13 bits, both slot re-runs."""
    ref, _, oi = short_reads()
    rs = S.ReadSet([_long_read(32_767)])
    idx = dev("short", ref)
    knobs()
    exp = check_allpos(idx, oi, rs, [1], [0], 1, "long")
    assert exp[0, 1] == 0 and exp[0, 2] >= 29_999 and exp[:, 2].max() > 32_000 and len(exp) > 32
    rounds = _expect[("all", "long")][1]
    assert 100 < rounds[0] < 32_767
    exp = check_last(idx, oi, rs, [20], 20, "long")
    assert len(exp) > 48 and exp[:, 2].max() > 8192


# ------------------------------------------------------------------ f. refusals
ERR_ARG = -1
SENT = 0x5A


def _last_error():
    from genomicsbench_palisade_amd import lib
    return lib().gb_last_error().decode(errors="replace")


def _sentinels(nt, cap=256):
    out = np.zeros(cap, fmi_util.SMEM_DTYPE)
    out.view(np.uint8)[:] = SENT
    return out, np.full(nt, 0x5A5A, np.int16), np.full(nt, 0x5A5A5A5A, np.int32)


def _untouched(out, nxt, rnd):
    return (out.view(np.uint8) == SENT).all() and (nxt == 0x5A5A).all() and (rnd == 0x5A5A5A5A).all()


def _refused(idx, rs_args, tasks, text, modes=("one", "all", "last")):
    """Every named entry point refuses the call: GB_ERR_ARG, `text` in gb_last_error(), the outputs
    left as they were. rs_args = (codes, lens, offs, nrid); tasks = (qpos, intv, rid, ntasks)."""
    codes, lens, offs, nrid = rs_args
    qpos, intv, rid, nt = tasks
    for mode in modes:
        out, nxt, rnd = _sentinels(max(nt, 1))
        if mode == "one":
            st, _, _ = idx.smem_onepos_raw(codes, lens, offs, nrid, qpos, intv, rid, nt, 1, out, len(out), nxt)
        elif mode == "all":
            st, _, _ = idx.smem_allpos_raw(codes, lens, offs, nrid, intv, rid, nt, 1, out, len(out), rnd)
        else:
            st, _, _ = idx.last_seeds_raw(codes, lens, offs, nrid, None if intv is None else [20] * nrid, 1, out,
                                          len(out))
        assert st == ERR_ARG, (mode, st)
        assert text in _last_error(), (mode, _last_error())
        assert _untouched(out, nxt, rnd), mode


@gpu
def test_refusals(dev, knobs):
    ref, rs0, oi = short_reads()
    idx = dev("short", ref)
    knobs()
    rs = S.ReadSet(rs0.reads[:3])
    ok = (rs.flat, rs.lens, rs.offs, 3)
    q, i, r = [5, 6, 7], [1, 1, 1], [0, 1, 2]
    # a task names a read outside [0, nrid) (LAST names its reads itself)
    _refused(idx, ok, (q, i, [0, -1, 2], 3), "names read -1", ("one", "all"))
    _refused(idx, ok, (q, i, [0, 1, 3], 3), "names read 3", ("one", "all"))
    # query positions outside the read
    _refused(idx, ok, ([5, -1, 7], i, r, 3), "query position -1", ("one",))
    _refused(idx, ok, ([5, 6, 100], i, r, 3), "query position 100 outside read 2", ("one",))
    # lengths and offsets
    lens = rs.lens.copy()
    lens[1] = -5
    _refused(idx, (rs.flat, lens, rs.offs, 3), (q, i, r, 3), "read 1 has length -5")
    offs = rs.offs.copy()
    offs[2] = -3
    _refused(idx, (rs.flat, rs.lens, offs, 3), (q, i, r, 3), "offset -3")
    big = np.zeros(32_768 + 300, np.uint8)
    big[:300] = rs.flat[:300]
    lens = rs.lens.copy()
    lens[2] = 32_768
    offs = np.array([0, 100, 200], np.int32)
    _refused(idx, (big, lens, offs, 3), (q, i, r, 3), "read 2 has length 32768")
    # null arrays with tasks to run
    _refused(idx, (None, rs.lens, rs.offs, 3), (q, i, r, 3), "null array")
    _refused(idx, (rs.flat, None, rs.offs, 3), (q, i, r, 3), "null array")
    _refused(idx, (rs.flat, rs.lens, None, 3), (q, i, r, 3), "null array")
    _refused(idx, ok, (q, None, r, 3), "null array")
    _refused(idx, ok, (q, i, None, 3), "null array", ("one", "all"))
    _refused(idx, ok, (None, i, r, 3), "null array", ("one",))
    # no tasks: nothing to do, whatever the arrays
    out, nxt, rnd = _sentinels(1)
    assert idx.smem_onepos_raw(None, None, None, 0, None, None, None, 0, 1, out, len(out), nxt)[:2] == (0, 0)
    assert idx.smem_allpos_raw(None, None, None, 0, None, None, 0, 1, out, len(out), rnd)[:2] == (0, 0)
    assert idx.last_seeds_raw(None, None, None, 0, None, 1, out, len(out))[:2] == (0, 0)
    assert idx.get_smems_raw(None, 0, 100, 1, 1, out, len(out))[:2] == (0, 0)
    assert _untouched(out, nxt, rnd)


@gpu
def test_out_cap_one_short(dev, knobs):
    """out_cap one below the need: refused with *nout = the need and nothing written -- not the
    records, not next_pos / rounds; the exact capacity succeeds."""
    ref, rs0, oi = short_reads()
    idx = dev("short", ref)
    knobs()
    rs = S.ReadSet(rs0.reads[:6])
    rid = np.arange(6)
    q, ones = [50] * 6, [1] * 6
    e_one, enx, _ = S.oracle_onepos(oi, rs, q, ones, rid, 12)
    e_all, ernd, _ = S.oracle_allpos(oi, rs, ones, rid, 12)
    e_last, _ = S.oracle_last(oi, rs, [20] * 6, 13)
    codes = np.stack(rs.reads)
    e_right, _ = S.oracle_get_smems(oi, codes, 6, 12)
    calls = {
        "gb_fmi_smem_onepos": (e_one, lambda out, cap, nxt, rnd: idx.smem_onepos_raw(
            rs.flat, rs.lens, rs.offs, 6, q, ones, rid, 6, 12, out, cap, nxt)),
        "gb_fmi_smem_allpos": (e_all, lambda out, cap, nxt, rnd: idx.smem_allpos_raw(
            rs.flat, rs.lens, rs.offs, 6, ones, rid, 6, 12, out, cap, rnd)),
        "gb_fmi_last_seeds": (e_last, lambda out, cap, nxt, rnd: idx.last_seeds_raw(
            rs.flat, rs.lens, rs.offs, 6, [20] * 6, 13, out, cap)),
        "gb_fmi_get_smems": (e_right, lambda out, cap, nxt, rnd: idx.get_smems_raw(codes, 6, 100, 12, 1, out, cap)),
    }
    for name, (exp, call) in calls.items():
        need = len(exp)
        assert need > 1
        out, nxt, rnd = _sentinels(6)
        st, nout, _ = call(out, need - 1, nxt, rnd)
        assert (st, nout) == (ERR_ARG, need), name
        assert f"{name}: {need} SMEMs exceed out_cap {need - 1}" in _last_error()
        assert _untouched(out, nxt, rnd), name
        st, nout, _ = call(out, need, nxt, rnd)
        assert (st, nout) == (0, need), name
        same(out[:need], exp, name)
        assert (out[need:].view(np.uint8) == SENT).all()
        if name == "gb_fmi_smem_onepos":
            assert (nxt == enx).all()
        if name == "gb_fmi_smem_allpos":
            assert (rnd == ernd).all()


@gpu
def test_get_smems_limits(dev, knobs):
    """getSMEMs takes reads of any length (32 768 bases, refused by the phase calls), refuses nthreads
    0 and a first quota of 2^31 bases or more."""
    ref, _, oi = short_reads()
    idx = dev("short", ref)
    knobs()
    codes = np.random.default_rng(6).integers(0, 4, (1, 32_768), dtype=np.uint8)
    exp, ecalls = S.oracle_get_smems(oi, codes, 1, 12)
    st, nout, calls = idx.get_smems_raw(codes, 1, 32_768, 12, 1, None, 0)
    assert (st, nout, calls) == (0, len(exp), ecalls) and nout > 64
    out, _, _ = _sentinels(1)
    small = codes[:, :100]
    st, _, _ = idx.get_smems_raw(small, 1, 100, 12, 0, out, len(out))
    assert st == ERR_ARG and "gb_fmi_get_smems: bad arguments" in _last_error()
    st, _, _ = idx.get_smems_raw(small, 65_536, 32_768, 12, 1, out, len(out))   # refused before any read
    assert st == ERR_ARG and "65536 reads x 32768 bases exceed 2^31" in _last_error()
    assert (out.view(np.uint8) == SENT).all()
    # two threads halve the quota: 32 768 reads x 32 768 bases is below the limit again, but there are
    # no such reads to hand over -- the bound itself is what is checked above


# ------------------------------------------------------------------ g. getSMEMs
@gpu
@pytest.mark.parametrize("tile", [None, "1", "5"])
def test_get_smems_slots(dev, knobs, tile):
    """getSMEMs (the lane kernel only, slots of 64 records) on reads that emit 64, 65 and 130."""
    c = S.case("G256")
    idx = dev("G256", c.ref)
    knobs(tile=tile)
    codes = np.stack(c.rs.reads)
    exp = check_get_smems(idx, c.oi, codes, 1, 1, ("G256", 1))
    assert np.bincount(exp[:, 0], minlength=6)[:3].tolist() == [64, 65, 130]
    check_get_smems(idx, c.oi, codes, 19, 1, ("G256", 19))
    check_get_smems(idx, c.oi, codes[::-1], 1, 2, ("G256", "reversed, tid 0 of 2"))
    check_get_smems(idx, c.oi, codes[1:2], 1, 1, ("G256", "alone"))


@gpu
def test_get_smems_257(dev, knobs):
    c = S.case("L257")
    idx = dev("L257", c.ref)
    knobs()
    codes = np.stack([r for r in c.rs.reads if len(r) == 257])
    exp = check_get_smems(idx, c.oi, codes, 1, 1, ("L257", 1))
    assert np.bincount(exp[:, 0])[1] == 61
