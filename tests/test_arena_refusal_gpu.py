"""GPU: the arena refusal of the five batched calls behind the mapper's opt-in passes — wm_extra_batch, wm_fix_extra_batch, wm_eqx_batch, wm_cs_batch (cs-long mode) and
wm_ksw_ll_batch, in the byte form, which needs no index — on a context whose arena holds 1 MiB: a batch of many small jobs (the random generators of the five case lists,
repeated) whose sequences and CIGAR ops alone exceed the arena is refused with WM_ENOMEM and the text GpuOps::run_split looks for ("does not fit the arena"), every result
array as it was; the same context then serves both halves, which joined are the whole batch run once on a 1 GiB context and what the case lists' restated rules give. The
largest batch that still fits (found by halving from the refused one, then bisecting) is served, and — for the two calls that take arena memory a second time, after their
count pass — a batch 8 jobs larger is refused THERE, again with every result array as it was. Then the mapper under an arena that small that its batched calls are split
(wm_arena_split_stats): all five passes on give what all five off give and what a 2 GiB arena gives, and a final pass was among the calls that were split."""
import ctypes as C
import os
import tempfile
import numpy as np
import pytest
import wmtest as W
import extracases as X
import fixcases as F
import eqxcases as QE
import cscases as QC
import llcases as QL
from winnowmap_amd import build, gpu, synth

pytestmark = pytest.mark.gpu

SMALL = 1 << 20
WM_ENOMEM = -3
ARENA_TEXT = "does not fit the arena"
SWITCHES = ("fix", "extra", "eqx", "cs", "ll")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
# jobs of the largest batch each call serves on a context of SMALL bytes, found on an MI355X by halving from the refused batch and bisecting between the two (the only
# numbers here that come from the device; every job past them adds its sequences and ops to what the call takes from the arena)
FIT = {"extra": 277, "fix": 258, "eqx": 174, "cs": 179, "ll": 1638}
SECOND_SITE = ("eqx", "cs")          # their write pass takes the output from the arena once the count pass has sized it
PAST_FIT = 8                         # jobs past FIT: about 30 KB of sequences, far less than the output the write pass asks for (a sixth and a quarter of the arena)


@pytest.fixture(autouse=True)
def restore_switches():
    try:
        yield
    finally:
        for s in SWITCHES:
            getattr(gpu, "set_%s_device" % s)(-1)


@pytest.fixture(scope="module")
def small():
    c = gpu.Context(0, SMALL)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big():
    c = gpu.Context(0, 1 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def WALK():
    L = C.CDLL(build.build_harness())
    L.h_extra_walk_both.argtypes = [C.c_void_p, C.c_void_p, W.u32p, C.c_int] + [C.c_int] * 5 + [i32p, i32p]

    def walk(cig, q, t, sc):
        f, g = np.zeros(6, np.int32), np.zeros(6, np.int32)
        cg = np.ascontiguousarray(cig, np.uint32) if len(cig) else np.zeros(1, np.uint32)
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        L.h_extra_walk_both(q.ctypes.data, t.ctypes.data, cg, len(cig), *[int(v) for v in sc], f, g)
        return tuple(int(v) for v in g)
    return walk


def pack_final(cases):
    """(name, cigar, q, t, ...) -> jobs, seqs, cigars of a byte-form call"""
    jobs = np.zeros(len(cases), gpu.EXTRA_JOB_DTYPE)
    seqs, cigs = [], [np.zeros(0, np.uint32)]
    at = ops = 0
    for i, c in enumerate(cases):
        cig, q, t = c[1], c[2], c[3]
        jobs[i] = (at, at + len(q), ops, len(cig))
        seqs += [q, t]; at += len(q) + len(t); cigs.append(cig); ops += len(cig)
    return jobs, np.ascontiguousarray(np.concatenate(seqs), np.uint8), np.ascontiguousarray(np.concatenate(cigs), np.uint32)


def ints(a):
    return tuple(int(v) for v in a)


class Call:
    """one batched call through the C ABI, every result array pre-filled by the caller: run(ctx, jobs) -> (rc, arrays); per_job(jobs, arrays) -> what each job got"""
    def __init__(self, name, distinct, want):
        self.name, self.distinct, self.want = name, distinct, want

    def jobs_of(self, n):
        return [self.distinct[i % len(self.distinct)] for i in range(n)]

    def wants_of(self, n):
        return [self.want[i % len(self.distinct)] for i in range(n)]

    def need(self, cases):
        """bytes the call cannot do without: its sequences and one word per CIGAR op, both of which it puts in the arena"""
        return sum(len(c[2]) + len(c[3]) + 4 * len(c[1]) for c in cases)

    def refused_count(self):
        n = len(self.distinct)
        while self.need(self.jobs_of(n)) <= SMALL:
            n += 10
        return n


class Extra(Call):
    def run(self, ctx, cases):
        jobs, seqs, cigs = pack_final(cases)
        sc = np.array(X.ONT, np.int32)
        out = np.full((len(cases), 6), -7, np.int32)
        L = gpu.lib()
        L.wm_extra_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        rc = L.wm_extra_batch(ctx._h, sc.ctypes.data, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, cigs.ctypes.data, len(cigs), out.ctypes.data)
        return rc, [out]

    def per_job(self, cases, arrays):
        return [ints(r) for r in arrays[0]]


class Fix(Call):
    def run(self, ctx, cases):
        jobs, seqs, cigs = pack_final(cases)
        sc = np.array(F.ONT, np.int32)
        out = np.full(len(cigs), 0xdeadbeef, np.uint32); fix = np.full((len(cases), 4), -7, np.int32); extra = np.full((len(cases), 6), -7, np.int32)
        L = gpu.lib()
        L.wm_fix_extra_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.wm_fix_extra_batch(ctx._h, sc.ctypes.data, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, cigs.ctypes.data, len(cigs), out.ctypes.data, fix.ctypes.data, extra.ctypes.data)
        return rc, [out, fix, extra]

    def per_job(self, cases, arrays):
        out, fix, extra = arrays
        got, at = [], 0
        for c, f, x in zip(cases, fix, extra):
            got.append((ints(out[at:at + int(f[0])]), ints(f), ints(x)))
            at += len(c[1])
        return got


class Eqx(Call):
    def run(self, ctx, cases):
        jobs, seqs, cigs = pack_final(cases)
        cap = len(cigs) + int((cigs[(cigs & 0xf) == 0] >> 4).astype(np.int64).sum()) + 1      # every op, and one more per M column: what the CIGARs can become at most
        pool = np.full(cap, 0xdeadbeef, np.uint32); res = np.full(len(cases) * gpu.EQX_RES_DTYPE.itemsize, 0x5a, np.uint8)
        used = C.c_size_t(0)
        L = gpu.lib()
        L.wm_eqx_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        rc = L.wm_eqx_batch(ctx._h, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, cigs.ctypes.data, len(cigs), pool.ctypes.data, cap, C.byref(used), res.ctypes.data)
        return rc, [pool, res]

    def per_job(self, cases, arrays):
        pool, res = arrays[0], arrays[1].view(gpu.EQX_RES_DTYPE)
        return [(ints(pool[int(r["off"]):int(r["off"]) + int(r["n_cigar"])]), int(r["in_place"])) for r in res]


class Cs(Call):
    def run(self, ctx, cases):
        jobs, seqs, cigs = pack_final(cases)
        cap = sum(QC.bound(c[1]) for c in cases) + 1
        pool = np.full(cap, 0x5a, np.uint8); res = np.full(len(cases) * gpu.CS_RES_DTYPE.itemsize, 0x5a, np.uint8)
        used = C.c_size_t(0)
        L = gpu.lib()
        L.wm_cs_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        rc = L.wm_cs_batch(ctx._h, QC.LONG, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, cigs.ctypes.data, len(cigs), pool.ctypes.data, cap, C.byref(used), res.ctypes.data)
        return rc, [pool, res]

    def per_job(self, cases, arrays):
        pool, res = arrays[0], arrays[1].view(gpu.CS_RES_DTYPE)
        return [pool[int(r["off"]):int(r["off"]) + int(r["len"])].tobytes() for r in res]


class Ll(Call):
    def need(self, cases):
        return sum(len(c["q"]) + len(c["t"]) for c in cases)                       # the sequence slab

    def run(self, ctx, cases):
        q_off, t_off, ql, tl, st, seqs = QL.pack(cases, 1)
        jobs = np.zeros(len(cases), gpu.LL_JOB_DTYPE)
        jobs["q_off"], jobs["t_off"], jobs["qlen"], jobs["tlen"], jobs["step"] = q_off, t_off, ql, tl, st
        mat = QL.simple_mat(2, 4, 1)
        out = np.full((len(cases), 3), -7, np.int32)
        L = gpu.lib()
        L.wm_ksw_ll_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        rc = L.wm_ksw_ll_batch(ctx._h, mat.ctypes.data, 4, 2, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, out.ctypes.data)
        return rc, [out]

    def per_job(self, cases, arrays):
        return [ints(r) for r in arrays[0]]


@pytest.fixture(scope="module")
def CALLS(WALK):
    """computed once: per call its distinct jobs — the random generators of its case list, under one scoring — and what the restated rules give for each"""
    made = {}
    ex = X.batch70()
    made["extra"] = Extra("extra", ex, [WALK(c[1], c[2], c[3], X.ONT) for c in ex])
    fx = F.batch70() + [c for c in F.random_cases() if c[4] == F.ONT]
    want = []
    for c in fx:
        fixed, qs, ts, ch, _ = F.fix_py(c[1], c[2], c[3])
        want.append((ints(fixed), (len(fixed), qs, ts, ch), WALK(np.array(fixed, np.uint32), c[2][qs:], c[3][ts:], F.ONT)))
    made["fix"] = Fix("fix", fx, want)
    eq = QE.batch70()
    made["eqx"] = Eqx("eqx", eq, [(lambda w: (ints(w[0]), int(w[1])))(QE.restated(c[1], c[2], c[3])) for c in eq])
    cs = QC.batch70()
    made["cs"] = Cs("cs", cs, [QC.restated(QC.LONG, c[1], c[2], c[3]) for c in cs])
    # the operands of llcases.random_jobs, all under map-ont's scoring (one call takes one): the restated rules for the first 60, the host form (tests/test_abi.py pins
    # it to the reference) for all 300
    ll = [QL.case(c["name"], c["q"], c["t"]) for c in QL.random_jobs(300, 600, 123)]
    L = gpu.lib()
    L.wm_ksw_ll_i16.restype = C.c_int
    L.wm_ksw_ll_i16.argtypes = [C.c_int, W.u8p, C.c_int, W.u8p, W.i8p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    mat = QL.simple_mat(2, 4, 1)
    want = []
    for k, c in enumerate(ll):
        qe, te = C.c_int(), C.c_int()
        s = L.wm_ksw_ll_i16(len(c["q"]), c["q"], len(c["t"]), c["t"], mat, 4, 2, C.byref(qe), C.byref(te))
        want.append((s, qe.value, te.value))
        if k < 60:
            assert ints(QL.restated(c["q"], c["t"], mat, 4, 2)[:3]) == want[-1], c["name"]
    made["ll"] = Ll("ll", ll, want)
    return made


def still_sentinels(arrays):
    """every result array holds the one value it was pre-filled with: the call wrote nothing"""
    return all(a.size > 0 and int(a.flat[0]) in (-7, 0xdeadbeef, 0x5a) and bool((a == a.flat[0]).all()) for a in arrays)


@pytest.mark.parametrize("name", list(FIT))
def test_a_batch_past_the_arena_is_refused_untouched_and_its_halves_are_served(small, big, CALLS, name):
    call = CALLS[name]
    n = call.refused_count()
    cases, wants = call.jobs_of(n), call.wants_of(n)
    assert call.need(cases) > SMALL and n > len(call.distinct) and max(call.need([c]) for c in cases) < SMALL // 50      # many small jobs
    rc, arrays = call.run(small, cases)
    err = gpu.lib().wm_last_error().decode()
    assert rc == WM_ENOMEM and ARENA_TEXT in err and " out) " not in err, (rc, err)          # refused where the call stages its input
    assert still_sentinels(arrays), name
    # the context is as good as new: both halves, which joined are the whole batch on a large arena and the restated rules
    halves = []
    for part in (cases[:n // 2], cases[n // 2:]):
        rc, arr = call.run(small, part)
        assert rc == 0, (name, len(part), gpu.lib().wm_last_error().decode())
        halves += call.per_job(part, arr)
    rc, arr = call.run(big, cases)
    assert rc == 0, gpu.lib().wm_last_error().decode()
    whole = call.per_job(cases, arr)
    assert halves == whole
    for k, (g, w) in enumerate(zip(whole, wants)):
        assert g == w, (name, k, cases[k]["name"] if isinstance(cases[k], dict) else cases[k][0])


@pytest.mark.parametrize("name", list(FIT))
def test_the_largest_batch_that_fits_is_served_and_past_it_the_write_pass_is_refused_untouched(small, CALLS, name):
    call = CALLS[name]
    n = FIT[name]
    assert 0 < n < call.refused_count() and 2 * n >= call.refused_count() - 1
    cases = call.jobs_of(n)
    rc, arr = call.run(small, cases)
    assert rc == 0, (name, n, gpu.lib().wm_last_error().decode())
    assert call.per_job(cases, arr) == call.wants_of(n)
    if name in SECOND_SITE:
        cases = call.jobs_of(n + PAST_FIT)
        assert call.need(cases) < SMALL
        rc, arrays = call.run(small, cases)
        err = gpu.lib().wm_last_error().decode()
        assert rc == WM_ENOMEM and ARENA_TEXT in err and " out) " in err, (rc, err)          # refused behind the count pass, where the output is taken
        assert still_sentinels(arrays), name
        rc, arr = call.run(small, call.jobs_of(n))
        assert rc == 0 and call.per_job(call.jobs_of(n), arr) == call.wants_of(n)


# ---- the mapper under an arena that splits its batched calls ---------------------------------------------------------------------------------------
# No power of two serves: at 8 MiB (and 16, 32 MiB) the run with all five passes on is split exactly as often as the run with all five off (7 : 7, 3 : 3, 1 : 1 — the window
# calls), and at 4 MiB one ksw call alone asks for 4.8 MB and fails the mapping call. At 6 MiB an MI355X counted 8 halvings and 12 parts issued with all five on, 7 and 8 with
# all five off (the same at 5.5 and 5.25 MiB; at 6.5 and 7 MiB 7 : 7 again).
SPLIT_ARENA = 6 << 20


@pytest.fixture(scope="module")
def READS():
    """400 ont reads of 3 kb from a 1 Mb reference"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(1, 1000000, 51, repeat_frac=0.05)
    fa = os.path.join(tmp, "ref.fa")
    synth.write_fasta(fa, ref, prefix="chr")
    reads = [synth.codes_to_ascii(r) for r in synth.make_reads(ref, 400, 3000, 52, profile="ont")[0]]
    return fa, reads, ["read%d" % i for i in range(len(reads))]


def map_under(fa, reads, names, arena, on):
    """one mapping call on a context, and worker contexts, of `arena` bytes each -> (results, wm_arena_split_stats, the five accounts)"""
    ctx = gpu.Context(0, arena)
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, "map-ont", gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG | gpu.MM_F_EQX | gpu.MM_F_OUT_CS | gpu.MM_F_OUT_CS_LONG)
    try:
        m.set_threads(4, arena)
        for s in SWITCHES:
            getattr(gpu, "set_%s_device" % s)(on)
            getattr(gpu, "%s_stats" % s)(reset=True)
        gpu.arena_split_stats(reset=True)
        res = m.map(names, reads)
        return res, gpu.arena_split_stats(), {s: getattr(gpu, "%s_stats" % s)() for s in SWITCHES}
    finally:
        m.close(); idx.close(); ctx.close()


def test_the_mapper_under_a_small_arena_splits_a_final_pass_and_gives_the_same(READS):
    """SPLIT_ARENA (see there for what was observed) is an arena at which the run with all five passes on is split more often than the run with all five off while both
    succeed. It is not a tolerance: the test asserts > 0 and >."""
    fa, reads, names = READS
    small_on, split_on, st = map_under(fa, reads, names, SPLIT_ARENA, 1)
    small_off, split_off, _ = map_under(fa, reads, names, SPLIT_ARENA, 0)
    large_on, split_large, _ = map_under(fa, reads, names, 2 << 30, 1)
    for other in (small_off, large_on):
        assert small_on[0] == other[0] and all(np.array_equal(a, b) for a, b in zip(small_on[1:], other[1:]))
    assert len(small_on[1]) >= len(reads) - 4 and small_on[0].count(b"\tcs:Z:") >= len(reads) - 4
    # a final pass was split, not only the window calls: the passes are the only difference between the two small runs
    assert split_on[0] > 0 and split_on[0] > split_off[0] and split_on[1] > split_on[0], (split_on, split_off)
    assert split_large[0] == 0 and split_large[1] > 0, split_large
    for s in SWITCHES:
        assert st[s]["on_host"] == 0, (s, st[s])
    for s in ("fix", "eqx", "cs"):
        assert st[s]["on_device"] == st[s]["deferred"] - st[s].get("early_on_host", 0) > 0, (s, st[s])
