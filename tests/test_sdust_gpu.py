"""GPU: the -T filter. (a) wm_sdust_batch against the reference's own sdust() (src/sdust.c:166, W = 64) on the case list of tests/sdustcases.py;
(b) the window call with the threshold against sketch -> mm_dust_minier restated (sdustcases.restated_filter over the reference's intervals) -> the
seeding entry on the squeezed list -> the oracle's chaining; (c) the reference's CLI bound to the library with -T 20 against the reference with -T 20;
(d) threshold 0 through the new entry is the old entry. Every comparison is exact."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import sdustcases as S
import wmtest as W
from winnowmap_amd import gpu, parity
from test_aux_gpu import env, M128  # noqa: F401
from test_sdust_emu import ref_sdust  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not W.have_ref(), reason="oracle/_ref not built")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_ref")
WM_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_wm")
PAR = (5000, 1000, 5000, 500, 25, 5000, 3, 40)


@pytest.fixture(scope="module")
def cases():
    seqs = [c for _, c in S.named_cases()] + [S.mixture(s) for s in range(S.N_MIXTURES)] + [S.long_case()]
    return [np.ascontiguousarray(s, np.uint8) for s in seqs]


def _pairs(a):
    return [(int(p[0]), int(p[1])) for p in a]


@pytest.mark.parametrize("T", S.THRESHOLDS)
def test_sdust_batch_equals_the_reference(env, cases, ref_sdust, T):  # noqa: F811
    ctx = env[0]
    lens = np.array([len(s) for s in cases], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    flat = np.concatenate(cases)
    want = [ref_sdust(s, T) for s in cases]
    got, high = ctx.sdust_batch(flat, off, lens, T)
    for i in range(len(cases)):
        assert _pairs(got[i]) == want[i], ("staged", i, len(cases[i]), T, _pairs(got[i])[:4], want[i][:4])
    # the same bases as resident packed reads (every second sequence; the others stay staged)
    ctx.reads_upload(flat)
    res = (np.arange(len(cases)) & 1).astype(np.uint8)
    got2, high2 = ctx.sdust_batch(flat, off, lens, T, resident=res)
    for i in range(len(cases)):
        assert _pairs(got2[i]) == want[i], ("resident" if res[i] else "staged", i, len(cases[i]), T)
    assert np.array_equal(high, high2)
    assert sum(len(w) for w in want) > 500 and int(high.max()) <= 4096 and (T != 20 or int(high.max()) > 1000), int(high.max())
    print("T=%d: %d intervals, largest list of perfect intervals %d, kernel %.2f ms" % (T, sum(len(w) for w in want), int(high.max()), gpu.lib().wm_last_aux_ms(ctx._h)))


def test_sdust_batch_list_overflow_is_finished_by_the_host(env, cases, ref_sdust, monkeypatch):  # noqa: F811
    """WM_SDUST_CAP=64 shrinks the wavefront's list: the sequences that need more are finished by the host restatement"""
    ctx = env[0]
    sub = cases[:80]
    lens = np.array([len(s) for s in sub], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    before = gpu.sdust_stats()["host_jobs"]
    monkeypatch.setenv("WM_SDUST_CAP", "64")
    got, high = ctx.sdust_batch(np.concatenate(sub), off, lens, 20)
    monkeypatch.delenv("WM_SDUST_CAP")
    for i in range(len(sub)):
        assert _pairs(got[i]) == ref_sdust(sub[i], 20), (i, len(sub[i]))
    assert gpu.sdust_stats()["host_jobs"] - before >= 3 and int(high.max()) > 1000


def _per_job(out):
    """a window call's results job by job: the counts, the chains and their anchors as bytes. (Where a job's chains lie in the two dense pools is the
    order in which the jobs' wavefronts took their room — it differs from call to call — so calls are compared job by job, not pool by pool.)"""
    res, up, ap = out
    return [(int(r["n_anchors"]), int(r["rep_len"]), int(r["n_mini"]), up[int(r["u_off"]):int(r["u_off"]) + int(r["n_u"])].tobytes(),
             ap[int(r["a_off"]):int(r["a_off"]) + int(r["n_v"])].tobytes()) for r in res]


def _window_jobs(ref):
    """windows over a read with implanted runs — staged and resident — plus windows that are nothing but a run (no minimizer survives) and a short one"""
    rng = np.random.default_rng(12)
    seqs = []
    for r in range(10):
        st = int(rng.integers(0, len(ref[0]) - 9000))
        s = ref[r % len(ref)][st:st + 6000].copy()
        for _ in range(int(rng.integers(1, 5))):
            p, n = int(rng.integers(0, 5500)), int(rng.integers(30, 500))
            s[p:p + n] = S.unit_run(rng, S.rnd(rng, int(rng.integers(1, 4))), len(s[p:p + n]), 0.02)
        if r % 3 == 0:
            s[int(rng.integers(0, len(s)))] = 4
        seqs += [s[a:a + 2000].copy() for a in (0, 2000, 4000)] + [s]
    seqs += [S.unit_run(rng, (0, 3), 1500), S.unit_run(rng, (1,), 700, 0.01), S.rnd(rng, 40), S.p_list_stress(rng)]
    return [np.ascontiguousarray(s, np.uint8) for s in seqs]


def _expected(ctx, L, idx, bloom, seqs, iv_of, max_occ, T):
    out = []
    for s in seqs:
        mx, my = W.o_sketch(bytes(s), 50, 15, rid=0, bloom=bloom)
        keep = S.restated_filter(mx, my, iv_of(s, T)) if T > 0 else list(range(len(mx)))
        out.append((mx[keep], my[keep]))
    nm = np.array([len(m[0]) for m in out], np.int32)
    moff = np.concatenate([[0], np.cumsum(nm)[:-1]]).astype(np.uint64)
    allm = np.zeros((max(1, int(nm.sum())), 2), np.uint64)
    for i, (mx, my) in enumerate(out):
        allm[int(moff[i]):int(moff[i]) + len(mx), 0] = mx
        allm[int(moff[i]):int(moff[i]) + len(mx), 1] = my
    qlen = np.array([len(s) for s in seqs], np.int32)
    anchors, ooff, na, rl = ctx.seed_batch_keyed(allm, moff, nm, qlen, None, max_occ, 0, 1 << 21)      # today's seeding on the squeezed lists
    return nm, anchors, ooff, na, rl


def test_window_batch_with_threshold(env, ref_sdust):  # noqa: F811
    ctx, idx, ref, bloom, L = env
    seqs = _window_jobs(ref)
    n_w = len(seqs)
    flat = np.concatenate(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])[:-1]])
    ctx.reads_upload(flat)
    J = np.zeros(2 * n_w, gpu.WINDOW_JOB)
    for i, s in enumerate(seqs):
        for q, (so, sto) in enumerate(((-1, int(off[i])), (int(off[i]), 0))):       # staged, then resident
            j = J[2 * i + q]
            j["seq_off"], j["stage_off"], j["len"] = so, sto, len(s)
            (j["max_dist_x"], j["min_dist_x"], j["max_dist_y"], j["bw"], j["max_skip"], j["max_iter"], j["min_cnt"], j["min_sc"]), j["gap_scale"] = PAR, 1.0
    T, max_occ = 20, 5000
    nm, anchors, ooff, na, rl = _expected(ctx, L, idx, bloom, seqs, ref_sdust, max_occ, T)
    nm0 = _expected(ctx, L, idx, bloom, seqs, ref_sdust, max_occ, 0)[0]
    assert int((nm0 - nm).sum()) > 100 and int((nm == 0).sum()) >= 2 and int(((nm > 0) & (nm < nm0)).sum()) >= 10, (nm0, nm)
    res, up, ap = ctx.window_batch_dust(J, None, flat, np.zeros((1, 2), np.uint64), max_occ, 0, T, 1 << 20, 1 << 21)
    n_chained = 0
    for i in range(n_w):
        a = anchors[int(ooff[i]):int(ooff[i]) + int(na[i])]
        ou, obx, oby = W.o_chain_dp(a[:, 0].copy(), a[:, 1].copy(), max_dist_x=PAR[0], min_dist_x=PAR[1], max_dist_y=PAR[2], bw=PAR[3]) if len(a) else (np.zeros(0, np.uint64),) * 3
        for q in (0, 1):
            r = res[2 * i + q]
            assert r["n_mini"] == nm[i] and r["n_anchors"] == na[i] and r["rep_len"] == rl[i], (i, q, len(seqs[i]), r, nm[i], na[i], rl[i])
            gu = up[int(r["u_off"]):int(r["u_off"]) + int(r["n_u"])]
            ga = ap[int(r["a_off"]):int(r["a_off"]) + int(r["n_v"])]
            assert np.array_equal(gu, ou) and np.array_equal(ga[:, 0], obx) and np.array_equal(ga[:, 1], oby), (i, q, len(a))
        n_chained += int(len(ou) > 0)
    assert n_chained >= 20
    # the wavefront's list shrunk to 64 entries: the jobs that need more are finished by the host, the call's results are the same
    before = gpu.sdust_stats()["host_jobs"]
    os.environ["WM_SDUST_CAP"] = "64"
    try:
        res2, up2, ap2 = ctx.window_batch_dust(J, None, flat, np.zeros((1, 2), np.uint64), max_occ, 0, T, 1 << 20, 1 << 21)
    finally:
        del os.environ["WM_SDUST_CAP"]
    assert gpu.sdust_stats()["host_jobs"] - before >= 2
    assert _per_job((res2, up2, ap2)) == _per_job((res, up, ap)) and len(up2) == len(up) and len(ap2) == len(ap)


def test_threshold_zero_is_the_old_entry(env):  # noqa: F811
    ctx, idx, ref, bloom, L = env
    seqs = _window_jobs(ref)[:12]
    flat = np.concatenate(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])[:-1]])
    J = np.zeros(len(seqs), gpu.WINDOW_JOB)
    for i, s in enumerate(seqs):
        j = J[i]
        j["seq_off"], j["stage_off"], j["len"] = -1, int(off[i]), len(s)
        (j["max_dist_x"], j["min_dist_x"], j["max_dist_y"], j["bw"], j["max_skip"], j["max_iter"], j["min_cnt"], j["min_sc"]), j["gap_scale"] = PAR, 1.0
    calls = gpu.sdust_stats()["window_calls"]
    a = ctx.window_batch_keyed(J, None, flat, np.zeros((1, 2), np.uint64), 5000, 0, 1 << 20, 1 << 21)
    b = ctx.window_batch_dust(J, None, flat, np.zeros((1, 2), np.uint64), 5000, 0, 0, 1 << 20, 1 << 21)
    assert _per_job(a) == _per_job(b) and len(a[1]) == len(b[1]) and len(a[2]) == len(b[2]) and int(a[0]["n_u"].sum()) > 0      # every job's bytes
    assert gpu.sdust_stats()["window_calls"] == calls                   # nothing more was launched
    c = ctx.window_batch_dust(J, None, flat, np.zeros((1, 2), np.uint64), 5000, 0, 20, 1 << 20, 1 << 21)
    assert [j[:3] for j in _per_job(c)] != [j[:3] for j in _per_job(a)] and gpu.sdust_stats()["window_calls"] == calls + 1


def _run(binary, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stdout, p.stderr


@pytest.mark.skipif(not (os.path.exists(REF_BIN) and os.path.exists(WM_BIN)), reason="oracle/_ref/winnowmap_ref / winnowmap_wm not built")
def test_bound_cli_with_T_prints_what_the_reference_prints():
    tmp = tempfile.mkdtemp()
    fa, rq = S.e2e_inputs(tmp)
    args = ["-t", "4", "-cx", "map-ont", fa, rq]
    plain = _run(REF_BIN, args)[0]
    want = _run(REF_BIN, ["-T", "20"] + args)[0]
    d0 = parity.diff_texts(plain, want, sam=False)
    assert d0["reads"] == 60 and d0["mismatches"] >= 30, d0            # the option changes the reference's own output on these reads
    got, err = _run(WM_BIN, ["-T", "20"] + args, env={"WM_SDUST_REPORT": "1"})
    d = parity.diff_texts(want, got, sam=False)
    assert d["reads"] == 60 and d["hits"] >= 55 and d["mismatches"] == 0, d
    print(b"\n".join(l for l in err.split(b"\n") if b"sdust" in l).decode(errors="replace"))
