"""GPU: the chain fill and the extraction at their edges — the cases of tests/chaincases.py (class sizes, both density rules, every chain parameter at
its limits, hand-placed score edges) through wm_chain_batch and, as handed-in anchors with each job's own parameters, through wm_window_batch; seeded
window jobs with a gap scale, the splice gap cost and a low min_cnt / min_sc; the dense fill in its other geometries (per call, and — where the switch is
read once per process — in a child process each); the bound CLI with the four chain options against the reference's. The expectation is the oracle's
mm_chain_dp (pinned to the reference on the same cases: tests/test_oracle_vs_ref.py), through the case's own min_cnt / min_sc and through the open
observer (1, 0). Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import chaincases as CC
import wmtest as W
from winnowmap_amd import gpu, parity
from test_aux_gpu import env, _windows, M128  # noqa: F401
from test_chain_edges_emu import expected, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_ref")
WM_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_wm")
CHILD = os.path.join(ROOT, "tests", "chain_edges_child.py")
PAR = np.dtype([("p", np.int32, 8), ("gs", np.float32), ("is_cdna", np.int32)])      # wm_chain_par_t (include/wm_gpu.h)
PAR_KEYS = ("max_dist_x", "min_dist_x", "max_dist_y", "bw", "max_skip", "max_iter", "min_cnt", "min_sc")
EMPTY = dict(name="empty", group="edge", x=np.zeros(0, np.uint64), y=np.zeros(0, np.uint64), par=CC.par())


def jobs_of(cases):
    """every case under both observers, as (case, parameters)"""
    return [(c, p) for c in cases for p in CC.observers(c["par"])]


def want(c, p):
    return expected(c, p) if len(c["x"]) else (np.zeros(0, np.uint64),) * 3


def chain_batch(ctx, jobs):
    """one wm_chain_batch call over (case, parameters) jobs -> [(u, x, y)]"""
    L = gpu.lib()
    L.wm_chain_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, W.u64p, W.i32p, C.c_void_p, W.u64p, W.u64p, W.i32p, W.i32p]
    n = len(jobs)
    na = np.array([len(c["x"]) for c, _ in jobs], np.int32)
    aoff = np.concatenate([[0], np.cumsum(na)[:-1]]).astype(np.uint64)
    a = np.zeros(int(na.sum()) + 1, M128)
    par = np.zeros(n, PAR)
    for i, (c, p) in enumerate(jobs):
        a["x"][int(aoff[i]):int(aoff[i]) + na[i]] = c["x"]; a["y"][int(aoff[i]):int(aoff[i]) + na[i]] = c["y"]
        par[i]["p"] = [p[k] for k in PAR_KEYS]; par[i]["gs"] = p["gap_scale"]; par[i]["is_cdna"] = p["is_cdna"]
    u = np.zeros(len(a) + 1, np.uint64); uoff = np.zeros(n, np.uint64); nu = np.zeros(n, np.int32); nv = np.zeros(n, np.int32)
    assert L.wm_chain_batch(ctx._h, n, a.ctypes.data, aoff, na, par.ctypes.data, u, uoff, nu, nv) == 0, L.wm_last_error()
    return [(u[int(uoff[i]):int(uoff[i]) + nu[i]], a["x"][int(aoff[i]):int(aoff[i]) + nv[i]], a["y"][int(aoff[i]):int(aoff[i]) + nv[i]]) for i in range(n)]


def window_batch(ctx, jobs):
    """one wm_window_batch call over (case, parameters) jobs, the anchors handed in (seq_off = -2: the job's anchors are exactly these, in this order)
    -> (results, [(u, x, y)], chains in the pool, anchors in the pool)"""
    n = len(jobs)
    J = np.zeros(n, gpu.WINDOW_JOB)
    na = [len(c["x"]) for c, _ in jobs]
    pre = np.zeros((sum(na) + 1, 2), np.uint64)
    pos = 0
    for i, (c, p) in enumerate(jobs):
        J[i]["seq_off"], J[i]["pre_off"], J[i]["n_pre"] = -2, pos, na[i]
        for k in PAR_KEYS + ("gap_scale", "is_cdna"):
            J[i][k] = p[k]
        pre[pos:pos + na[i], 0] = c["x"]; pre[pos:pos + na[i], 1] = c["y"]
        pos += na[i]
    res, up, ap = ctx.window_batch_keyed(J, None, np.zeros(8, np.uint8), pre, 5000, 0, sum(na) + 64, sum(na) + 64)
    out = [(up[int(r["u_off"]):int(r["u_off"]) + int(r["n_u"])], ap[int(r["a_off"]):int(r["a_off"]) + int(r["n_v"]), 0], ap[int(r["a_off"]):int(r["a_off"]) + int(r["n_v"]), 1]) for r in res]
    return res, out, len(up), len(ap)


def mixed_cases():
    """all cases, with an empty job and the one-anchor job behind each of the largest ones"""
    cases = CC.all_cases()
    one = [c for c in cases if len(c["x"]) == 1][0]
    out = []
    for c in cases:
        out.append(c)
        if len(c["x"]) >= 4096:
            out += [EMPTY, one]
    return out


def check(jobs, got, what):
    bad = [(c["name"], p["min_cnt"], p["min_sc"]) for (c, p), g in zip(jobs, got) if not same(g, want(c, p))]
    assert not bad, (what, len(bad), bad[:8])


def test_chain_batch_on_every_case_in_one_mixed_call(env):
    """wm_chain_batch: all four classes launch from one call — chain_kernel with W = 256 and 1024, the one-wavefront kernel with the wrapping window, the
    dense fill — with empty and one-anchor jobs between the large ones"""
    ctx = env[0]
    jobs = jobs_of(mixed_cases())
    assert {CC.klass_chain_batch(c["x"], p["max_dist_x"]) for c, p in jobs} == {0, 1, 2, 3}
    check(jobs, chain_batch(ctx, jobs), "wm_chain_batch")


def test_window_batch_on_every_case_with_each_jobs_own_parameters(env):
    """wm_window_batch on handed-in anchors: win_small_kernel (n <= 256), win_plan_wave's classes (its own dense rule included), the fills, both
    win_extract_kernel launches (LDS up to 4096 anchors, global beyond) — n_anchors, n_u, n_v, the chains, their anchors and the pool totals"""
    ctx = env[0]
    jobs = jobs_of(mixed_cases())
    assert {CC.klass_window(c["x"], p["max_dist_x"]) for c, p in jobs} == {0, 1, 2, 3}
    assert {(CC.klass_window(c["x"], p["max_dist_x"]), CC.klass_chain_batch(c["x"], p["max_dist_x"])) for c, p in jobs} >= {(0, 1)}      # dense by the window's rule alone
    res, got, n_up, n_ap = window_batch(ctx, jobs)
    for (c, p), r in zip(jobs, res):
        assert r["n_anchors"] == len(c["x"]) and r["n_mini"] == 0 and r["rep_len"] == 0, (c["name"], r)
    check(jobs, got, "wm_window_batch")
    assert n_up == int(res["n_u"].sum()) == sum(len(want(c, p)[0]) for c, p in jobs) and n_ap == int(res["n_v"].sum()) == sum(len(want(c, p)[1]) for c, p in jobs)


def test_seeded_window_jobs_with_gap_scale_splice_cost_and_a_low_threshold(env):
    """sequences through the whole call (sketch, seeds, sort, fill, extraction) with gap_scale = 0.8, is_cdna = 1 and min_cnt / min_sc = (1, 10): stage by
    stage as tests/test_window_gpu.py expects them"""
    from test_window_gpu import expected_seeds
    ctx, idx, ref, bloom, L = env
    seqs = _windows(ref)[::9]
    J = np.zeros(len(seqs), gpu.WINDOW_JOB)
    prm = []
    spos = 0
    for i, s in enumerate(seqs):
        p = CC.par(CC.STAGE2 if i % 2 else CC.DEFAULT, gap_scale=0.8 if i % 3 != 1 else 1.0, is_cdna=int(i % 3 != 0), min_cnt=1 if i % 4 != 3 else 3, min_sc=10 if i % 4 != 3 else 40)
        prm.append(p)
        J[i]["seq_off"], J[i]["stage_off"], J[i]["len"] = -1, spos, len(s)
        spos += len(s)
        for k in PAR_KEYS + ("gap_scale", "is_cdna"):
            J[i][k] = p[k]
    res, up, ap = ctx.window_batch_keyed(J, None, np.concatenate(seqs), np.zeros((1, 2), np.uint64), 5000, 0, 1 << 18, 1 << 20)
    n_chained = n_changed = 0
    for i, s in enumerate(seqs):
        mx, my = W.o_sketch(bytes(s), 50, 15, rid=0, bloom=bloom)
        ex, ey, rep = expected_seeds(L, idx, s, mx, my)
        sx, sy = W.o_radix_sort_128x(ex, ey)
        r = res[i]
        assert r["n_anchors"] == len(sx) and r["rep_len"] == rep and r["n_mini"] == len(mx), (i, r, len(sx), rep, len(mx))
        ou, obx, oby = W.o_chain_dp(sx, sy, **prm[i]) if len(sx) else (np.zeros(0, np.uint64),) * 3
        gu = up[int(r["u_off"]):int(r["u_off"]) + int(r["n_u"])]
        ga = ap[int(r["a_off"]):int(r["a_off"]) + int(r["n_v"])]
        assert same((gu, ga[:, 0], ga[:, 1]), (ou, obx, oby)), (i, len(sx), prm[i], r)
        n_chained += len(ou) > 0
        n_changed += len(sx) > 0 and not same((ou, obx, oby), W.o_chain_dp(sx, sy, **CC.par(prm[i], gap_scale=1.0, is_cdna=0, min_cnt=3, min_sc=40)))
    assert n_chained >= 15 and n_changed >= 10, (n_chained, n_changed)      # (the non-default parameters decide the expectation: the defaults would not pass)


def dense_jobs():
    return jobs_of([c for c in CC.all_cases() if CC.klass_chain_batch(c["x"], c["par"]["max_dist_x"]) == 0 and (c["group"] != "size" or len(c["x"]) in (1025, 4097, 4160))])


@pytest.mark.parametrize("switches", [{"WM_CHAIN_WIDE_GEOM": "8x10"}, {"WM_CHAIN_WIDE_GEOM": "16x3"}, {"WM_CHAIN_WIDE_FIRST": "1"}, {"WM_CHAIN_WIDE_GEOM": "8x10", "WM_CHAIN_WIDE_FIRST": "1"}],
                         ids=["8x10", "16x3", "first1", "8x10-first1"])
def test_dense_fill_in_its_other_geometries(env, monkeypatch, switches):
    """chain_block_wide<10> on 8 wavefronts, <3> on 16, and one tile per wavefront in an anchor's first step (wm_chain_batch reads these per call), on the
    dense cases — the 7000-anchor one, whose windows take a second step at 16 x 5 and 8 x 10 and a third at 16 x 3, among them"""
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    jobs = dense_jobs()
    assert len(jobs) >= 80 and any(c["group"] == "wide2" for c, _ in jobs)
    check(jobs, chain_batch(env[0], jobs), switches)


_child_fault = []


@pytest.mark.parametrize("mode,switches", [("chain+window", {"WM_CHAIN_WIDE": "0"}), ("window", {"WM_CHAIN_WIDE_FIRST": "1"})], ids=["wide0", "window-first1"])
def test_fill_switches_read_once_per_process(mode, switches):
    """WM_CHAIN_WIDE=0 (chain_block on 8 wavefronts: the fill before chain_block_wide, still shipped) in both calls, and the window call's
    WM_CHAIN_WIDE_FIRST: a fresh process each (tests/chain_edges_child.py), which prints its verdict"""
    assert not _child_fault, "an earlier child process faulted or timed out (%s): no further one is started" % _child_fault
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, CHILD, mode], env=dict(os.environ, **switches), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = p.stdout.decode(errors="replace")
    if p.returncode not in (0, 1):
        _child_fault.append((mode, p.returncode))
    assert p.returncode == 0, (p.returncode, out[-1500:], p.stderr.decode(errors="replace")[-1500:])
    verdict = [l for l in out.splitlines() if l.startswith("VERDICT")]
    assert verdict and verdict[-1].startswith("VERDICT ok") and ("jobs=%d" % len(dense_jobs())) in verdict[-1], verdict


def _run(binary, args):
    p = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stdout


@pytest.mark.skipif(not (os.path.exists(REF_BIN) and os.path.exists(WM_BIN)), reason="oracle/_ref/winnowmap_ref / winnowmap_wm not built")
def test_bound_cli_with_the_chain_options_prints_what_the_reference_prints():
    import sdustcases as S
    tmp = tempfile.mkdtemp()
    fa, rq = S.e2e_inputs(tmp)
    args = ["-t", "4", "-cx", "map-ont", fa, rq]
    opts = ["--max-chain-skip", "1", "--max-chain-iter", "50", "-n", "2", "-m", "20"]
    plain = _run(REF_BIN, args)
    ref_out = _run(REF_BIN, opts + args)
    d0 = parity.diff_texts(plain, ref_out, sam=False)
    assert d0["reads"] == 60 and d0["mismatches"] >= 20, d0            # the options change the reference's own output on these reads
    got = _run(WM_BIN, opts + args)
    d = parity.diff_texts(ref_out, got, sam=False)
    assert d["reads"] == 60 and d["hits"] >= 55 and d["mismatches"] == 0, d
    assert sorted(parity.group_by_read(got).items()) == sorted(parity.group_by_read(ref_out).items())      # every record, every column and tag (parity.py on what is masked)
