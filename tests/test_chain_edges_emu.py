"""The chain fill and the extraction at their edges, on the host wavefront emulator: every case of tests/chaincases.py (class sizes, the two density
rules, every chain parameter at its limits, hand-placed score edges) through every fill of seedchain_kernel.h — chain_wave with the 256- and the
1024-anchor window, chain_block on 8 wavefronts, chain_block_wide at 16 x 5, 8 x 10 and 16 x 3 tiles with 1 and KT tiles in an anchor's first step —
through win_small_wave, win_extract_wave (LDS and global) and win_plan_wave. The expectation is the oracle's mm_chain_dp (pinned to the reference on
the same cases by tests/test_oracle_vs_ref.py), looked at through the case's own min_cnt / min_sc and through the open observer (1, 0), which shows
the chain score of nearly every anchor. test_every_edge_value_matters is about the cases themselves: each edge value changes the oracle's output
against its neighbour on some case, so a kernel that is off by one there cannot pass."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import chaincases as CC
from winnowmap_amd import build
from test_kernels_emu import _load_emu

# (name, LDS window, wavefronts, tiles per wavefront and step, tiles in an anchor's first step)
FILLS = [("wave-256", 256, 0, 0, 0), ("wave-1024", 1024, 0, 0, 0), ("block-8", 4096, 8, 0, 0),
         ("wide-16x5", 4096, 16, 5, 5), ("wide-16x5-first1", 4096, 16, 5, 1), ("wide-8x10", 4096, 8, 10, 10), ("wide-8x10-first1", 4096, 8, 10, 1),
         ("wide-16x3", 4096, 16, 3, 3), ("wide-16x3-first1", 4096, 16, 3, 1)]
PRODUCTION = "wide-16x5"


@pytest.fixture(scope="module")
def emu():
    E = _load_emu()
    E.emu_chain_fill_geom.argtypes = [C.c_int64, W.u64p, W.u64p] + [C.c_int] * 6 + [C.c_float, C.c_float] + [C.c_int] * 5 + [W.i32p, W.i32p, W.i32p]
    E.emu_win_plan.argtypes = [C.c_int, W.u64p, W.u64p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    E.emu_win_extract.argtypes = [C.c_int, W.u64p, W.u64p, W.i32p, W.i32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), W.u64p]
    E.emu_win_small.argtypes = [C.c_int, C.c_int, C.c_int, W.u64p, W.u64p] + [C.c_int] * 8 + [C.c_float, C.POINTER(C.c_int), W.u64p]
    return E


@pytest.fixture(scope="module")
def host():
    H = C.CDLL(build.build_harness())
    H.h_chain_extract.restype = C.c_int64
    H.h_chain_extract.argtypes = [C.c_int64, W.u64p, W.u64p, W.i32p, W.i32p, W.i32p, C.c_int, C.c_int, C.POINTER(C.c_int), W.u64p, W.u64p, W.u64p]
    return H


_EXPECT = {}


def expected(c, p):
    """the oracle's (u, x, y) of case c under parameters p: computed once, shared by the tests of this module"""
    k = (c["name"], tuple(sorted(p.items())))
    if k not in _EXPECT:
        _EXPECT[k] = W.o_chain_dp(c["x"], c["y"], **p)
    return _EXPECT[k]


def same(a, b):
    return len(a[0]) == len(b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a, b))


def plan(E, c):
    avg, kl = C.c_float(), C.c_int()
    E.emu_win_plan(len(c["x"]), np.ascontiguousarray(c["x"]), np.ascontiguousarray(c["y"]), c["par"]["max_dist_x"], C.byref(avg), C.byref(kl))
    return avg.value, kl.value


def fill(E, c, win, nwv, kt, ktf):
    n, p = len(c["x"]), c["par"]
    f, pp, v = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = E.emu_chain_fill_geom(n, np.ascontiguousarray(c["x"]), np.ascontiguousarray(c["y"]), p["max_dist_x"], p["min_dist_x"], p["max_dist_y"], p["bw"], p["max_skip"], p["max_iter"],
                               plan(E, c)[0], p["gap_scale"], p["is_cdna"], win, nwv, kt, ktf, f, pp, v)
    assert rc == 0
    return f, pp, v


def host_extract(H, c, fpv, min_cnt, min_sc):
    n = len(c["x"])
    u, bx, by, nu = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_int()
    nv = H.h_chain_extract(n, np.ascontiguousarray(c["x"]), np.ascontiguousarray(c["y"]), fpv[0], fpv[1], fpv[2], min_cnt, min_sc, C.byref(nu), u, bx, by)
    return u[:nu.value], bx[:nv], by[:nv]


def heavy(c):
    """cases that take the emulator seconds per fill (thousands of predecessors per anchor): they run on the production geometry, and the 4096-anchor
    class edges on the fill their class launches; everything else runs everywhere"""
    return len(c["x"]) > 1500


def test_every_edge_value_matters():
    cases = CC.all_cases()
    for name, v, nb in CC.NEIGHBOURS:
        hit = 0
        for c in cases:
            if c["par"][name] != v:
                continue
            for p in CC.observers(c["par"])[:1 if name in ("min_cnt", "min_sc") else 2]:
                hit += not same(expected(c, p), expected(c, dict(p, **{name: nb})))
        assert hit > 0, (name, v, nb)
    # and what the cases say about themselves
    assert sorted(set(len(c["x"]) for c in cases if c["group"] == "size")) == list(CC.SIZES)
    c = [c for c in cases if c["name"] == "param-sparse-max_dist_y=0"][0]
    assert len(expected(c, dict(c["par"], **CC.OPEN))[0]) == len(c["x"]) and len(expected(c, c["par"])[0]) == 0      # f = span everywhere: every anchor a chain of its own
    for c in cases:
        assert np.all(c["x"][1:] >= c["x"][:-1]), c["name"]


def test_density_rules_as_the_kernels_state_them(emu):
    """the probe's figures on the density cases are what the case list says, the restated rules put each case on its side of both thresholds, and
    win_plan_wave (window_kernel.h) takes the class that the restated window rule takes — on every case of the list"""
    want = {"density-uniform-4500": (1, 0), "density-uniform-4505": (0, 0), "density-clustered-3200": (1, 1), "density-clustered-3225": (1, 0)}      # (wm_chain_batch, window)
    for c, worst, over in CC.density_edges():
        assert CC.probe(c["x"], c["par"]["max_dist_x"]) == (worst, over), c["name"]
        assert (CC.klass_chain_batch(c["x"], c["par"]["max_dist_x"]), CC.klass_window(c["x"], c["par"]["max_dist_x"])) == want[c["name"]], c["name"]
    seen = set()
    for c in CC.all_cases():
        kl = plan(emu, c)[1]
        assert kl == CC.klass_window(c["x"], c["par"]["max_dist_x"]), (c["name"], kl)
        kb = CC.klass_chain_batch(c["x"], c["par"]["max_dist_x"])
        seen.add((kl, kb))
        if c["group"] == "size" and len(c["x"]) > 1024:                   # sparse at every size, dense beyond 1024: by both rules
            assert kl == kb == (0 if "dense" in c["name"] else 1), c["name"]
    assert seen == {(0, 0), (0, 1), (1, 1), (2, 2), (3, 3)}, seen


@pytest.mark.parametrize("name,win,nwv,kt,ktf", FILLS, ids=[f[0] for f in FILLS])
def test_fill_matches_the_oracle_under_both_observers(emu, host, name, win, nwv, kt, ktf):
    n_run = 0
    for c in CC.all_cases():
        if heavy(c) and name != PRODUCTION and not (c["group"] == "size" and name == ("wave-1024" if "sparse" in c["name"] else "block-8")):
            continue
        fpv = fill(emu, c, win, nwv, kt, ktf)
        for p in CC.observers(c["par"]):
            assert same(host_extract(host, c, fpv, p["min_cnt"], p["min_sc"]), expected(c, p)), (name, c["name"], p["min_cnt"], p["min_sc"])
        n_run += 1
    assert n_run >= 100


def test_small_jobs_in_one_wavefront_match_the_oracle(emu):
    """win_small_wave: sort (nothing to do: handed-in anchors), fill and extraction of a job of at most 256 anchors in LDS"""
    n_run = 0
    for c in CC.all_cases():
        n = len(c["x"])
        if n > 256:
            continue
        for p in CC.observers(c["par"]):
            jx, jy = c["x"].copy(), c["y"].copy()
            u, nu = np.zeros(n, np.uint64), C.c_int()
            emu.emu_win_small_set_cdna(p["is_cdna"])
            try:
                nv = emu.emu_win_small(n, n, 0, jx, jy, p["max_dist_x"], p["min_dist_x"], p["max_dist_y"], p["bw"], p["max_skip"], p["max_iter"], p["min_cnt"], p["min_sc"],
                                       p["gap_scale"], C.byref(nu), u)
            finally:
                emu.emu_win_small_set_cdna(0)
            assert same((u[:nu.value], jx[:nv], jy[:nv]), expected(c, p)), (c["name"], p["min_cnt"], p["min_sc"])
            n_run += 1
    assert n_run >= 20


def test_extraction_in_lds_and_in_global_memory_under_every_observer(emu):
    """win_extract_wave on the fill's f and p (one fill per anchor set and fill parameters), for every min_cnt / min_sc of the case list"""
    n_run = 0
    fills = {}
    for c in CC.all_cases():
        if c["group"] not in ("param", "score") and not (c["group"] == "size" and len(c["x"]) in (1, 2, 64, 257, 4096, 4097)):
            continue
        n = len(c["x"])
        key = (c["x"].tobytes(), tuple(c["par"][k] for k in CC.FILL_KEYS))
        if key not in fills:
            fills[key] = fill(emu, c, 4096, 16, 5, 5) if n > 1024 else fill(emu, c, 1024, 0, 0, 0)
        f, pp, _ = fills[key]
        obs = CC.OBSERVERS if c["name"].endswith(("max_skip=25", "bw500")) or c["group"] == "size" else [(c["par"]["min_cnt"], c["par"]["min_sc"]), (1, 0)]
        for min_cnt, min_sc in obs:
            want = expected(c, dict(c["par"], min_cnt=min_cnt, min_sc=min_sc))
            for glob in (0, 1):
                bx, by = c["x"].copy(), c["y"].copy()
                u, nu = np.zeros(n, np.uint64), C.c_int()
                nv = emu.emu_win_extract(n, bx, by, f, pp, min_cnt, min_sc, glob, C.byref(nu), u)
                assert nv >= 0 and same((u[:nu.value], bx[:nv], by[:nv]), want), (c["name"], min_cnt, min_sc, glob)
                n_run += 1
    assert n_run >= 300
