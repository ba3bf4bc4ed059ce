"""GPU parity at the sizes and scores where the ksw routing changes hands (winnowmap_amd/csrc/ksw_plan.h): jobs either side of every class edge, tlen / qlen /
band at the stripe ends of the chained-workgroup kernel, the 4096-row hand-over of the 8-pair class, the scoring sets up to the limit wm_ksw_score_ok admits —
under every routing the library offers, bit-exact against the oracle (which tests/test_oracle_vs_ref.py pins to the reference on these very generators), and
with the context's per-class launch counters as the proof that the intended kernel ran."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import wmtest as W
import kswcases
from winnowmap_amd import gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 4 << 30)
    yield c
    c.close()


def _library_default_routing():
    """what the library chooses by itself (wm_ksw.hip: chain_mode, stripe_min_rows)"""
    gpu.set_ksw_chain_routing(int(os.environ.get("WM_KSW_CHAIN", 1)) & 7, int(os.environ.get("WM_KSW_CHAIN_ROWS", 2048)), 4 if os.environ.get("WM_KSW_CHAIN_BP") == "4" else 2)
    w16 = int(os.environ.get("WM_KSW_STRIPE16", 1)) & 3
    on = 0 if os.environ.get("WM_KSW_STRIPE") == "0" else 3 if w16 == 0 else 2 if w16 >= 2 else 1
    gpu.set_ksw_routing(on, int(os.environ.get("WM_KSW_STRIPE_ROWS4", 0)), int(os.environ.get("WM_KSW_STRIPE_ROWS8", 4096)))


@pytest.fixture(autouse=True)
def restore_routing():
    """the routing is process-global: every test sets its own and leaves the library's default behind"""
    yield
    _library_default_routing()


# (chain mode, rows from which exact 8-pair extensions are chained, pairs per chained wavefront), (stripe mode, ROWS4, ROWS8): wm_ksw_set_chain_routing, wm_ksw_set_routing
ROUTINGS = {
    "default": ((1, 2048, 2), (1, 0, 4096)),            # the library's: wide and long jobs on the chained kernels, 256-lane stripes
    "bp4": ((1, 2048, 4), (1, 0, 4096)),                # ... 512-lane stripes
    "chain_off": ((0, 2048, 2), (1, 0, 4096)),          # the route-around the watchdog's error text recommends: the stripe kernels, <2,16> for 1793..3840 lanes
    "no16": ((0, 2048, 2), (3, 0, 4096)),               # ... without the sixteen-wavefront geometries: <4,8> and <8,8> there (only here is 3584 an edge)
    "both_off": ((0, 2048, 2), (0, 0, 4096)),           # the 16-pair classes, BLOCK / BLOCK2 (ksw_pmulti_kernel) and BLOCK3 (ksw_block_kernel)
}


def set_routing(name):
    chain, stripe = ROUTINGS[name]
    gpu.set_ksw_chain_routing(*chain)
    gpu.set_ksw_routing(*stripe)


def family(k):
    """the kernel family of a class id (the enum of ksw_plan.h), without its CLIP / HASN / EXACT instantiation"""
    if k < 24:
        return ("P4", "P8", "P16")[k >> 3]
    if k < 28:
        return ("BLOCK", "BLOCK2", "BLOCK3", "GENERIC")[k - 24]
    if k < 52:
        return "S" + ("<2,4>", "<2,8>", "<4,8>", "<8,8>", "<1,16>", "<2,16>")[(k - 28) >> 2]
    return "C%d" % (2, 4)[(k - 52) >> 2]


S24, S28, S48, S88, S216 = "S<2,4>", "S<2,8>", "S<4,8>", "S<8,8>", "S<2,16>"
# edge -> routing -> families of the jobs with n_col == edge, families of those with n_col == edge + 16. Derived from ksw_plan.h:
#   wm_ksw_classify: n_col <= 496 P4, <= 1008 P8, <= 2032 P16, <= 4080 BLOCK, <= 8176 BLOCK2, else BLOCK3
#   wm_ksw_route (stripe kernels on): P8 from ROWS8 = 4096 rows on -> <2,4> up to 768, else <2,8>; everything from P16 on -> <2,8> up to 1792, <4,8> up to
#     3584, <8,8> up to 7168, beyond that it keeps its class; with the sixteen-wavefront geometries <2,16> replaces them for 1793 .. 3840
#   wm_ksw_route_chain (mode 1): everything from P16 on, stripe classes included -> the chained kernel
# Of the jobs of edge 768 two have 4096 rows and more (kswcases.class_edge_cases), all others are shorter.
EDGE_FAMILIES = {
    496: dict(default=("P4", "P8"), bp4=("P4", "P8"), chain_off=("P4", "P8"), no16=("P4", "P8"), both_off=("P4", "P8")),
    768: dict(default=("P8 C2", "P8 C2"), bp4=("P8 C4", "P8 C4"), chain_off=("P8 " + S24, "P8 " + S28), no16=("P8 " + S24, "P8 " + S28), both_off=("P8", "P8")),
    1008: dict(default=("P8", "C2"), bp4=("P8", "C4"), chain_off=("P8", S28), no16=("P8", S28), both_off=("P8", "P16")),
    1792: dict(default=("C2", "C2"), bp4=("C4", "C4"), chain_off=(S28, S216), no16=(S28, S48), both_off=("P16", "P16")),
    2032: dict(default=("C2", "C2"), bp4=("C4", "C4"), chain_off=(S216, S216), no16=(S48, S48), both_off=("P16", "BLOCK")),
    3584: dict(default=("C2", "C2"), bp4=("C4", "C4"), chain_off=(S216, S216), no16=(S48, S88), both_off=("BLOCK", "BLOCK")),
    3840: dict(default=("C2", "C2"), bp4=("C4", "C4"), chain_off=(S216, S88), no16=(S88, S88), both_off=("BLOCK", "BLOCK")),
    4080: dict(default=("C2", "C2"), bp4=("C4", "C4"), chain_off=(S88, S88), no16=(S88, S88), both_off=("BLOCK", "BLOCK2")),
    7168: dict(default=("C2", "C2"), bp4=("C4", "C4"), chain_off=(S88, "BLOCK2"), no16=(S88, "BLOCK2"), both_off=("BLOCK2", "BLOCK2")),
    8176: dict(default=("C2", "C2"), bp4=("C4", "C4"), chain_off=("BLOCK2", "BLOCK3"), no16=("BLOCK2", "BLOCK3"), both_off=("BLOCK2", "BLOCK3")),
}


def test_every_edge_changes_hands_in_some_routing():
    for E, per in EDGE_FAMILIES.items():
        assert any(lo != hi for lo, hi in per.values()), E


# ---- cases and expectations: made once per module, shared by the routings ----
@functools.lru_cache(maxsize=None)
def edge_cases(edges, si):
    return kswcases.class_edge_cases(60 + si, edges, kswcases.SCORING_EDGE[si])


@functools.lru_cache(maxsize=None)
def stripe_end_cases(sw, si):
    return kswcases.chain_stripe_edge_cases(70 + si, sw, kswcases.SCORING_EDGE[si])


@functools.lru_cache(maxsize=None)
def row_cases():
    return kswcases.row_threshold_cases(80)


def _oracle(c):
    return W.o_ksw_extd2(c["q"], c["t"], mat=W.simple_mat(c["a"], c["b"], 1), q=c["q_"], e=c["e"], q2=c["q2"], e2=c["e2"],
                         w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flag=c["flag"])


def expectations(cases):
    """the oracle's results, computed once per job (eight at a time: ctypes releases the GIL) and kept on the job"""
    todo = [c for c in cases if "_o" not in c]
    if todo:
        W.oracle()
        with ThreadPoolExecutor(8) as ex:
            for c, o in zip(todo, ex.map(_oracle, todo)):
                c["_o"] = o
    return [c["_o"] for c in cases]


def run_batch(ctx, cases):
    """one call (one scoring set) -> (jobs that differ from the oracle, families of the classes it launched)"""
    c0 = cases[0]
    sc = gpu.KswScore(c0["a"], -c0["b"], -1, c0["q_"], c0["e"], c0["q2"], c0["e2"])
    jobs, seqs = gpu.pack_jobs([(c["q"], c["t"], dict(w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flag=c["flag"])) for c in cases])
    exp = expectations(cases)
    s0 = ctx.kernel_stats()
    res, pool = ctx.ksw_batch(sc, jobs, seqs)
    s1 = ctx.kernel_stats()
    bad = []
    for i, (c, o) in enumerate(zip(cases, exp)):
        g = res[i]
        cig = pool[g["cig_off"]:g["cig_off"] + g["n_cigar"]]
        if not (all(int(g[k]) == o[k] for k in W.EZ_FIELDS) and np.array_equal(cig, o["cigar"])):
            bad.append((i, len(c["q"]), len(c["t"]), c["w"], hex(c["flag"]), c["zdrop"], {k: (int(g[k]), o[k]) for k in W.EZ_FIELDS if int(g[k]) != o[k]},
                        W.cigar_str(cig)[:50], W.cigar_str(o["cigar"])[:50]))
    return bad, {family(k) for k in s1 if s1[k][2] > s0[k][2]}


@pytest.mark.parametrize("edge", kswcases.CLASS_EDGES)
@pytest.mark.parametrize("routing", sorted(ROUTINGS))
def test_both_sides_of_a_class_edge(ctx, routing, edge):
    """map-ont scoring: the jobs with n_col == edge and those with n_col == edge + 16 as a call each — the results, and that each call launched exactly the
    kernel families ksw_plan.h sends it to under this routing"""
    set_routing(routing)
    cases = edge_cases((edge,), 0)
    for n_col, want in zip((edge, edge + 16), EDGE_FAMILIES[edge][routing]):
        side = [c for c in cases if c["n_col"] == n_col]
        assert len(side) >= 2
        bad, ran = run_batch(ctx, side)
        assert not bad, (n_col, bad[:3])
        assert ran == set(want.split()), (n_col, ran, want)


@pytest.mark.parametrize("si", range(1, len(kswcases.SCORING_EDGE)))
@pytest.mark.parametrize("routing", ["default", "bp4", "chain_off", "both_off"])
def test_class_edges_under_every_scoring_set(ctx, routing, si):
    """the edges up to 2032 and the two unbanded gap fills either side of 4080 under asm5's wrapping penalties, asm10, the two sets on the limit
    (q+e)+(q2+e2) == 127 and a large match score: one call per set"""
    set_routing(routing)
    cases = edge_cases((496, 768, 1008, 1792, 2032), si) + edge_cases((4080,), si)[::2]
    bad, ran = run_batch(ctx, cases)
    assert not bad, bad[:3]
    want = set(" ".join(" ".join(EDGE_FAMILIES[E][routing]) for E in (496, 768, 1008, 1792, 2032, 4080)).split())
    assert ran == want, (ran, want)


@pytest.mark.parametrize("si", range(len(kswcases.SCORING_EDGE)))
@pytest.mark.parametrize("bp", [2, 4])
def test_stripe_ends_of_the_chained_kernel(ctx, bp, si):
    """every job on the chained-workgroup kernel (mode 4), tlen / qlen / band at the ends of its 128 * bp-lane stripes, under each scoring set"""
    gpu.set_ksw_chain_routing(4, 1, bp)
    bad, ran = run_batch(ctx, stripe_end_cases(128 * bp, si))
    assert not bad, bad[:3]
    assert ran == {"C%d" % bp}, ran


@pytest.mark.parametrize("routing", ["default", "chain_off"])
def test_the_row_count_at_which_a_long_job_leaves_its_wavefront(ctx, routing):
    """4095 rows stay on the 8-pair register class, 4096 and 4097 go to four stripe wavefronts, and from there (by default) to the chained kernel"""
    set_routing(routing)
    for rows in (4095, 4096, 4097):
        bad, ran = run_batch(ctx, [c for c in row_cases() if c["rows"] == rows])
        assert not bad, (rows, bad[:3])
        assert ran == {"P8" if rows < 4096 else "C2" if routing == "default" else S24}, (rows, ran)


def test_scoring_under_which_a_mismatch_can_never_be_seen(ctx):
    """src/ksw2_extd2_sse.c:92: the reference returns at once; every job is degenerate, none is launched, the results are the untouched ez"""
    set_routing("default")
    sc = (1, 30, 4, 2, 24, 1)
    cases = kswcases.class_edge_cases(7, (496,), sc) + kswcases.chain_stripe_edge_cases(8, 256, sc)[::5]
    bad, ran = run_batch(ctx, cases)
    assert not bad, bad[:3]
    assert ran == set(), ran
    assert all(len(o["cigar"]) == 0 and o["score"] == -0x40000000 for o in expectations(cases))


def test_scoring_beyond_the_limit_is_refused(ctx):
    """(q+e)+(q2+e2) == 128: WM_EINVAL (wm_ksw_score_ok), as mm_check_opt refuses it (src/options.c:166-176); 127 is served (the tests above)"""
    c = dict(kswcases.class_edge_cases(9, (496,))[0])
    jobs, seqs = gpu.pack_jobs([(c["q"], c["t"], dict(w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flag=c["flag"]))])
    for q, e, q2, e2 in ((40, 4, 80, 4), (60, 4, 62, 2), (80, 4, 40, 4)):
        assert q + e + q2 + e2 == 128
        with pytest.raises(gpu.WmError, match="libwmgpu error -2:"):
            ctx.ksw_batch(gpu.KswScore(1, -4, -1, q, e, q2, e2), jobs, seqs)
