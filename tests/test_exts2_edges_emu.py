"""The splice-aware extension at its edges, on the host wavefront emulator: every case of tests/exts2cases.py through ksw_dp_exts2 +
ksw_exts2_backtrack_thread (ksw_exts2_kernel.h) against the oracle's ksw_exts2_sse (pinned to the reference on the same cases by
tests/test_oracle_vs_ref.py), in every field and the CIGAR. test_every_edge_matters is about the cases themselves: each edge changes the oracle's
result against its neighbour, so a kernel that is off by one there cannot pass. The lane priority of the exact-maximum reduction (ksw_pri_pack,
ksw_kernel.h: every ksw kernel packs the lane of a row's maximum with it) is checked on its own and by jobs whose maximum lies beyond target base 2^20."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import exts2cases as XC
from test_kernels_emu import _load_emu, _load_stripe, _load_chain, emu_ksw

# cases of the list whose oracle CIGAR holds an N: counted on this list (test_every_edge_matters asserts the count does not fall below it)
N_FLOOR = 270          # the list yields 276


@pytest.fixture(scope="module")
def emu():
    E = _load_emu()
    E.emu_ksw_exts2.argtypes = [C.c_int, W.u8p, C.c_int, W.u8p, W.i8p] + [C.c_int] * 7 + [C.c_void_p, W.i32p, W.u32p, C.c_int]
    for f in (E.emu_ksw_pri_pack, E.emu_ksw_pri_pack_v):
        f.argtypes = [C.c_int, C.c_int]
    E.emu_ksw_pri_lane.argtypes = [C.c_int]
    return E


CASES = XC.edge_cases()
BY_NAME = {c["name"]: c for c in CASES}
_EXPECT = {}


def oracle_of(c):
    """the oracle's result of a case: computed once, shared by the tests of this module"""
    if c["name"] not in _EXPECT:
        _EXPECT[c["name"]] = W.o_ksw_exts2(c["q"], c["t"], mat=W.simple_mat(c["a"], c["b"], c["sc_ambi"]), q=c["q_"], e=c["e"], q2=c["q2"], noncan=c["noncan"],
                                           zdrop=c["zdrop"], junc_bonus=c["junc_bonus"], flag=c["flag"], junc=c["junc"])
    return _EXPECT[c["name"]]


def emu_of(E, c):
    ez = np.zeros(10, np.int32)
    cig = np.zeros(len(c["q"]) + len(c["t"]) + 4, np.uint32)
    n = E.emu_ksw_exts2(len(c["q"]), c["q"], len(c["t"]), c["t"], W.simple_mat(c["a"], c["b"], c["sc_ambi"]), c["q_"], c["e"], c["q2"], c["noncan"], c["zdrop"],
                        c["junc_bonus"], c["flag"], None if c["junc"] is None else c["junc"].ctypes.data, ez, cig, len(cig))
    return n, [int(x) for x in ez], cig[:max(n, 0)]


def same(a, b):
    return all(a[k] == b[k] for k in W.EZ_FIELDS) and np.array_equal(a["cigar"], b["cigar"])


def has_n(o):
    return any((int(x) & 0xf) == 3 for x in o["cigar"])


def test_every_case_emulated_matches_oracle(emu):
    bad = []
    for c in CASES:
        o = oracle_of(c)
        n, ez, cig = emu_of(emu, c)
        if n < 0 or ez != [o[k] for k in W.EZ_FIELDS] or not np.array_equal(cig, o["cigar"]):
            bad.append((c["name"], n, {k: (g, o[k]) for k, g in zip(W.EZ_FIELDS, ez) if g != o[k]}, W.cigar_str(cig)[:40], W.cigar_str(o["cigar"])[:40]))
    assert not bad, (len(bad), bad[:8])


def test_every_edge_matters():
    """on the oracle alone: each edge of the list against its neighbour"""
    for label, a, b in XC.PAIRS:
        assert not same(oracle_of(BY_NAME[a]), oracle_of(BY_NAME[b])), label
    # the admitted positions take the intron, the refused ones the deletion
    assert has_n(oracle_of(BY_NAME["donor_at_tlen-5"])) and not has_n(oracle_of(BY_NAME["donor_at_tlen-4"]))
    assert oracle_of(BY_NAME["acceptor_at_2"])["score"] == 13 + 15 - 8 and oracle_of(BY_NAME["acceptor_at_1"])["score"] == 13 + 15 - 8 - 5
    # -noncan / 2 is -4 for noncan 9 and for 8: a half-canonical donor costs the same, a site with no motif does not
    assert [oracle_of(BY_NAME["flank_GTC_%s_flank_nc%d" % (a, n)])["score"] for a in ("CAG", "AAA") for n in (9, 8)] == [24 - 8 - 4, 24 - 8 - 4, 24 - 8 - 4 - 9, 24 - 8 - 4 - 8]
    assert [oracle_of(BY_NAME["zdrop_%d_extz" % z])["zdropped"] for z in (XC.ZDROP_FULL, XC.ZDROP_FULL - 1, 0, -1)] == [0, 1, 1, 0]
    # the backtrack's leftover target bases: D up to min_intron of them, N from min_intron + 1 on
    # (with q2 = 127 the int8 lanes wrap and the alignment is no longer a plain overhang: that set is held by PAIRS alone)
    for nm, sc in (("lt1", XC.LT1), ("lt9", XC.LT9), ("ltmin", XC.LTMIN)):
        lt = XC.long_thres(sc)
        assert W.cigar_str(oracle_of(BY_NAME["overhang_%s_%d_for" % (nm, lt)])["cigar"]) == "%dD10M" % lt, nm
        assert W.cigar_str(oracle_of(BY_NAME["overhang_%s_%d_for" % (nm, lt + 1)])["cigar"]) == "%dN10M" % (lt + 1), nm
    # every junction bit a flag combination reads changes the result at some position; the bits it does not read change nothing anywhere; NULL == zeros
    for fn, _ in XC.JUNC_FLAGS:
        none = oracle_of(BY_NAME["junc_none_%s" % fn])
        assert same(none, oracle_of(BY_NAME["junc_null_%s" % fn])), fn
        for bit in XC.JUNC_BITS:
            diff = [pn for pn in XC.JUNC_POS if not same(none, oracle_of(BY_NAME["junc_b%d_at_%s_%s" % (bit, pn, fn)]))]
            if bit & XC.JUNC_LIVE[fn]:
                assert diff, (fn, bit)
            else:
                assert not diff, (fn, bit, diff)
    # an extension with no positive cell
    for nm in ("nopos_1x1", "nopos_3x7", "nopos_20x20"):
        o = oracle_of(BY_NAME[nm])
        assert (o["max"], o["max_t"], o["max_q"], len(o["cigar"])) == (0, -1, -1, 0), nm
    n_intron = sum(has_n(oracle_of(c)) for c in CASES)
    assert n_intron >= N_FLOOR, n_intron


def test_rejected_scoring_sets(emu):
    """the reference returns a reset result for these (src/ksw2_exts2_sse.c:66, :84): so does the oracle, and the argument check wm_ksw_exts2_batch applies
    (wm_ksw_exts2_score_check, ksw_plan.h) refuses them — the N score below -2 (q + e) included; the sets on the limit pass it"""
    c0 = BY_NAME["limit_ambi_at_limit_%x" % XC.FOR]
    for nm, (a, b, q, e, q2, amb) in XC.REJECTED:
        c = dict(c0, name="rejected_" + nm, a=a, b=b, q_=q, e=e, q2=q2, sc_ambi=amb)
        o = oracle_of(c)
        assert [o[k] for k in W.EZ_FIELDS] == [0, 0, -1, -1, -0x40000000, -1, -0x40000000, -1, -0x40000000, 0] and len(o["cigar"]) == 0, nm
        assert emu_of(emu, c)[0] == -2, nm
    assert emu_of(emu, c0)[0] >= 0


def test_lane_priority_helper(emu):
    """ksw_pri_pack / ksw_pri_lane: under equal H the greater group wins, then the smaller lane; the lane comes back; the value fits a signed 32-bit maximum
    next to -1 = no lane. At lane 0, either side of 2^20 and at the largest lane an entry point admits, for every group"""
    tmax = (1 << 28) - 1
    ts = (0, 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, tmax - 1, tmax)
    keys = []
    for grp in range(6):
        for t in ts:
            p = emu.emu_ksw_pri_pack(grp, t)
            assert p == emu.emu_ksw_pri_pack_v(grp, t)
            assert 0 <= p < (1 << 31) and emu.emu_ksw_pri_lane(p) == t and p >> 28 == grp, (grp, t, p)
            keys.append((grp, -t, p))
    assert emu.emu_ksw_pri_lane(-1) == 0                       # (what the 32-bit reductions make of "no lane": lane 0, as before)
    for a in keys:
        for b in keys:
            assert (a[:2] < b[:2]) == (a[2] < b[2]), (a, b)
    # H above the priority: (H << 32) + pri as the 64-bit reductions form it
    for ha, hb in ((5, 6), (-3, -2), (-0x40000000, 0)):
        assert (ha << 32) + emu.emu_ksw_pri_pack(5, 0) < (hb << 32) + emu.emu_ksw_pri_pack(0, tmax)


def test_exts2_maximum_beyond_2_to_20_target_bases(emu):
    """a 1 048 600-base intron: the maximum stands at target base 1 048 679 (the same job just below 2^20 runs on the device, tests/test_exts2_edges_gpu.py).
    About 40 s of emulation"""
    for n in (1048600,):
        c = XC.long_intron_case(n)
        o = oracle_of(c)
        assert (o["max"], o["max_q"], o["max_t"]) == (48, 79, n + 79) and W.cigar_str(o["cigar"]) == "20M%dN60M" % n
        k, ez, cig = emu_of(emu, c)
        assert k >= 0 and ez == [o[f] for f in W.EZ_FIELDS], (n, ez)
        assert np.array_equal(cig, o["cigar"]), (n, W.cigar_str(cig)[:60])


def _extd2_expect(c):
    return W.o_ksw_extd2(c["q"], c["t"], mat=W.simple_mat(c["a"], c["b"], 1), q=c["q_"], e=c["e"], q2=c["q2"], e2=c["e2"], w=c["w"], zdrop=c["zdrop"],
                         end_bonus=c["end_bonus"], flag=c["flag"])


def test_extd2_maximum_beyond_2_to_20_target_bases_packed(emu):
    """query == target of 1 048 700 bases under a band of 10: the 4-pair packed class with exact maximum (ksw_packed_kernel.h). About 100 s, most of it the oracle's and the emulator's 2 097 399 rows"""
    for n in (1048700,):
        c = XC.long_identity_case(n)
        o = _extd2_expect(c)
        assert (o["max"], o["max_q"], o["max_t"]) == (2 * n, n - 1, n - 1)
        k, ez, cig, klass = emu_ksw(emu, c)
        assert k >= 0 and klass == 6, (k, klass)
        assert [int(x) for x in ez] == [o[f] for f in W.EZ_FIELDS], (n, [int(x) for x in ez])
        assert np.array_equal(cig, o["cigar"])


@pytest.mark.parametrize("force", [27, 202, 126])
def test_extd2_maximum_beyond_2_to_20_target_bases_forced_families(emu, force):
    """the same job forced through the one-wavefront generic kernel (27: ksw_dp_generic, ksw_kernel.h), the packed multi-wave kernel (202: ksw_dp_pmulti<1,2>
    with CLIP, ksw_packed_multi_kernel.h) and the block kernel on two wavefronts (126: ksw_dp_block, ksw_kernel.h), which no thin job reaches by itself.
    50 s, 60 s and 90 s of emulation"""
    c = XC.long_identity_case(1048700)
    o = _extd2_expect(c)
    k, ez, cig, klass = emu_ksw(emu, c, force)
    assert k >= 0, (force, k)
    assert [int(x) for x in ez] == [o[f] for f in W.EZ_FIELDS], (force, [int(x) for x in ez])
    assert np.array_equal(cig, o["cigar"])


@pytest.mark.parametrize("family,force", [("stripe", 302), ("chain", 412)])
def test_extd2_maximum_beyond_2_to_20_target_bases_stripe_and_chain(family, force):
    """and through the stripe-pipelined kernel (302: ksw_dp_stripe<1,2> with CLIP, ksw_stripe_kernel.h) and the chained-workgroup kernel (412: 512-lane stripes
    with CLIP, ksw_chain_kernel.h), two emulated wavefronts each: the row maximum's lane travels from stripe to stripe as a priority. About 50 s and 110 s"""
    E = _load_stripe() if family == "stripe" else _load_chain()
    c = XC.long_identity_case(1048700)
    o = _extd2_expect(c)
    k, ez, cig, klass = emu_ksw(E, c, force)
    assert k >= 0, (family, k)
    assert [int(x) for x in ez] == [o[f] for f in W.EZ_FIELDS], (family, [int(x) for x in ez])
    assert np.array_equal(cig, o["cigar"])
