"""CPU: mm_fix_cigar on the wavefront emulator (csrc/fix_kernel.h; src/align.c:91-167) — every named and random case of fixcases, byte form and position
form over wm_pack_codes data, against the specification (csrc/cigar_fix.h): CIGAR, count, both shifts, `changed`; the fused form (fix, then the scan of
extra_kernel.h on the fixed CIGAR with the operands advanced by both shifts) at three routings against wm_extra_walk on the fixed CIGAR; specification and
emulator against the reference's own mm_update_extra where oracle/_ref is built; and the Python restatement of fixcases against the specification."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import extracases as X
import fixcases as F
from winnowmap_amd import build

i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
i64p = np.ctypeslib.ndpointer(np.int64, flags="C")
ALL_SHORT, ALL_LONG = 1 << 30, 1
ROUTES = [(ALL_SHORT, X.T), (ALL_LONG, 64), (ALL_LONG, X.T)]


@pytest.fixture(scope="module")
def E():
    L = C.CDLL(build.build_emu_fix())
    L.emu_fix_spec.argtypes = [W.u32p, C.c_int, W.u8p, W.u8p, i32p]
    L.emu_fix_spec.restype = None
    L.emu_fix_batch.argtypes = [C.c_int, C.c_void_p, W.u32p, W.u32p, W.u32p, i32p, W.u8p, C.c_size_t, W.u32p, W.u32p, C.c_int, C.c_int, i32p, i32p]
    L.emu_fix_batch_pos.argtypes = [C.c_int, C.c_void_p, i64p, i32p, i32p, i64p, W.u32p, i32p, W.u8p, C.c_size_t, W.u8p, C.c_size_t, W.u32p, W.u32p,
                                    C.c_int, C.c_int, i32p, i32p]
    return L


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    L.h_extra_walk_both.argtypes = [C.c_void_p, C.c_void_p, W.u32p, C.c_int] + [C.c_int] * 5 + [i32p, i32p]
    return L


def spec(E, cig, q, t):
    """wm_fix_cigar -> (fixed cigar, [n_cigar, qshift, tshift, changed])"""
    c = np.concatenate([np.ascontiguousarray(cig, np.uint32), np.zeros(1, np.uint32)])
    o = np.zeros(4, np.int32)
    E.emu_fix_spec(c, len(cig), np.ascontiguousarray(q), np.ascontiguousarray(t), o)
    return c[:o[0]].copy(), o


def walk(H, cig, q, t, sc):
    f, g = np.zeros(6, np.int32), np.zeros(6, np.int32)
    cg = np.ascontiguousarray(cig, np.uint32) if len(cig) else np.zeros(1, np.uint32)
    q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
    H.h_extra_walk_both(q.ctypes.data, t.ctypes.data, cg, len(cig), *[int(v) for v in sc], f, g)
    return g


@pytest.fixture(scope="module")
def CASES():
    return F.make_cases() + F.batch70() + F.random_cases() + F.random_zero_cases()


@pytest.fixture(scope="module")
def WANT(E, CASES):
    """computed once: the specification's answer for every byte-form case"""
    return {c[0]: spec(E, c[1], c[2], c[3]) for c in CASES}


def run_bytes(E, cases, score=None, long_min=ALL_SHORT, tile=X.T):
    q_off, t_off, cig_off, n_cig, seqs, cigs = [], [], [], [], [], []
    at = ops = 0
    for _, cig, q, t, _ in cases:
        q_off.append(at); seqs.append(q); at += len(q)
        t_off.append(at); seqs.append(t); at += len(t)
        cig_off.append(ops); n_cig.append(len(cig)); cigs.append(cig); ops += len(cig)
    cigs = np.concatenate(cigs + [np.zeros(1, np.uint32)]).astype(np.uint32)
    seqs = np.ascontiguousarray(np.concatenate(seqs))
    out = np.full(len(cigs), 0xdeadbeef, np.uint32); fix = np.full((len(cases), 4), -7, np.int32); ex = np.full((len(cases), 6), -7, np.int32)
    sc = None if score is None else np.array(score, np.int32).ctypes.data
    assert E.emu_fix_batch(len(cases), sc, np.array(q_off, np.uint32), np.array(t_off, np.uint32), np.array(cig_off, np.uint32), np.array(n_cig, np.int32),
                           seqs, len(seqs), cigs, out, long_min, tile, fix, ex) == 0
    return [(out[o:o + f[0]], f, x) for o, f, x in zip(cig_off, fix, ex)]


def by_score(cases):
    groups = {}
    for c in cases:
        groups.setdefault(tuple(c[4]), []).append(c)
    return list(groups.values())


def test_the_restatement_equals_the_specification(E, CASES, WANT):
    for c in CASES:
        fixed, qs, ts, ch, info = F.fix_py(c[1], c[2], c[3])
        wc, wo = WANT[c[0]]
        assert fixed == [int(w) for w in wc] and [len(fixed), qs, ts, ch] == [int(v) for v in wo], c[0]
    for p in F.make_pos_cases():
        q, t = F.pos_operands(p)
        fixed, qs, ts, ch, info = F.fix_py(p[1], q, t)
        wc, wo = spec(E, p[1], q, t)
        assert fixed == [int(w) for w in wc] and [len(fixed), qs, ts, ch] == [int(v) for v in wo], p[0]


def test_the_random_cases_reach_the_rare_paths(E):
    """a guard on the INPUTS (the events are counted by the restatement, whose answer is held against the specification here as well)"""
    cnt = {k: 0 for k in F.FLOORS}
    R = F.random_cases()
    assert len(R) == 300 and all(2 <= len(c[1]) <= 200 for c in R)
    for c in R:
        fixed, qs, ts, ch, info = F.fix_py(c[1], c[2], c[3])
        assert [len(fixed), qs, ts, ch] == [int(v) for v in spec(E, c[1], c[2], c[3])[1]], c[0]
        for k, v in F.events(info).items():
            cnt[k] += v
    print(cnt)
    for k, floor in F.FLOORS.items():
        assert cnt[k] >= floor, (k, cnt)
    # the zero-length set: a raw zero-length M behind an eligible op that shifted (it has grown when the loop reaches it) in at least a quarter of the cases
    # (56 of 100 when this was written)
    Z = F.random_zero_cases()
    grown = 0
    for c in Z:
        info = F.fix_py(c[1], c[2], c[3])[4]
        cg = [int(w) for w in c[1]]
        grown += any(k + 1 < len(cg) and cg[k + 1] >> 4 == 0 and l > 0 for k, (l, p) in info["l"].items())
    assert len(Z) == 100 and grown >= 25, grown


def test_the_cases_pin_what_their_names_say(E):
    """a guard on the INPUTS, through the restatement (held against the specification case by case)"""
    by = {c[0]: c for c in F.make_cases()}

    def fx(name):
        c = by[name]
        fixed, qs, ts, ch, info = F.fix_py(c[1], c[2], c[3])
        wc, wo = spec(E, c[1], c[2], c[3])
        assert fixed == [int(w) for w in wc] and [len(fixed), qs, ts, ch] == [int(v) for v in wo], name
        return [(w & 0xf, w >> 4) for w in fixed], qs, ts, ch, info
    M, I, D, N = F.M, F.I, F.D, F.N
    assert fx("n_cigar_1_5I_alone_is_untouched")[:4] == ([(I, 5)], 0, 0, 0) and fx("n_cigar_1_5D_alone_is_untouched")[:4] == ([(D, 5)], 0, 0, 0)
    assert fx("n_cigar_2_I_M_loses_its_I")[:4] == ([(M, 5)], 2, 0, 1)
    assert fx("I_shifted_partly")[0] == [(M, 6), (I, 2), (M, 14)] and fx("I_shifted_fully_zeroes_the_M")[:2] == ([(M, 20)], 2)
    assert fx("I_not_shifted")[3] == 0
    assert fx("D_shifted_partly")[0] == [(M, 3), (D, 3), (M, 17)] and fx("D_shifted_fully_zeroes_the_M")[:3] == ([(M, 20)], 0, 3)
    assert fx("I_decided_by_the_query_the_target_says_0")[4]["l"][1][0] == 5 and fx("I_decided_by_the_query_the_target_says_more")[4]["l"][1][0] == 2
    assert fx("D_decided_by_the_target_the_query_says_0")[4]["l"][1][0] == 5 and fx("D_decided_by_the_target_the_query_says_more")[4]["l"][1][0] == 2
    assert fx("N_equals_N_continues_the_run")[4]["l"][1][0] == 6 and fx("N_against_a_base_stops_the_run")[4]["l"][1][0] == 1
    for name in ("not_eligible_indel_at_k_0", "not_eligible_indel_at_k_n_minus_1"):
        assert sorted(fx(name)[4]["l"]) == [2 if name.endswith("k_0") else 1]
    assert fx("not_eligible_next_to_an_N_op")[4]["l"] == {} and fx("not_eligible_next_to_another_indel")[4]["l"] == {}
    f = fx("prev_len_0_sets_to_shrink_without_a_shift")
    assert f[4]["l"][2] == (0, 0) and f[4]["shrink"] and f[0] == [(M, 4), (I, 2), (M, 8)]
    for r in (63, 64, 65):
        assert fx("I_compare_of_200_first_mismatch_at_%d" % r)[4]["l"][1] == (r, 200) and fx("D_compare_of_200_first_mismatch_at_%d" % r)[4]["l"][1] == (r, 200)
    assert fx("chain_1M1I_x70_homopolymer_one_leading_70I")[:3] == ([(M, 75)], 70, 0) and fx("chain_1M1D_x70_homopolymer_one_leading_70D")[:3] == ([(M, 75)], 0, 70)
    assert fx("chain_extension_of_150_bases")[4]["l"] == {1: (150, 150), 3: (151, 151)}
    for at in (63, 64, 65):
        assert fx("eligible_op_at_index_%d" % at)[4]["l"][at][0] > 0
    for n in (64, 65, 128):
        assert len(by["cigar_of_exactly_%d_ops" % n][1]) == n
    assert fx("pass_2_run_straddles_ops_62_to_66")[4]["rewrites"] == [62] and fx("pass_2_run_longer_than_a_tile")[4]["rewrites"] == [1]
    assert len(by["pass_2_run_ends_the_cigar_at_a_tile_edge"][1]) == 64 and fx("pass_2_run_ends_the_cigar_at_a_tile_edge")[4]["rewrites"] == [61]
    assert fx("pass_2_I_D_I_merged")[0] == [(M, 5), (I, 12), (D, 6), (M, 5)] and fx("pass_2_I_D_left_alone")[3] == 0
    assert fx("pass_2_D_I_D_I")[0] == [(M, 5), (I, 6), (D, 4), (M, 5)]
    assert fx("pass_2_run_ends_the_cigar_start_at_n_minus_3")[0] == [(M, 5), (I, 12), (D, 6)] and fx("pass_2_start_at_n_minus_2_is_no_start")[4]["rewrites"] == []
    assert fx("pass_2_run_followed_by_N")[0] == [(M, 5), (I, 12), (D, 6), (N, 40), (M, 5)]
    assert fx("pass_2_5I_6D_2M_7I_pass_1_zeroes_the_2M")[0] == [(M, 5), (I, 12), (D, 6), (M, 7)] and fx("pass_2_5I_6D_2M_7I_the_2M_stays")[4]["rewrites"] == []
    assert fx("pass_2_5I_0M_6D_7I_trigger_after_the_zero")[:3] == ([(D, 6), (I, 7)], 5, 0)
    assert fx("pass_2_N_M_at_the_trigger_test")[4]["rewrites"] == [] and fx("pass_2_I_I_D_I_starts_at_the_second_I")[0] == [(M, 5), (I, 7), (D, 3), (M, 5)]
    assert fx("pass_2_only_one_kind_of_gap_has_length")[0] == [(M, 5), (I, 3), (M, 5)]
    assert fx("shrink_5M_3M_2I_4M_without_a_zero_stays_unmerged")[0][:2] == [(M, 5), (M, 3)] and fx("shrink_5M_3M_2I_4M_with_a_zero_elsewhere_merges")[0][0][0:1] == (M,)
    assert len(fx("shrink_5M_3M_2I_4M_with_a_zero_elsewhere_merges")[0]) == 3
    assert fx("lead_2I_3D_5M_only_one_op_removed")[:3] == ([(D, 3), (M, 5)], 2, 0) and fx("lead_D_gives_tshift")[1:3] == (0, 4)
    assert fx("lead_indel_appears_only_after_the_squeeze")[1:3] == (3, 0) and fx("lead_indel_made_by_pass_1")[:3] == ([(M, 11)], 2, 0)
    assert fx("lead_merged_indels_are_one_op")[:3] == ([(M, 6)], 5, 0)
    f = fx("zero_M_behind_a_partly_shifting_I_is_no_zero_any_more")
    assert f[0] == [(M, 9), (I, 2), (M, 1), (M, 5), (M, 3)] and not f[4]["shrink"] and f[3] == 1
    f = fx("zero_M_behind_a_partly_shifting_D_is_no_zero_any_more")
    assert f[0] == [(M, 6), (D, 3), (M, 4), (I, 1), (M, 2), (M, 2)] and not f[4]["shrink"]
    assert fx("zero_M_behind_an_I_that_does_not_shift_is_a_zero")[0] == [(M, 10), (I, 2), (M, 8)]
    f = fx("zero_M_behind_a_partly_shifting_I_across_the_tile_edge")
    assert f[4]["l"][63] == (3, 9) and not f[4]["shrink"] and f[0][62:67] == [(M, 6), (I, 1), (M, 3), (M, 2), (M, 2)] and len(by["zero_M_behind_a_partly_shifting_I_across_the_tile_edge"][1]) == 69
    f = fx("op_codes_4_to_9_with_a_length_are_inert")
    assert (7, 9) in f[0] and (4, 3) in f[0] and (9, 4) in f[0]
    assert len(by["one_job_of_5000_ops"][1]) == 5000


def check_fix(name, got, want):
    (gc, gf, _), (wc, wf) = got, want
    assert np.array_equal(gf, wf) and np.array_equal(gc, wc), (name, gf, wf, gc[:12], wc[:12])


def test_every_case_in_byte_form_equals_the_specification(E, CASES, WANT):
    got = run_bytes(E, CASES)
    for c, g in zip(CASES, got):
        check_fix(c[0], g, WANT[c[0]])
    assert len(CASES) > 530


def pos_arrays(P, lead=F.LEAD):
    reads = [np.full(lead, 4, np.uint8)]; ref = [np.full(13, 4, np.uint8)]
    qwin, qlen, qpos, tbase, cig_off, n_cig, cigs = [], [], [], [], [], [], []
    rn, fn, ops = lead, 13, 0
    for name, cig, read, q_pos, contig, t_pos, score in P:
        qwin.append(lead); qlen.append(len(read)); qpos.append(q_pos)
        tbase.append(fn + t_pos); ref.append(contig); fn += len(contig)
        cig_off.append(ops); n_cig.append(len(cig)); cigs.append(cig); ops += len(cig)
    reads.append(P[0][2])
    return (np.array(qwin, np.int64), np.array(qlen, np.int32), np.array(qpos, np.int32), np.array(tbase, np.int64), np.array(cig_off, np.uint32),
            np.array(n_cig, np.int32), np.ascontiguousarray(np.concatenate(reads)), np.ascontiguousarray(np.concatenate(ref)),
            np.concatenate(cigs).astype(np.uint32))


@pytest.mark.parametrize("fused,long_min,tile", [(False, ALL_SHORT, X.T)] + [(True,) + r for r in ROUTES])
def test_position_form_over_packed_reads_and_nibbles_equals_the_specification(E, H, fused, long_min, tile):
    P = F.make_pos_cases()
    assert all(p[2] is P[0][2] for p in P)
    for score in sorted(set(tuple(p[6]) for p in P)):
        G = [p for p in P if tuple(p[6]) == score]
        qwin, qlen, qpos, tbase, cig_off, n_cig, reads, ref, cigs = pos_arrays(G)
        out = np.full(len(cigs) + 1, 0xdeadbeef, np.uint32); fix = np.full((len(G), 4), -7, np.int32); ex = np.full((len(G), 6), -7, np.int32)
        sc = np.array(score, np.int32)
        assert E.emu_fix_batch_pos(len(G), sc.ctypes.data if fused else None, qwin, qlen, qpos, tbase, cig_off, n_cig, reads, len(reads), ref, len(ref), cigs, out,
                                   long_min, tile, fix, ex) == 0
        for p, o, f, x in zip(G, cig_off, fix, ex):
            q, t = F.pos_operands(p)
            wc, wf = spec(E, p[1], q, t)
            check_fix(p[0], (out[o:o + f[0]], f, None), (wc, wf))
            if fused:
                want = walk(H, wc, q[wf[1]:], t[wf[2]:], score)
                assert np.array_equal(x, want), (p[0], x, want)


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_the_fused_form_equals_wm_extra_walk_on_the_fixed_cigar(E, H, CASES, WANT, long_min, tile):
    for group in by_score(CASES):
        score = group[0][4]
        got = run_bytes(E, group, score, long_min, tile)
        for c, g in zip(group, got):
            wc, wf = WANT[c[0]]
            check_fix(c[0], g, (wc, wf))
            want = walk(H, wc, c[2][wf[1]:], c[3][wf[2]:], score)
            assert np.array_equal(g[2], want), (c[0], long_min, tile, g[2], want)


@pytest.mark.skipif(not W.have_ref(), reason="oracle/_ref not built")
def test_specification_and_emulator_equal_the_references_own_mm_update_extra(E, CASES, WANT):
    """every case the reference can take (ops M / I / D / N, match > 0, no zero-length op of code >= 3, not all lengths zero): the CIGAR it leaves, qs / qe for rev 0 and
    1, rs, and blen, mlen, n_ambi, dp_max"""
    R = W.ref()
    R.refshim_update_extra.argtypes = [C.c_int] * 5 + [W.u8p, W.u8p, W.i8p, C.c_int, C.c_int] + [C.c_uint32, W.u32p, i32p, W.u32p, C.c_int, C.POINTER(C.c_int)]
    ok = [c for c in CASES if len(c[1]) and c[4][0] > 0 and all((int(w) & 0xf) <= 3 for w in c[1]) and not any((int(w) & 0xf) == 3 and int(w) >> 4 == 0 for w in c[1])
          and any(int(w) >> 4 for w in c[1])]
    assert len(ok) > 400
    fused = {}
    for group in by_score(ok):
        for c, g in zip(group, run_bytes(E, group, group[0][4], ALL_SHORT, X.T)):
            fused[c[0]] = g
    for c in ok:
        name, cig, q, t, score = c
        mat = W.simple_mat(score[0], -score[1], -score[2])
        ql = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 1)); tl = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 2, 3))
        wc, wf = WANT[name]
        gc, gf, gx = fused[name]
        for rev in (0, 1):
            o = np.zeros(6, np.int32); c1 = np.zeros(len(cig) + 4, np.uint32); n1 = C.c_int()
            R.refshim_update_extra(rev, 100, 100 + ql, 1000, 1000 + tl, np.ascontiguousarray(q), np.ascontiguousarray(t), mat, score[3], score[4], len(cig),
                                   np.ascontiguousarray(cig, np.uint32), o, c1, len(c1), C.byref(n1))
            assert n1.value == wf[0] == gf[0] and np.array_equal(c1[:n1.value], wc) and np.array_equal(gc, wc), (name, rev)
            assert int(o[4]) == (100 + ql - wf[1] if rev else 100 + wf[1]) and int(o[5]) == 1000 + wf[2], (name, rev, o, wf)
            assert np.array_equal(gf, wf)
            assert (int(gx[2]), int(gx[1]), int(gx[3]), int(gx[0])) == tuple(int(v) for v in o[:4]), (name, rev, gx, o)      # blen, mlen, n_ambi, dp_max
