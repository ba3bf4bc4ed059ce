"""CPU: mm_update_cigar_eqx (src/align.c:169-238) — the specification (csrc/cigar_eqx.h) against a numpy restatement of its rules, and the kernels of
csrc/eqx_kernel.h on the wavefront emulator (prefix, count pass, scan over jobs, write pass; one wavefront per job / one per tile + combine; tile sizes 64 and
the default; byte form and position form over wm_pack_codes data) against the specification, op for op and branch for branch."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import extracases as X
import eqxcases as Q
from winnowmap_amd import build
from test_host_simd import random_alignment

i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
i64p = np.ctypeslib.ndpointer(np.int64, flags="C")
ALL_SHORT, ALL_LONG = 1 << 30, 1
ROUTES = [(ALL_SHORT, 64), (ALL_SHORT, Q.T), (ALL_LONG, 64), (ALL_LONG, Q.T)]


@pytest.fixture(scope="module")
def E():
    L = C.CDLL(build.build_emu_eqx())
    L.emu_eqx_spec.argtypes = [W.u32p, C.c_int, W.u8p, W.u8p, W.u32p, i32p]
    L.emu_eqx_batch.argtypes = [C.c_int, W.u32p, W.u32p, W.u32p, i32p, W.u8p, C.c_size_t, W.u32p, C.c_int, C.c_int, W.u32p, C.c_size_t, i32p]
    L.emu_eqx_batch_pos.argtypes = [C.c_int, i64p, i32p, i32p, i64p, W.u32p, i32p, W.u8p, C.c_size_t, W.u8p, C.c_size_t, W.u32p, C.c_int, C.c_int, W.u32p, C.c_size_t, i32p]
    return L


def spec(E, cig, q, t):
    cg = np.ascontiguousarray(cig, np.uint32) if len(cig) else np.zeros(1, np.uint32)
    out = np.zeros(len(cig) + Q.m_columns(cig) + 1, np.uint32); ip = np.zeros(1, np.int32)
    n = E.emu_eqx_spec(cg, len(cig), np.ascontiguousarray(q), np.ascontiguousarray(t), out, ip)
    return out[:n].copy(), int(ip[0])


def text(cig):
    return "".join("%d%s" % (int(w) >> 4, "MIDNSHP=XB??????"[int(w) & 0xf]) for w in cig)


@pytest.fixture(scope="module")
def CASES(E):
    """computed once: every byte-form case with what the specification gives"""
    cases = Q.make_cases() + Q.batch70() + [Q.long_40k()]
    return [(c, spec(E, c[1], c[2], c[3])) for c in cases]


def run_bytes(E, cases, long_min, tile, cap=None):
    q_off, t_off, cig_off, n_cig, seqs, cigs, ops = X_pack(cases)
    bound = ops + sum(Q.m_columns(c[1]) for c in cases)
    out = np.zeros(bound + 1, np.uint32); res = np.full((len(cases), 4), -7, np.int32)
    total = E.emu_eqx_batch(len(cases), q_off, t_off, cig_off, n_cig, seqs, len(seqs), cigs, long_min, tile, out, bound if cap is None else cap, res)
    return total, out, res


def X_pack(cases):
    q_off, t_off, cig_off, n_cig, seqs, cigs = [], [], [], [], [], []
    at = ops = 0
    for _, cig, q, t in cases:
        q_off.append(at); seqs.append(q); at += len(q)
        t_off.append(at); seqs.append(t); at += len(t)
        cig_off.append(ops); n_cig.append(len(cig)); cigs.append(cig); ops += len(cig)
    cigs = np.concatenate(cigs + [np.zeros(1, np.uint32)]).astype(np.uint32)
    return (np.array(q_off, np.uint32), np.array(t_off, np.uint32), np.array(cig_off, np.uint32), np.array(n_cig, np.int32),
            np.ascontiguousarray(np.concatenate(seqs)), cigs, ops)


def check(cases, wants, total, out, res, tag):
    at = 0
    for i, (c, (want, ip)) in enumerate(zip(cases, wants)):
        off, hi, n, got_ip = (int(v) for v in res[i])
        assert hi == 0 and off == at, (c[0], tag, off, at)                      # back to back, in job order
        assert got_ip == ip, (c[0], tag, "branch", got_ip, ip)
        assert n == len(want) and np.array_equal(out[off:off + n], want), (c[0], tag, text(out[off:off + n])[:200], text(want)[:200])
        at += n
    assert total == at


def test_the_case_list_is_what_the_issue_asks_for():
    cases = Q.make_cases()
    assert len(cases) > 60 and len(set(c[0] for c in cases)) == len(cases)
    assert len(Q.batch70()) == 70 and Q.m_columns(Q.long_40k()[1]) == 40000 and Q.T % 64 == 0


def test_specification_equals_the_numpy_restatement(CASES):
    n_ip = 0
    for c, (got, ip) in CASES:
        want, want_ip = Q.restated(c[1], c[2], c[3])
        assert ip == want_ip and np.array_equal(got, want), (c[0], text(got)[:200], text(want)[:200])
        n_ip += ip
    assert 10 < n_ip < len(CASES) - 40                                          # both branches, often


def test_the_cases_pin_what_their_names_say(CASES):
    by = {c[0]: (text(got), ip) for c, (got, ip) in CASES}
    assert by["all_match_single_M_in_place"] == ("100=", 1)
    assert by["one_mismatch_first_column"] == ("1X99=", 0) and by["one_mismatch_last_column"] == ("99=1X", 0) and by["one_mismatch_middle_column"] == ("50=1X49=", 0)
    assert by["all_mismatch_single_M_is_relabelled_in_place"] == ("70=", 1)
    assert by["quirk_all_mismatch_M_among_all_match_ones_comes_out_as_EQ"] == ("10=1I1=1D10=", 1)
    assert by["quirk_broken_by_one_more_mismatch_comes_out_as_X"] == ("10=1I1X1D4=1X5=", 0)
    assert by["adjacent_M_ops_agreeing_bases_in_place"] == ("10=10=", 1) and by["adjacent_M_ops_agreeing_bases_rewritten"] == ("3=1X6=10=", 0)
    assert by["adjacent_M_ops_mismatches_on_both_sides_of_the_boundary"] == ("9=1X1X9=", 0)
    assert by["zero_length_M_vanishes_in_the_rewrite_branch"] == ("5=2I5=", 0) and by["zero_length_M_balances_an_extra_run_in_place"] == ("5=0=2I5=", 1)
    assert by["input_ops_7_8_4_5_and_zero_length_I_copied_rewrite"] == ("3S5=2=1X3=0I2X4=2H", 0)
    assert by["input_ops_7_8_4_5_and_zero_length_I_copied_in_place"] == ("3S5=6=0I2X4=2H", 1)
    assert by["only_I_and_D"] == ("5I9D1I", 1) and by["empty_cigar_between_two_real_jobs"] == ("", 1)
    assert by["N_against_N_is_EQ"] == ("40=", 1) and by["N_against_N_is_EQ_beside_a_mismatch"] == ("11=1X28=", 0) and by["N_against_a_base_is_X"] == ("10=1X19=1X9=", 0)
    for t in Q.TILES:
        got = by["alternating_every_column_%d_columns_tile_%d" % (t + 1, t)]
        assert got == ("1=" + "1X1=" * (t // 2), 0)
        assert by["run_spans_three_tiles_middle_one_without_a_head_%d" % t] == ("%d=1X%d=" % (t - 5, 2 * t - 6), 0)
        assert by["X_run_spans_three_tiles_middle_one_without_a_head_%d" % t] == ("%d=%dX%d=" % (t - 5, t + 14, t - 19), 0)
        assert by["head_on_a_tiles_first_column_%d" % t] == ("%d=1X%d=" % (t - 1, t), 0)


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_emulated_kernels_equal_the_specification_on_every_named_case(E, CASES, long_min, tile):
    cases = [c for c, _ in CASES if c[0] != "long_40k" or (long_min, tile) == (ALL_LONG, Q.T)]      # (the emulator takes seconds for that one: once, and under the default routing below)
    wants = [w for c, w in CASES if c in cases]
    total, out, res = run_bytes(E, cases, long_min, tile)
    check(cases, wants, total, out, res, (long_min, tile))


def test_the_default_routing_sends_40000_columns_to_the_long_class_and_the_rest_to_the_short_one(E, CASES):
    pick = [(c, w) for c, w in CASES if c[0] == "long_40k" or c[0].startswith("mixed") or c[0].startswith("quirk")]
    cases = [c for c, _ in pick]
    total, out, res = run_bytes(E, cases, 32768, Q.T)
    check(cases, [w for _, w in pick], total, out, res, "default routing")


def test_a_pool_one_op_too_small_reports_the_needed_count_and_writes_nothing(E, CASES):
    pick = [(c, w) for c, w in CASES if c[0].startswith("batch70")]
    cases = [c for c, _ in pick]
    needed = sum(len(w[0]) for _, w in pick)
    total, out, res = run_bytes(E, cases, ALL_SHORT, 64, cap=needed - 1)
    assert total == needed and not out.any()
    assert [int(r[2]) for r in res] == [len(w[0]) for _, w in pick]             # res is already filled
    total, out, res = run_bytes(E, cases, ALL_SHORT, 64, cap=needed)
    check(cases, [w for _, w in pick], total, out, res, "exact capacity")


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_300_random_alignments_equal_the_specification(E, long_min, tile):
    rng = np.random.default_rng(13)
    cases = []
    for it in range(300):
        cig, q, t = random_alignment(rng, int(rng.integers(1, 60)), 0.0 if it % 3 else 0.02)
        if it % 5 == 0:                       # a third of the alignments would otherwise never take the in-place branch: make the query agree along M
            qo = to = 0
            q = q.copy()
            for w in cig:
                op, ln = int(w) & 0xf, int(w) >> 4
                if op == 0:
                    q[qo:qo + ln] = t[to:to + ln]
                qo += ln if op in (0, 1) else 0; to += ln if op in (0, 2, 3) else 0
        cases.append(("random_%d" % it, cig, np.concatenate([q, np.full(16, 4, np.uint8)]), np.concatenate([t, np.full(16, 4, np.uint8)])))
    wants = [spec(E, c[1], c[2], c[3]) for c in cases]
    assert 30 < sum(ip for _, ip in wants) < 270
    for c, (want, ip) in zip(cases, wants):
        r, rip = Q.restated(c[1], c[2], c[3])
        assert rip == ip and np.array_equal(r, want), c[0]
    total, out, res = run_bytes(E, cases, long_min, tile)
    check(cases, wants, total, out, res, (long_min, tile))


def pos_arrays(P):
    """position cases -> one read buffer / one reference buffer behind leads that are no multiple of the word sizes, and the operands spelled out"""
    reads = [np.full(37, 4, np.uint8)]; ref = [np.full(13, 4, np.uint8)]
    qwin, qlen, qpos, tbase, cig_off, n_cig, cigs, operands = [], [], [], [], [], [], [], []
    rn, fn, ops = 37, 13, 0
    for name, cig, read, q_pos, contig, t_pos, score in P:
        qwin.append(rn); qlen.append(len(read)); qpos.append(q_pos); reads.append(read); rn += len(read)
        tbase.append(fn + t_pos); ref.append(contig); fn += len(contig)
        cig_off.append(ops); n_cig.append(len(cig)); cigs.append(cig); ops += len(cig)
        ql = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 1)); tl = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 2, 3))
        operands.append((np.concatenate([X.two_strand(read, q_pos, ql), np.full(16, 4, np.uint8)]), np.concatenate([contig[t_pos:t_pos + tl], np.full(16, 4, np.uint8)])))
    return (np.array(qwin, np.int64), np.array(qlen, np.int32), np.array(qpos, np.int32), np.array(tbase, np.int64), np.array(cig_off, np.uint32),
            np.array(n_cig, np.int32), np.ascontiguousarray(np.concatenate(reads)), np.ascontiguousarray(np.concatenate(ref)),
            np.concatenate(cigs).astype(np.uint32), ops, operands)


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_position_form_over_packed_reads_and_nibbles_equals_the_specification(E, long_min, tile):
    """extracases' position cases: forward and reverse strand, a query that starts in front of its strand (the other strand's tail, or N padding) and one that runs
    off the end of two-strand space (N), every target alignment mod 8"""
    P = X.make_pos_cases()
    qwin, qlen, qpos, tbase, cig_off, n_cig, reads, ref, cigs, ops, operands = pos_arrays(P)
    bound = ops + sum(Q.m_columns(p[1]) for p in P)
    out = np.zeros(bound + 1, np.uint32); res = np.full((len(P), 4), -7, np.int32)
    total = E.emu_eqx_batch_pos(len(P), qwin, qlen, qpos, tbase, cig_off, n_cig, reads, len(reads), ref, len(ref), cigs, long_min, tile, out, bound, res)
    cases = [(p[0], p[1], q, t) for p, (q, t) in zip(P, operands)]
    wants = [spec(E, c[1], c[2], c[3]) for c in cases]
    assert any((int(w) & 0xf) == 8 for want, _ in wants for w in want)
    check(cases, wants, total, out, res, (long_min, tile))
