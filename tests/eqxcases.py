"""Named, deterministic cases for mm_update_cigar_eqx over final CIGARs (csrc/cigar_eqx.h, csrc/eqx_kernel.h; src/align.c:169-238), shared by the emulator
and the GPU tests. A case is (name, cigar, q, t): BAM-encoded ops and both sequences as 0..4 codes of exactly the CIGAR's extent plus 16 bytes of N padding
(extracases.build). Names say what a case pins; `mm` lists the M columns (numbered over the M ops only) whose bases differ. Cases that depend on a tile size
are built for T in TILES = (64, the library's default): a lane's share of a tile is T / 64 columns."""
import zlib
import numpy as np
import extracases as X

T = X.T
TILES = (64, T)
M, I, D, N = X.M, X.I, X.D, X.N
EQ, DIFF = 7, 8


def _case(name, ops, **kw):
    return (name,) + X.build(ops, seed=zlib.crc32(name.encode()), **kw)


def make_cases():
    C = []
    # ---- one M op
    C.append(_case("all_match_single_M_in_place", [(M, 100)]))
    C.append(_case("one_mismatch_first_column", [(M, 100)], mm=[0]))
    C.append(_case("one_mismatch_last_column", [(M, 100)], mm=[99]))
    C.append(_case("one_mismatch_middle_column", [(M, 100)], mm=[50]))
    C.append(_case("all_mismatch_single_M_is_relabelled_in_place", [(M, 70)], all_mm=True))      # one run, one M op: '=' (the quirk in its smallest form)
    for n in (1, 2, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1):
        C.append(_case("single_M_%d_random_mismatches" % n, [(M, n)], mm_rate=0.15))
    for t in TILES:
        s = t // 64
        C.append(_case("alternating_every_column_%d_columns_tile_%d" % (t + 1, t), [(M, t + 1)], mm=list(range(1, t + 1, 2))))
        for e, tag in ((s - 1, "one_before"), (s, "at"), (s + 1, "one_after")):          # the first run ends with column e - 1 ... (e = 0: the op starts with the X)
            C.append(_case("run_ends_%s_a_lanes_share_tile_%d" % (tag, t), [(M, 3 * s + 5)], mm=[e]))
        for e, tag in ((t - 1, "one_before"), (t, "at"), (t + 1, "one_after")):
            C.append(_case("run_ends_%s_the_tile_edge_%d" % (tag, t), [(M, 2 * t + 3)], mm=[e]))
        C.append(_case("run_spans_three_tiles_middle_one_without_a_head_%d" % t, [(M, 3 * t - 10)], mm=[t - 5]))          # '=' from t - 4 to the end
        C.append(_case("X_run_spans_three_tiles_middle_one_without_a_head_%d" % t, [(M, 3 * t - 10)], mm=list(range(t - 5, 2 * t + 9))))
        C.append(_case("head_on_a_tiles_first_column_%d" % t, [(M, 2 * t)], mm=[t - 1]))
        C.append(_case("op_boundary_on_a_tile_edge_%d" % t, [(M, t), (M, t), (I, 2), (M, t + 1)], mm=[2 * t + 1]))
    # ---- op boundaries
    C.append(_case("adjacent_M_ops_agreeing_bases_in_place", [(M, 10), (M, 10)]))
    C.append(_case("adjacent_M_ops_agreeing_bases_rewritten", [(M, 10), (M, 10)], mm=[3]))
    C.append(_case("adjacent_M_ops_mismatches_on_both_sides_of_the_boundary", [(M, 10), (M, 10)], mm=[9, 10]))
    C.append(_case("I_D_N_between_M_ops_operands_advanced", [(M, 30), (I, 4), (M, 25), (D, 7), (M, 40), (N, 90), (M, 33)], mm=[3, 31, 60, 61, 127]))
    C.append(_case("I_D_N_between_M_ops_all_match_in_place", [(M, 30), (I, 4), (M, 25), (D, 7), (M, 40), (N, 90), (M, 33)]))
    C.append(_case("leading_and_trailing_gaps", [(I, 3), (D, 2), (M, 20), (D, 5), (I, 1)], mm=[7]))
    # ---- the quirk (src/align.c:195-201): n_EQX == n_M relabels without looking
    C.append(_case("quirk_all_mismatch_M_among_all_match_ones_comes_out_as_EQ", [(M, 10), (I, 1), (M, 1), (D, 1), (M, 10)], mm=[10]))
    C.append(_case("quirk_broken_by_one_more_mismatch_comes_out_as_X", [(M, 10), (I, 1), (M, 1), (D, 1), (M, 10)], mm=[10, 15]))
    C.append(_case("quirk_long_all_mismatch_M", [(M, 80), (D, 2), (M, 130), (I, 3), (M, 9)], mm=list(range(80, 210))))
    C.append(_case("zero_length_M_vanishes_in_the_rewrite_branch", [(M, 5), (M, 0), (I, 2), (M, 5)]))               # n_M = 3, n_EQX = 2
    C.append(_case("zero_length_M_balances_an_extra_run_in_place", [(M, 5), (M, 0), (I, 2), (M, 5)], mm=[0]))       # n_M = 3, n_EQX = 3: 5=0=2I5=
    C.append(_case("zero_length_M_first_and_last", [(M, 0), (M, 12), (D, 1), (M, 0)], mm=[4, 5]))
    # ---- ops that are copied as they stand
    C.append(_case("input_ops_7_8_4_5_and_zero_length_I_copied_rewrite", [(4, 3), (7, 5), (M, 6), (I, 0), (8, 2), (M, 4), (5, 2)], mm=[2]))
    C.append(_case("input_ops_7_8_4_5_and_zero_length_I_copied_in_place", [(4, 3), (7, 5), (M, 6), (I, 0), (8, 2), (M, 4), (5, 2)]))
    C.append(_case("op_codes_6_9_15_and_zero_length_D_N", [(6, 1), (M, 8), (D, 0), (9, 4), (N, 0), (M, 8), (15, 7)], mm=[7, 8]))
    C.append(_case("only_I_and_D", [(I, 5), (D, 9), (I, 1)]))
    C.append(_case("only_one_I", [(I, 5)]))
    C.append(_case("empty_cigar_between_two_real_jobs", []))
    C.append(_case("after_the_empty_cigar", [(M, 66)], mm=[64]))
    # ---- N
    C.append(_case("N_against_N_is_EQ", [(M, 40)], q_n=[10, 20], t_n=[10, 20]))
    C.append(_case("N_against_N_is_EQ_beside_a_mismatch", [(M, 40)], q_n=[10, 20], t_n=[10, 20], mm=[11]))
    C.append(_case("N_against_a_base_is_X", [(M, 40)], q_n=[10], t_n=[30]))
    # ---- mixed shapes at several mismatch rates
    mixed = [(M, 120), (I, 2), (M, 300), (D, 11), (M, 95), (I, 1), (M, 64), (N, 20), (M, T + 3)]
    for rate in (0.01, 0.1, 0.5, 0.9):
        C.append(_case("mixed_mismatch_rate_%g" % rate, mixed, mm_rate=rate, q_n=[5], t_n=[200]))
    C.append(_case("mixed_all_mismatch_in_place", mixed, all_mm=True))
    return C


def batch70():
    """70 jobs of mixed sizes in one call: empty CIGARs, exactly one tile, exactly 4 tiles, both branches"""
    rng = np.random.default_rng(170)
    C = []
    for k in range(70):
        if k in (3, 69):
            ops = []
        elif k == 10:
            ops = [(M, T)]
        elif k == 20:
            ops = [(M, 4 * T)]
        else:
            ops = []
            for i in range(int(rng.integers(1, 30))):
                ops.append((M, int(rng.integers(0, 200))))
                if rng.random() < 0.8:
                    ops.append((int(rng.choice([I, D, D, N])), int(rng.integers(0, 90))))
        C.append(_case("batch70_%d" % k, ops, mm_rate=(0.0, 0.07, 0.3)[k % 3]))
    return C


def long_40k():
    """one 40 000-column job (the long class under the default routing) with sparse mismatches, between indels"""
    rng = np.random.default_rng(9)
    ops = []
    for k in range(20):
        ops += [(M, 2000), (int(rng.choice([I, D])), int(rng.integers(1, 300)))]
    return ("long_40k",) + X.build(ops, seed=9, mm_rate=0.02, t_n=[5, 30000], q_n=[777])


def m_columns(cig):
    return int(sum(int(w) >> 4 for w in cig if (int(w) & 0xf) == 0))


def restated(cig, q, t):
    """mm_update_cigar_eqx from its rules, with numpy: -> (new CIGAR, in_place)"""
    cig = [int(w) for w in cig]
    runs_of = []                      # per op: None (not M) or its runs [(len, code)]
    qo = to = 0
    for w in cig:
        op, ln = w & 0xf, w >> 4
        if op == 0:
            e = np.asarray(q[qo:qo + ln]) == np.asarray(t[to:to + ln])
            cut = np.flatnonzero(e[1:] != e[:-1]) + 1 if ln else np.zeros(0, int)
            edges = np.concatenate([[0], cut, [ln]]).astype(int) if ln else np.zeros(1, int)
            runs_of.append([(int(edges[i + 1] - edges[i]), EQ if e[edges[i]] else DIFF) for i in range(len(edges) - 1)])
            qo += ln; to += ln
        else:
            runs_of.append(None)
            if op == 1:
                qo += ln
            elif op in (2, 3):
                to += ln
    n_m = sum(r is not None for r in runs_of); n_eqx = sum(len(r) for r in runs_of if r is not None)
    if n_eqx == n_m:
        return np.array([(w >> 4) << 4 | EQ if (w & 0xf) == 0 else w for w in cig], np.uint32), 1
    out = []
    for w, r in zip(cig, runs_of):
        out += [w] if r is None else [ln << 4 | code for ln, code in r]
    return np.array(out, np.uint32), 0
