"""Named, deterministic cases for the cs:Z / MD:Z bodies over final CIGARs (csrc/cigar_cs.h, csrc/cs_kernel.h; write_cs_core / write_MD_core, src/format.c:141-218),
shared by the emulator and the GPU tests, and a restatement of the rules in Python that owes nothing to the C header. A case is (name, cigar, q, t): BAM-encoded
ops, both sequences as 0..4 codes of exactly the CIGAR's extent plus 16 bytes of N padding (extracases.build). Names say what a case pins. T is the library's
default tile size; cases in which a tile matters exist for a tile of 64 columns and for T, laid out around both. In a CIGAR that is one M op, column c of the
kernels' column space is M column c in every mode (cs_kernel.h)."""
import zlib
import numpy as np
import extracases as X

T = X.T
TILES = (64, T)
M, I, D, N = X.M, X.I, X.D, X.N
EQ, XX = 7, 8
SHORT, LONG, MD = 0, 1, 2
MODES = (SHORT, LONG, MD)
LOW, UP = b"acgtn", b"ACGTN"


# ---- the rules, restated ------------------------------------------------------------------------------------------------------------------
def restated(mode, cig, q, t):
    """the body of the tag as bytes. cs: the identical run belongs to one op of code 0 / 7 / 8; MD: one run over the whole CIGAR, through I and N"""
    q = np.minimum(np.asarray(q, np.uint8), 4); t = np.minimum(np.asarray(t, np.uint8), 4)
    out = []
    qo = to = 0
    md_run = 0
    for w in cig:
        op, ln = int(w) & 0xf, int(w) >> 4
        assert op in (0, 1, 2, 3, 7, 8)
        if op in (0, 7, 8):
            qs, ts = q[qo:qo + ln], t[to:to + ln]
            prev = 0
            for p in list(np.flatnonzero(qs != ts)) + [ln]:
                p = int(p)
                same = p - prev                              # identical columns [prev, p)
                if mode == MD:
                    md_run += same
                    if p < ln:
                        out.append(b"%d" % md_run + UP[ts[p]:ts[p] + 1]); md_run = 0
                else:
                    if same > 0:
                        out.append(b":%d" % same if mode == SHORT else b"=" + bytes(UP[c] for c in qs[prev:p]))
                    if p < ln:
                        out.append(b"*" + LOW[ts[p]:ts[p] + 1] + LOW[qs[p]:qs[p] + 1])
                prev = p + 1
            qo += ln; to += ln
        elif op == 1:
            if mode != MD:
                out.append(b"+" + bytes(LOW[c] for c in q[qo:qo + ln]))
            qo += ln
        elif op == 2:
            if mode == MD:
                out.append(b"%d^" % md_run + bytes(UP[c] for c in t[to:to + ln])); md_run = 0
            else:
                out.append(b"-" + bytes(LOW[c] for c in t[to:to + ln]))
            to += ln
        else:
            if mode != MD:
                assert ln >= 2
                out.append(b"~" + bytes(LOW[c] for c in t[to:to + 2]) + b"%d" % ln + bytes(LOW[c] for c in t[to + ln - 2:to + ln]))
            to += ln
    if mode == MD and md_run > 0:
        out.append(b"%d" % md_run)
    return b"".join(out)


def bound(cig):
    """bytes no body exceeds (wm_cigar_cs_bound, restated)"""
    return 11 + sum((ln + 12) if op in (1, 2) else 16 if op == 3 else 3 * ln + 12 for op, ln in ((int(w) & 0xf, int(w) >> 4) for w in cig))


def columns(mode, cig):
    """columns of the kernels' column space (cs_kernel.h): what routes a job"""
    n = 1
    for w in cig:
        op, ln = int(w) & 0xf, int(w) >> 4
        if op in (0, 7, 8):
            n += ln + (mode != MD)
        elif op == 2 or (op == 1 and mode != MD):
            n += ln + 1
        elif op == 3 and mode != MD:
            n += 1
    return n


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def _case(name, ops, codes=None, **kw):
    cig, q, t = X.build(ops, seed=zlib.crc32(name.encode()), **kw)
    if codes is not None:                                    # relabel M ops as = / X, as --eqx leaves them (or against the bases)
        cig = np.array([(int(w) >> 4) << 4 | c for w, c in zip(cig, codes)], np.uint32)
    return (name, cig, q, t)


def make_cases():
    C = []
    # ---- single M op
    C.append(_case("single_M_all_match", [(M, 100)]))
    C.append(_case("single_M_all_mismatch", [(M, 70)], all_mm=True))
    C.append(_case("single_M_one_mismatch_first_column", [(M, 100)], mm=[0]))
    C.append(_case("single_M_one_mismatch_last_column", [(M, 100)], mm=[99]))
    C.append(_case("single_M_one_mismatch_middle_column", [(M, 100)], mm=[50]))
    for n in (1, 2, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1):
        C.append(_case("single_M_%d_random_mismatches" % n, [(M, n)], mm_rate=0.15))
    # ---- runs at tile edges and digit widths
    for e in TILES:
        share = e // 64
        for z, tag in ((-1, "one_before"), (0, "at"), (1, "one_after")):
            C.append(_case("run_ends_%s_a_lanes_share_tile_%d" % (tag, e), [(M, 3 * e)], mm=[2, 5 * share + z, 5 * share + z + 1, 3 * e - 2]))
            C.append(_case("run_ends_%s_a_tile_edge_%d" % (tag, e), [(M, 3 * e)], mm=[2, e + z, 2 * e + z, 3 * e - 2]))
        C.append(_case("run_spans_three_tiles_middle_one_without_a_break_%d" % e, [(M, 3 * e)], mm=[e - 5, 2 * e + 6]))
        for w in (10, 100, 1000):
            edge = e * ((w + 1 + e - 1) // e)                # the first tile edge with w columns in front of it
            C.append(_case("run_%d_to_%d_completed_across_a_tile_edge_%d" % (w - 1, w, e), [(M, edge + 40)], mm=[edge - w, edge + 1, edge + 3]))
    C.append(_case("run_of_100000", [(M, 100050)], mm=[7, 100008, 100030]))
    # ---- MD carried across ops
    for e in TILES:
        C.append(_case("md_run_carried_across_I_%d" % e, [(M, e - 3), (I, 5), (M, e + 9)], mm=[1, 2 * e]))
        C.append(_case("md_run_carried_across_N_%d" % e, [(M, e - 3), (N, 77), (M, e + 9)], mm=[1, 2 * e]))
        C.append(_case("md_run_carried_across_an_op_boundary_on_a_tile_edge_%d" % e, [(M, e), (M, e), (M, 7)], mm=[3, 2 * e + 2]))
    C.append(_case("md_zero_before_a_first_column_mismatch_and_between_adjacent_ones", [(M, 30)], mm=[0, 1, 2, 10, 11]))
    C.append(_case("md_mismatch_right_after_a_D", [(M, 5), (D, 2), (M, 9)], mm=[5]))
    C.append(_case("md_trailing_run_of_0_not_printed", [(M, 12)], mm=[11]))
    C.append(_case("md_trailing_D", [(M, 12), (D, 3)], mm=[4]))
    # ---- cs at op boundaries
    C.append(_case("cs_flushes_at_an_op_boundary", [(M, 10), (M, 10)]))
    C.append(_case("cs_flushes_at_an_op_boundary_under_eqx_ops", [(M, 10), (M, 1), (M, 9)], codes=[EQ, XX, EQ], mm=[10]))
    C.append(_case("X_op_over_equal_bases_and_EQ_op_over_unequal_ones", [(M, 8), (M, 6), (M, 5)], codes=[XX, EQ, 0], mm=[9, 10]))
    for e in TILES:
        C.append(_case("op_boundaries_around_a_tile_edge_%d" % e, [(M, e - 2), (M, 1), (M, 1), (M, 1), (M, e)], mm=[e - 1, e + 30]))
    # ---- gap ops
    for n in (1, 63, 64, 65, 130, T + 1):
        C.append(_case("I_and_D_of_%d" % n, [(M, 9), (I, n), (M, 11), (D, n), (M, 6)], mm=[3, 12]))
    C.append(_case("zero_length_M_I_D", [(M, 20), (I, 0), (M, 0), (D, 0), (M, 20), (D, 0), (I, 0)], mm=[25]))
    C.append(_case("leading_and_trailing_gaps", [(I, 3), (D, 2), (M, 40), (D, 4), (I, 70)], mm=[0, 39]))
    C.append(_case("only_I_and_D", [(I, 5), (D, 9), (I, 1)]))
    C.append(_case("only_D", [(D, 3)]))
    for e in TILES:
        for n in (2, 3, 99, 100000):
            # cs column of the intron = e - 1 (M columns + the flush), so its flanks straddle the tile edge in the target
            C.append(_case("intron_%d_on_a_tile_edge_%d" % (n, e), [(M, e - 2), (N, n), (M, e + 2)], mm=[e - 3, e - 2]))
    # ---- N bases
    C.append(_case("N_against_N", [(M, 40)], q_n=[11, 12], t_n=[11, 12]))
    C.append(_case("N_against_N_beside_a_mismatch", [(M, 40)], q_n=[11], t_n=[11], mm=[12]))
    C.append(_case("N_against_a_base", [(M, 40), (I, 3), (M, 5), (D, 3), (M, 5)], q_n=[10, 41], t_n=[30, 46]))
    # ---- jobs
    C.append(_case("empty_cigar_between_two_real_jobs", []))
    mixed = [(M, 120), (I, 2), (M, 300), (D, 11), (M, 95), (N, 1234), (M, 64), (I, 1), (M, 700)]
    for rate in (0.01, 0.1, 0.5, 0.9):
        C.append(_case("mixed_shapes_mismatch_rate_%g" % rate, mixed, mm_rate=rate))
    return C


def no_short_introns(cig):
    """an N op shorter than 2 is an error in the cs modes (src/format.c:180): such an op becomes a D, which consumes the same target"""
    return np.array([(int(w) & ~0xf) | 2 if (int(w) & 0xf) == 3 and (int(w) >> 4) < 2 else int(w) for w in cig], np.uint32)


def batch70():
    return [(c[0].replace("batch70", "cs_batch70"), no_short_introns(c[1]), c[2], c[3]) for c in X.batch70()]


def long_40k():
    ops = []
    for k in range(40):
        ops += [(M, 1000)] + ([(I, 3)] if k % 3 == 0 else [(D, 40)] if k % 3 == 1 else [(N, 500)])
    return _case("long_40k", ops[:-1], mm_rate=0.03)


def pack(cases):
    """cases -> the arrays of a byte-form call: q_off, t_off, cig_off, n_cigar, seqs, cigars, ops"""
    q_off, t_off, cig_off, n_cig, seqs, cigs = [], [], [], [], [], []
    at = ops = 0
    for _, cig, q, t in cases:
        q_off.append(at); seqs.append(q); at += len(q)
        t_off.append(at); seqs.append(t); at += len(t)
        cig_off.append(ops); n_cig.append(len(cig)); cigs.append(cig); ops += len(cig)
    cigs = np.concatenate(cigs + [np.zeros(1, np.uint32)]).astype(np.uint32)
    return (np.array(q_off, np.uint32), np.array(t_off, np.uint32), np.array(cig_off, np.uint32), np.array(n_cig, np.int32),
            np.ascontiguousarray(np.concatenate(seqs)), cigs, ops)
