"""Named, deterministic cases for the scan of mm_update_extra over final CIGARs (csrc/extra_kernel.h; src/align.c:240-286), shared by the emulator and
the GPU tests. A case is (name, cigar, q, t, score): BAM-encoded ops, both sequences as 0..4 codes of exactly the CIGAR's extent plus 16 bytes of N
padding, score = (match, mismatch, ambi, q, e) as literal values. Names say what a case pins. T is the library's default tile size; the tests also run
every case at a tile of 64 columns, so the tile-edge cases are laid out around both."""
import zlib
import numpy as np

T = 512                                  # default tile_cols (wm_extra_tile_cols() right after loading; the tests assert it)
ONT = (2, -4, -1, 4, 2)                  # map-ont
ASM20 = (1, -4, -1, 6, 2)
SPLICE = (1, -2, -1, 2, 1)
M, I, D, N = 0, 1, 2, 3
PAD = 16


def build(ops, mm=(), q_n=(), t_n=(), seed=0, mm_rate=0.0, all_mm=False):
    """sequences for `ops` = [(op, len)]: the query copies the target along M, except at the M columns listed in `mm` (numbered over M ops only), at
    random ones (mm_rate), or everywhere (all_mm); q_n / t_n = query / target offsets that become N"""
    rng = np.random.default_rng(seed)
    tl = sum(l for o, l in ops if o in (M, D, N)); ql = sum(l for o, l in ops if o in (M, I))
    t = rng.integers(0, 4, tl).astype(np.uint8)
    q = np.zeros(ql, np.uint8)
    qi = ti = mc = 0
    mm = set(mm)
    for o, l in ops:
        if o == M:
            seg = t[ti:ti + l].copy()
            for c in range(l):
                if all_mm or (mc + c) in mm or (mm_rate and rng.random() < mm_rate):
                    seg[c] = (seg[c] + 1 + int(rng.integers(0, 3))) % 4
            q[qi:qi + l] = seg; qi += l; ti += l; mc += l
        elif o == I:
            q[qi:qi + l] = rng.integers(0, 4, l); qi += l
        elif o in (D, N):
            ti += l
    for p in q_n:
        q[p] = 4
    for p in t_n:
        t[p] = 4
    cig = np.array([l << 4 | o for o, l in ops], np.uint32)
    return cig, np.concatenate([q, np.full(PAD, 4, np.uint8)]), np.concatenate([t, np.full(PAD, 4, np.uint8)])


def _case(name, ops, score=ONT, **kw):
    return (name,) + build(ops, seed=zlib.crc32(name.encode()), **kw) + (score,)


def make_cases():
    C = []
    # ---- tile-edge lengths: a single M around the lane / wave / tile sizes
    for n in (1, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 3 * T + 1):
        C.append(_case("single_M_%d" % n, [(M, n)], mm_rate=0.05))
    # ---- operator order: one mismatch on the last column of a tile, one on the first of the next (asymmetric: a swapped left / right shows)
    for e in (64, T):
        C.append(_case("order_mismatch_last_col_of_tile_%d" % e, [(M, 2 * e)], mm=[e - 1]))
        C.append(_case("order_mismatch_first_col_of_next_tile_%d" % e, [(M, 2 * e)], mm=[e]))
        C.append(_case("order_mismatch_both_sides_of_edge_%d" % e, [(M, 2 * e + 3)], mm=[e - 1, e]))
        C.append(_case("order_late_peak_after_early_dip_%d" % e, [(M, 2 * e)], mm=list(range(3, 9)) + [e + 1]))
    # ---- clamp at a tile edge: s = 8 after four matches, two mismatches take it to exactly 0 (s + d == 0) at column z, a third one below 0
    for e in (64, T):
        for z, tag in ((e - 2, "one_before"), (e - 1, "at"), (e, "one_after")):
            pre = list(range(0, z - 5))                      # mismatches from the start: s stays 0 until the four matches [z - 5, z - 1)
            C.append(_case("clamp_exact_zero_%s_edge_%d" % (tag, e), [(M, 2 * e)], mm=pre + [z - 1, z]))
            C.append(_case("clamp_below_zero_%s_edge_%d" % (tag, e), [(M, 2 * e)], mm=pre + [z - 1, z, z + 1]))
    # ---- position of the maximum
    C.append(_case("max_on_first_column", [(M, 200)], mm=list(range(1, 200))))
    C.append(_case("max_on_last_column", [(M, 200)], mm=list(range(0, 199))))
    C.append(_case("max_attained_twice", [(M, 130)], mm=[2] + list(range(5, 130))))
    C.append(_case("max_attained_twice_across_tile_64", [(M, 130)], mm=list(range(0, 62)) + [64] + list(range(67, 130))))
    # ---- all mismatches (dp_max = 0) / all matches
    C.append(_case("all_mismatches", [(M, T + 70)], all_mm=True))
    C.append(_case("all_matches", [(M, T + 70)]))
    # ---- gap ops
    for e in (64, T):
        C.append(_case("gap_first_element_of_tile_%d" % e, [(M, e), (I, 3), (M, e - 1), (D, 2), (M, 7)]))
        C.append(_case("gap_last_element_of_tile_%d" % e, [(M, e - 1), (D, 3), (M, e - 1), (I, 2), (M, 9)]))
    C.append(_case("gap_costs_more_than_s", [(M, 2), (D, 10), (M, 30)]))
    C.append(_case("gap_costs_less_than_s", [(M, 50), (I, 1), (M, 30)]))
    C.append(_case("gap_costs_exactly_s", [(M, 5), (I, 3), (M, 30)]))                 # s = 10, q + 3 e = 10
    C.append(_case("I_directly_followed_by_D", [(M, 40), (I, 4), (D, 7), (M, 40)]))
    C.append(_case("D_directly_followed_by_I_at_the_start", [(D, 2), (I, 3), (M, 20)]))
    C.append(_case("len_0_ops", [(M, 20), (I, 0), (M, 0), (D, 0), (M, 20), (N, 0), (M, 5)]))
    C.append(_case("D_5000_with_N_in_the_deleted_target", [(M, 100), (D, 5000), (M, 100)], t_n=[100, 101, 163, 164, 165, 1000, 2049, 5098, 5099], score=ASM20))
    C.append(_case("I_300_with_N_in_the_query", [(M, 77), (I, 300), (M, 90)], q_n=[77, 78, 140, 141, 142, 300, 376]))
    C.append(_case("D_64_65_128_exact_gap_chunks", [(M, 9), (D, 64), (M, 9), (D, 65), (M, 9), (I, 128), (M, 9), (I, 129), (M, 3)], t_n=[9 + 63, 9 + 64 + 9 + 64], q_n=[27 + 127, 27 + 128 + 9 + 128]))
    # ---- introns and unknown ops
    C.append(_case("N_op_between_Ms", [(M, 60), (N, 900), (M, 70), (N, 3), (M, 10)], score=SPLICE, mm_rate=0.05))
    C.append(_case("op_codes_above_3", [(4, 7), (M, 30), (7, 5), (M, 40), (5, 9)], mm_rate=0.05))
    # ---- ambiguous bases in M, ambi = 0 and -2
    for amb in (0, -2):
        sc = (2, -4, amb, 4, 2)
        C.append(_case("M_target_N_ambi_%d" % amb, [(M, 90)], t_n=[0, 40, 89], score=sc))
        C.append(_case("M_query_N_ambi_%d" % amb, [(M, 90)], q_n=[1, 63, 64], score=sc))
        C.append(_case("M_both_N_ambi_%d" % amb, [(M, 90)], q_n=[10, 70], t_n=[10, 71], score=sc))
    # ---- scoring sets
    mixed = [(M, 120), (I, 2), (M, 300), (D, 11), (M, 95), (I, 1), (M, 64)]
    for nm, sc in (("map_ont", ONT), ("asm20", ASM20), ("splice", SPLICE), ("match_0", (0, -3, -1, 4, 2)), ("match_negative", (-1, -4, -2, 4, 2))):
        C.append(_case("scoring_%s" % nm, mixed, score=sc, mm_rate=0.06, q_n=[5], t_n=[200]))
    return C


def batch70():
    """batch shape: 70 jobs of mixed sizes in one call, among them n_cigar = 0, exactly one tile and exactly 4 tiles"""
    rng = np.random.default_rng(70)
    C = []
    for k in range(70):
        if k == 3 or k == 69:
            ops = []
        elif k == 10:
            ops = [(M, T)]
        elif k == 20:
            ops = [(M, 4 * T)]
        else:
            ops = []
            for i in range(int(rng.integers(1, 30))):
                ops.append((M, int(rng.integers(1, 200))))
                if rng.random() < 0.8:
                    ops.append((int(rng.choice([I, D, D, N])), int(rng.integers(1, 90))))
        C.append(_case("batch70_%d" % k, ops, mm_rate=0.07, score=ONT))
    return C


# ---- position form: (name, cigar, read, q_pos, contig, t_pos, score). The query is the two-strand space of `read` from q_pos on, the target the contig from t_pos on.
def two_strand(read, p0, n):
    L = len(read)
    out = np.full(n, 4, np.uint8)
    for i in range(n):
        p = p0 + i
        if 0 <= p < L:
            out[i] = read[p]
        elif L <= p < 2 * L:
            c = read[2 * L - 1 - p]
            out[i] = 3 - c if c < 4 else 4
    return out


def make_pos_cases():
    rng = np.random.default_rng(77)
    L = 700
    read = rng.integers(0, 4, L).astype(np.uint8)
    read[[5, 333, 334, 640, 699]] = 4
    P = []

    def pos_case(name, ops, q_pos, t_pos, contig_len, score=ONT, t_n=()):
        ql = sum(l for o, l in ops if o in (M, I)); tl = sum(l for o, l in ops if o in (M, D, N))
        q = two_strand(read, q_pos, ql)
        contig = rng.integers(0, 4, contig_len).astype(np.uint8)
        qi, ti = 0, t_pos                                   # the target copies the query along M (sparse mismatches)
        for o, l in ops:
            if o == M:
                seg = q[qi:qi + l].copy(); bad = seg > 3; seg[bad] = 0
                flip = rng.random(l) < 0.06; seg[flip] = (seg[flip] + 1) % 4
                contig[ti:ti + l] = seg; qi += l; ti += l
            elif o == I:
                qi += l
            else:
                ti += l
        for p in t_n:
            contig[t_pos + p] = 4
        assert t_pos + tl <= contig_len
        P.append((name, np.array([l << 4 | o for o, l in ops], np.uint32), read, q_pos, contig, t_pos, score))

    ops = [(M, 150), (I, 70), (M, 130), (D, 140), (M, 90)]
    pos_case("pos_forward_strand", ops, 20, 40, 900, t_n=[3, 300, 301, 420])
    pos_case("pos_reverse_strand", ops, L + 100, 11, 900, t_n=[150, 289])
    pos_case("pos_q_3_bases_before_strand_1", ops, L - 3, 5, 900)
    pos_case("pos_q_3_bases_before_strand_0_is_padding", ops, -3, 5, 900)
    pos_case("pos_q_runs_off_the_end_of_strand_1", [(M, 60), (I, 30)], 2 * L - 80, 0, 100)
    for r in range(8):
        pos_case("pos_t_pos_mod_8_is_%d" % r, ops, 33 + r, 64 + r, 900, score=ASM20, t_n=[281 + r, 282 + r, 350])
    tl = sum(l for o, l in ops if o in (M, D, N))
    pos_case("pos_target_ends_at_the_contigs_last_base", ops, 10, 777 - tl, 777, t_n=[tl - 1])
    pos_case("pos_target_ends_with_a_deletion_at_the_last_base", [(M, 50), (D, 75)], 10, 1000 - 125, 1000, t_n=[124, 60])
    return P


# ---- the reference's own mm_update_extra (oracle/ref_align_shim.cpp; only where oracle/_ref is built) -----------------------------------------
def raw_alignments_for_the_reference():
    """[(cigar, q, t, score)]: the named cases and the batch the reference can take (match > 0, ops M / I / D / N, a CIGAR at all), plus 150 random alignments"""
    from test_host_simd import random_alignment
    rng = np.random.default_rng(32)
    raw = [(c[1], c[2], c[3], tuple(c[4])) for c in make_cases() + batch70() if len(c[1]) and c[4][0] > 0 and all((int(w) & 0xf) <= 3 for w in c[1])]
    for it in range(150):
        cig, q, t = random_alignment(rng, int(rng.integers(1, 60)), 0.0 if it % 3 else 0.02)
        raw.append((cig, np.concatenate([q, np.full(PAD, 4, np.uint8)]), np.concatenate([t, np.full(PAD, 4, np.uint8)]), ((2, -4, -1, 4, 2), (1, -9, -2, 16, 2))[it % 2]))
    return raw


def through_the_reference(R, raw):
    """every raw alignment through refshim_update_extra (mm_fix_cigar + the scan, rev = 0) -> cases holding the CIGAR it leaves and the sequences shifted by its
    qs / rs, and what it computed for each: (blen, mlen, n_ambi, dp_max)"""
    import ctypes as C
    import wmtest as W
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
    R.refshim_update_extra.argtypes = [C.c_int] * 5 + [W.u8p, W.u8p, W.i8p, C.c_int, C.c_int] + [C.c_uint32, W.u32p, i32p, W.u32p, C.c_int, C.POINTER(C.c_int)]
    cases, wants = [], []
    for cig, q, t, score in raw:
        mat = W.simple_mat(score[0], -score[1], -score[2])
        ql = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 1)); tl = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 2, 3))
        o = np.zeros(6, np.int32); c1 = np.zeros(len(cig) + 4, np.uint32); n1 = C.c_int()
        R.refshim_update_extra(0, 100, 100 + ql, 1000, 1000 + tl, np.ascontiguousarray(q), np.ascontiguousarray(t), mat, score[3], score[4], len(cig),
                               np.ascontiguousarray(cig, np.uint32), o, c1, len(c1), C.byref(n1))
        qs, rs = int(o[4]) - 100, int(o[5]) - 1000
        cases.append(("ref_%d" % len(cases), c1[:n1.value].copy(), np.ascontiguousarray(q[qs:]), np.ascontiguousarray(t[rs:]), score))
        wants.append(tuple(int(v) for v in o[:4]))
    return cases, wants
