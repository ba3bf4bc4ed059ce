"""Deterministic edge cases of the splice-aware extension (ksw_exts2_sse, src/ksw2_exts2_sse.c; ksw_exts2_kernel.h), shared by the oracle-vs-reference,
emulator and GPU tests. A case is a dict in the format of kswcases.make_splice_cases (q, t, a, b, q_, e, q2, noncan, junc_bonus, zdrop, flag, junc) plus
`name`, and `sc_ambi` (the N score as mat[24] holds it, <= 0; 0 means -e). Nothing here calls the oracle: the tests do, and
tests/test_exts2_edges_emu.py asserts on the oracle alone that every edge below changes the result against its neighbour (PAIRS, JUNC_*).
Line numbers: `:N` = src/ksw2_exts2_sse.c, `k:N` = winnowmap_amd/csrc/ksw_exts2_kernel.h."""
import numpy as np

FOR, REV, FLANK, RIGHT, APPROX, EXTZ, REVC = 0x100, 0x200, 0x400, 0x02, 0x08, 0x40, 0x80
A_, C_, G_, T_ = 0, 1, 2, 3

# (a, b, q, e, q2, noncan, junc_bonus)
SPLICE = (1, 2, 2, 1, 32, 9, 9)              # the splice preset (src/options.c:117-127)
CHEAP = (1, 2, 4, 3, 8, 9, 9)                # an intron (8) is cheaper than a deletion of two bases (10): signals decide on operands of a few bases; long_thres 1
BONUS = (1, 2, 2, 1, 8, 5, 20)               # an annotated junction is worth more than the intron costs
LT1 = (1, 2, 2, 2, 6, 9, 9)                  # q2 - q = 2 e: long_thres 1, long_diff -2 (:86-89)
LT9 = (1, 2, 4, 3, 32, 9, 9)                 # long_thres 9, long_diff -1
LT124 = (1, 2, 2, 1, 127, 9, 9)              # long_thres 124; q2 at the top of int8
LTMIN = (1, 2, 2, 2, 5, 9, 9)                # the least q2 the reference takes: q + e + 1 (:66); long_thres 1, long_diff -1
UNIT = (1, 1, 1, 1, 3, 2, 2)                 # everything costs about the same: ties everywhere


def long_thres(sc):
    """:86-88, k:51-52 (= the backtrack's min_intron, k:222-223)"""
    q, e, q2 = sc[2], sc[3], sc[4]
    lt = (q2 - q) // e - 1
    return lt + 1 if q2 > q + e + lt * e else lt


def _arr(x):
    return np.ascontiguousarray(np.asarray(x, np.uint8))


def _case(name, q, t, sc=SPLICE, flag=FOR, zdrop=-1, junc=None, sc_ambi=-1):
    q, t = _arr(q), _arr(t)
    assert len(q) > 0 and len(t) > 0 and (junc is None or len(junc) == len(t)), name
    return dict(name=name, q=q, t=t, a=sc[0], b=sc[1], q_=sc[2], e=sc[3], q2=sc[4], noncan=sc[5], junc_bonus=sc[6], zdrop=zdrop, flag=flag,
                junc=None if junc is None else _arr(junc), sc_ambi=sc_ambi)


def scoring_key(c):
    """what one wm_ksw_exts2_batch call shares"""
    return (c["a"], c["b"], c["sc_ambi"], c["q_"], c["e"], c["q2"], c["noncan"], c["junc_bonus"])


def _exon(rng, n):
    """random bases without G: no GT / AG / CT.AC motif of the forward strand forms by chance inside or across an exon boundary (CT / AC can: the REV cases
    take that as it comes)"""
    return rng.choice(np.array([A_, C_, T_], np.uint8), n)


FLAG_CYCLE = (FOR, REV | FLANK | REVC, FOR | EXTZ, FOR | APPROX, FOR | REV | RIGHT, FOR | FLANK | RIGHT | EXTZ, REV | APPROX | EXTZ, 0, FOR | REVC | EXTZ, REV)


def shape_cases():
    out = []
    rng = np.random.default_rng(7001)
    # qlen x tlen over 1..6: the donor loop `t < tlen - 4` (:118, k:77) is empty up to tlen = 4, the acceptor loop starts at t = 2 (:129, k:79); the target
    # is cut from AGTAAG / CAGGTA so that the motifs sit at every admitted and every refused position; once with the preset, once with the cheap intron
    k = 0
    for ql in range(1, 7):
        for tl in range(1, 7):
            t = ([A_, G_, T_, A_, A_, G_], [C_, A_, G_, G_, T_, A_])[(ql + tl) & 1][:tl]
            q = rng.integers(0, 4, ql)
            out.append(_case("tiny_%dx%d" % (ql, tl), q, t, SPLICE, FLAG_CYCLE[k % len(FLAG_CYCLE)], zdrop=(-1, 0, 5)[k % 3]))
            out.append(_case("tiny_cheap_%dx%d" % (ql, tl), q, t, CHEAP, FLAG_CYCLE[(k + 3) % len(FLAG_CYCLE)] | FLANK, zdrop=(-1, 0, 5)[(k + 1) % 3]))
            k += 1
    # lengths at the 16-lane hull (k:102), the n_col of the smaller operand (:78) and one / two / three / four 64-lane sweeps of a row (k:118), against a short
    # and a long partner. A long query (qlen >= tlen + 32) and a long target make st > 0: lane st - 1 is then read from the previous row when the hull start
    # has just moved on by 16 and is outside [last_st, last_en] on every other row (k:104-108)
    for L in (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193):
        ex = _exon(rng, L)
        h = L // 2
        intron = np.concatenate([[G_, T_, A_], _exon(rng, 54), [C_, A_, G_]])
        f = FLAG_CYCLE[k % len(FLAG_CYCLE)]
        k += 1
        out.append(_case("len_q%d_short_t" % L, ex, ex[:7], SPLICE, f, zdrop=-1))
        out.append(_case("len_t%d_short_q" % L, ex[3:10], ex, SPLICE, f | EXTZ, zdrop=-1))
        out.append(_case("len_q%d_spliced_t" % L, ex, np.concatenate([ex[:h], intron, ex[h:], _exon(rng, 8)]), SPLICE, FOR | (f & (RIGHT | APPROX | EXTZ)), zdrop=200))
        tq = ex.copy()
        tq[L // 3] = (tq[L // 3] + 1) % 4
        out.append(_case("len_t%d_long_q" % L, np.concatenate([tq, rng.integers(0, 4, 40 + L % 3)]), ex, SPLICE, f, zdrop=(-1, 30)[L & 1]))
    return out


def _spliced(rng, e1=12, e2=12, intron=()):
    ex1, ex2 = _exon(rng, e1), _exon(rng, e2)
    return np.concatenate([ex1, ex2]), np.concatenate([ex1, _arr(intron), ex2])


def signal_cases():
    """donor[t] prices an intron whose first base is t + 1, acceptor[t] one whose last base is t (:113-164, k:57-89)"""
    out = []
    rng = np.random.default_rng(7002)
    ex = _exon(rng, 12)
    # global jobs whose target runs 4 (3) bases past the query: those bases are a deletion (q + 4 e = 16) or, if the donor in front of them is admitted, an
    # intron (q2 = 8). GTAG at the end puts the donor at t = tlen - 5, the last one the loop `t < tlen - 4` admits (:118, k:77)
    out.append(_case("donor_at_tlen-5", ex, np.concatenate([ex, [G_, T_, A_, G_]]), CHEAP, FOR))
    # ... and GTA at the very end puts it at t = tlen - 4: not admitted, though all three of its bases exist. The acceptor at tlen - 1 is annotated, so only
    # the donor's price stands between the deletion (13) and the intron (8)
    jn = np.zeros(15, np.uint8)
    jn[14] = 2
    out.append(_case("donor_at_tlen-4", ex, np.concatenate([ex, [G_, T_, A_]]), CHEAP, FOR, junc=jn))
    # an intron that a junction annotation opens behind target base 0 (donor[0] = -5 + 20) and that ends in AG: at t = 2, the first acceptor the loop admits
    # (:129, k:79: the intron is worth 15 - 8), and at t = 1, which it does not (15 - 8 - 5). (A target that merely runs ahead of the query does not ask the
    # acceptor: the first column has its own price, see gap_schedule_cases)
    jn = np.zeros(15, np.uint8)
    jn[1] = 1
    out.append(_case("acceptor_at_2", np.concatenate([[T_], ex]), np.concatenate([[T_, A_, G_], ex]), BONUS, FOR, junc=jn))
    out.append(_case("acceptor_at_1", np.concatenate([[A_], ex]), np.concatenate([[A_, G_], ex]), BONUS, FOR, junc=jn[:14]))
    # the flank bases (:122, :133; mirrored :145, :156): GTA / GTG and yAG are free, GTC / GTT and rAG cost -noncan / 2 under SPLICE_FLANK, nothing without
    q, _ = _spliced(rng)
    for nm, d3, acc in (("GTA_CAG", A_, (C_, A_, G_)), ("GTG_TAG", G_, (T_, A_, G_)), ("GTC_CAG", C_, (C_, A_, G_)), ("GTT_TAG", T_, (T_, A_, G_)), ("GTA_AAG", A_, (A_, A_, G_)),
                        ("GTG_GAG", G_, (G_, A_, G_)), ("GTC_AAG", C_, (A_, A_, G_)), ("GTC_AAA", C_, (A_, A_, A_))):
        t = np.concatenate([q[:12], [G_, T_, d3], _exon(rng, 20), acc, q[12:]])
        for fl, fn in ((FOR | FLANK, "flank"), (FOR, "noflank"), (FOR | FLANK | RIGHT | EXTZ, "flank_right_extz"), (FOR | REV | FLANK | APPROX, "flank_both_approx")):
            # noncan 9: -noncan / 2 = -4 truncates toward zero where an arithmetic shift gives -5 (:114, k:58); noncan 8 has the same half and differs at the
            # sites with no motif (GTC_AAA); -5: a bonus of 2
            for nc in (9, 8, -5):
                out.append(_case("flank_%s_%s_nc%d" % (nm, fn, nc), q, t, CHEAP[:5] + (nc, 9), fl))
    # every motif under SPLICE_FOR, SPLICE_REV, both, and with REV_CIGAR (the mirrored motifs :141-158 on reversed operands)
    for nm, d, a in (("GT_AG", (G_, T_, A_), (C_, A_, G_)), ("CT_AC", (C_, T_, A_), (C_, A_, C_)), ("GA_TG", (G_, A_, C_), (A_, T_, G_)), ("CA_TC", (C_, A_, T_), (G_, T_, C_)),
                     ("none", (A_, A_, A_), (T_, T_, T_))):
        t = np.concatenate([q[:12], d, _exon(rng, 25), a, q[12:]])
        for fl, fn in ((FOR, "for"), (REV, "rev"), (FOR | REV, "both"), (FOR | REVC, "for_revc"), (REV | REVC, "rev_revc"), (FOR | REV | REVC | FLANK, "both_revc_flank"), (0, "off")):
            out.append(_case("motif_%s_%s" % (nm, fn), q, t, SPLICE[:4] + (14, 9, 9), fl))
    return out


JUNC_FLAGS = (("for", FOR), ("rev", REV), ("both", FOR | REV), ("for_revc", FOR | REVC), ("rev_revc", REV | REVC))
JUNC_BITS = (1, 2, 4, 8, 15)
JUNC_POS = ("0", "1", "tlen-2", "tlen-1")
# the bits a flag combination reads (:127, :138, :150, :161; k:62): donor | acceptor
JUNC_LIVE = {"for": 1 | 2, "rev": 8 | 4, "both": 15, "for_revc": 2 | 1, "rev_revc": 4 | 8}


def junction_cases():
    """one junction byte at t = 0, 1, tlen - 2, tlen - 1: the donor bit is read at t + 1 for t < tlen - 1, the acceptor bit at t for t < tlen (:126, :137;
    k:83-86). Bits 1, 2, 4, 8 one at a time and all four, under every flag combination; `junc_none_*` is the neighbour of them all"""
    out = []
    rng = np.random.default_rng(7003)
    q = _exon(rng, 14)
    t = np.concatenate([_exon(rng, 3), q[:7], _exon(rng, 9), q[7:], _exon(rng, 3)])
    for fn, fl in JUNC_FLAGS:
        out.append(_case("junc_none_%s" % fn, q, t, BONUS, fl, junc=np.zeros(len(t), np.uint8)))
        out.append(_case("junc_null_%s" % fn, q, t, BONUS, fl, junc=None))                 # junc = NULL against an all-zero array: equal results
        for bit in JUNC_BITS:
            for pn, p in zip(JUNC_POS, (0, 1, len(t) - 2, len(t) - 1)):
                jn = np.zeros(len(t), np.uint8)
                jn[p] = bit
                out.append(_case("junc_b%d_at_%s_%s" % (bit, pn, fn), q, t, BONUS, fl, junc=jn))
    # int8 wrap of donor / acceptor: -noncan + junc_bonus is stored as a byte (:128, k:89)
    jn = np.zeros(len(t), np.uint8)
    jn[[1, 9, 10, 18, 19, len(t) - 1]] = (1 | 8, 1 | 8, 2 | 4, 2 | 4, 15, 15)
    for nc, jb in ((127, -127), (127, 127), (100, 100), (-5, -127)):
        for fn, fl in (("both", FOR | REV), ("for_extz", FOR | EXTZ), ("rev_revc_right", REV | REVC | RIGHT)):
            out.append(_case("wrap_nc%d_jb%d_%s" % (nc, jb, fn), q, t, BONUS[:5] + (nc, jb), fl, junc=jn))
    return out


def gap_schedule_cases():
    """the first column's price of a leading target overhang changes from q + e (r + 1) to q2 at r = long_thres (:181-186, k:103), and the backtrack turns the
    target bases left over when the query is used up into N from min_intron + 1 of them on (src/ksw2.h:148, k:245)"""
    out = []
    rng = np.random.default_rng(7004)
    for nm, sc in (("lt1", LT1), ("lt9", LT9), ("lt124", LT124), ("ltmin", LTMIN)):
        lt = long_thres(sc)
        for rows in sorted(set(r for r in (lt - 1, lt, lt + 1, lt + 2, 4 * lt + 40) if r >= 1)):
            ql = 1 if rows < 3 else 2
            tl = rows + 1 - ql
            t = _exon(rng, tl)
            out.append(_case("rows_%s_%d" % (nm, rows), t[-ql:], t, sc, FOR, zdrop=-1))
        # global jobs whose target runs ahead of the query by about min_intron bases
        ex = _exon(rng, 10)
        for over in sorted(set(o for o in (lt - 1, lt, lt + 1, lt + 2) if o >= 1)):
            for fl, fn in ((FOR, "for"), (FOR | RIGHT, "right"), (REV | REVC, "rev_revc"), (FOR | APPROX, "approx")):
                out.append(_case("overhang_%s_%d_%s" % (nm, over, fn), ex, np.concatenate([_exon(np.random.default_rng(7100 + over), over), ex]), sc, fl, zdrop=-1))
    return out


ZDROP_FULL = 41        # see tie_and_zdrop_cases


def tie_and_zdrop_cases():
    out = []
    rng = np.random.default_rng(7005)
    # exact maximum on homopolymers and dinucleotide repeats: many cells of a row tie, the reference's SIMD order decides (:345-371, k:161-164: lane en0, then
    # residue groups of [st0, en1), then the tail), and a z-drop looks at whichever won (:375, k:185-186). Left- and right-aligned gaps
    for ql, tl in ((5, 5), (8, 5), (5, 8), (9, 9), (13, 9), (9, 13), (17, 16), (16, 17), (21, 30), (30, 21), (33, 33), (40, 70), (70, 40)):
        for fl, fn in ((FOR, "left"), (FOR | RIGHT, "right"), (FOR | EXTZ, "left_extz"), (FOR | RIGHT | EXTZ, "right_extz")):
            zd = (-1, 0, 1, 2, 3, 4)[(ql + tl + len(fn)) % 6]
            out.append(_case("homo_%dx%d_%s" % (ql, tl, fn), np.full(ql, A_), np.full(tl, A_), SPLICE, fl, zdrop=zd))
            out.append(_case("dinuc_%dx%d_%s" % (ql, tl, fn), np.tile([A_, C_], ql)[:ql], np.tile([A_, C_], tl)[1:tl + 1] if tl & 1 else np.tile([A_, C_], tl)[:tl], CHEAP, fl, zdrop=zd))
            out.append(_case("homo_gap_%dx%d_%s" % (ql, tl, fn), np.concatenate([np.full(ql, A_), [C_], np.full(3, A_)]), np.concatenate([np.full(tl, A_), [C_], np.full(3, A_)]), LT1, fl, zdrop=zd))
    # right-aligned gaps keep extending a deletion where extending and opening tie (`a >= 0` for `a > 0`, :309-315, k:49-50, k:150): the deletion moves to the
    # other side of the match. Found by a search against a kernel with the two thresholds exchanged, kept as they were found
    for i, (q, t, sc, fl) in enumerate((([C_], [A_, C_, A_, C_, C_, A_], SPLICE, FOR | RIGHT), ([A_], [C_, A_, A_, C_, G_], BONUS, FOR | RIGHT | REVC),
                                        ([C_, A_, G_], [C_, G_, T_, T_], UNIT, FOR | RIGHT), ([C_], [T_, C_, T_, C_, A_, C_, T_], BONUS, RIGHT),
                                        ([C_, C_], [C_, A_, C_, C_, A_], UNIT, FOR | RIGHT | REVC))):
        out.append(_case("right_extend_tie_%d" % i, q, t, sc, fl, zdrop=-1))
    # a row's maximum held by lane en1 — the first lane of the tail the four-lane groups leave over, which ranks below every group (:345-371, k:161) — and by
    # a lane of a group: the lane chosen is the new maximum's (max_t, max_q), or decides whether the z-drop test looks at the row at all. Found by a search
    # against a kernel that ranks lane en1 with the groups
    for i, (q, t, fl, zd) in enumerate((([1, 3, 1, 3, 1, 1, 3, 1, 0, 0], [1, 1, 3, 1, 3, 3], FOR | RIGHT | REVC, 3), ([0, 1, 0, 1, 0, 0, 1, 0], [0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 0], RIGHT, 2),
                                        ([1, 0, 0, 1, 0, 1, 0, 0, 0, 0], [0, 1, 1, 0, 1, 0, 1, 1, 1, 0], FOR, 2), ([3, 0, 1, 0, 1, 1, 3, 1, 3, 3, 0, 1], [3, 1, 0, 1, 0, 3, 0, 1, 3, 0, 0], RIGHT, 3))):
        out.append(_case("tail_lane_tie_%d" % i, q, t, UNIT, fl, zdrop=zd))
    # a matching prefix of 30 and a tail of 20 in which nothing matches (A against C): the maximum 30 stands at (29, 29); past it the best cell of a row
    # is 2 k lower on row 58 + 2 k (k mismatches) and 2 k + 3 lower on row 59 + 2 k (one gap base more), so the largest drop is that of row 97: 41. The test at
    # :375 passes e = 0: it fires when the drop EXCEEDS zdrop — never at 41, on row 97 at 40, on the first row past the maximum at 0 .. 2
    p = _exon(rng, 30)
    p[-1] = T_
    q, t = np.concatenate([p, np.full(20, A_)]), np.concatenate([p, np.full(20, C_)])
    for zd in (ZDROP_FULL, ZDROP_FULL - 1, 3, 2, 0, -1):
        for fl, fn in ((FOR | EXTZ, "extz"), (FOR, "global"), (FOR | EXTZ | RIGHT, "extz_right"), (FOR | EXTZ | REVC, "extz_revc")):
            out.append(_case("zdrop_%d_%s" % (zd, fn), q, t, SPLICE, fl, zdrop=zd))
    # extension-only jobs with no positive cell: max 0, max_t -1, no CIGAR (:400-405, k:204-205)
    for ql, tl in ((1, 1), (3, 7), (20, 20)):
        out.append(_case("nopos_%dx%d" % (ql, tl), np.full(ql, A_), np.full(tl, C_), SPLICE, FOR | EXTZ, zdrop=-1))
    return out


def scoring_limit_cases():
    """the reference returns without aligning when the lowest score of the matrix is below -2 (q + e) (:80-84): the sets ON the limit, mismatch and N score;
    the N score written as 0 (then -e, :74, k:50); a large match score"""
    out = []
    rng = np.random.default_rng(7006)
    q, t = _spliced(rng, 14, 14, np.concatenate([[G_, T_, A_], _exon(rng, 30), [C_, A_, G_]]))
    q = q.copy()
    t = t.copy()
    q[5] = 4
    t[20] = 4
    t[40] = (t[40] + 1) % 4 if t[40] != 1 else 0
    for nm, sc, amb in (("b_at_limit", (1, 6, 2, 1, 32, 9, 9), -1), ("ambi_0", SPLICE, 0), ("ambi_-1", SPLICE, -1), ("ambi_at_limit", SPLICE, -6),
                        ("ambi_at_limit_q0", (1, 2, 0, 1, 32, 9, 9), -2), ("a6", (6, 6, 2, 1, 32, 9, 9), -3), ("a6_cheap", (6, 2, 4, 3, 20, 9, 9), 0)):
        for fl in (FOR, FOR | EXTZ | RIGHT, FOR | APPROX):
            out.append(_case("limit_%s_%x" % (nm, fl), q, t, sc, fl, zdrop=200, sc_ambi=amb))
    return out


# scoring sets the reference refuses (:66, :84): (a, b, q, e, q2, sc_ambi) — mismatch or N score one below -2 (q + e) (with sc_ambi 0 the N score is -e), q2 not
# above q + e
REJECTED = (("b_past_limit", (1, 7, 2, 1, 32, -1)), ("ambi_past_limit", (1, 2, 2, 1, 32, -7)), ("ambi_past_limit_q0", (1, 2, 0, 1, 32, -3)), ("q2_at_q+e", (1, 2, 2, 1, 3, -1)))


def edge_cases():
    out = shape_cases() + signal_cases() + junction_cases() + gap_schedule_cases() + tie_and_zdrop_cases() + scoring_limit_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# (label, case, its neighbour): the oracle must tell them apart — in a field, or in the CIGAR
PAIRS = [("donor at tlen-5 / tlen-4", "donor_at_tlen-5", "donor_at_tlen-4"),
         ("acceptor at 2 / 1", "acceptor_at_2", "acceptor_at_1"),
         ("donor flank on / off", "flank_GTA_CAG_flank_nc9", "flank_GTC_CAG_flank_nc9"),
         ("acceptor flank on / off", "flank_GTA_CAG_flank_nc9", "flank_GTA_AAG_flank_nc9"),
         ("noncan 9 / 8 under FLANK", "flank_GTC_AAA_flank_nc9", "flank_GTC_AAA_flank_nc8"),
         ("zdrop at the drop / one less", "zdrop_%d_extz" % ZDROP_FULL, "zdrop_%d_extz" % (ZDROP_FULL - 1))] + \
        [("overhang min_intron / min_intron + 1 (%s)" % nm, "overhang_%s_%d_for" % (nm, long_thres(sc)), "overhang_%s_%d_for" % (nm, long_thres(sc) + 1))
         for nm, sc in (("lt1", LT1), ("lt9", LT9), ("lt124", LT124), ("ltmin", LTMIN))]


def long_intron_case(intron_len):
    """a 20-base and a 60-base exon joined in the query, GTA ... CAG of intron_len bases between them in the target, 10 bases of tail; splice preset,
    extension-only, exact maximum. With the maximum beyond target base 2^20 the lane of the maximum no longer fits 20 bits"""
    rng = np.random.default_rng(7007)
    e1, e2 = _exon(rng, 20), _exon(rng, 60)
    intron = rng.choice(np.array([A_, C_, T_], np.uint8), intron_len)
    intron[:3] = (G_, T_, A_)
    intron[-3:] = (C_, A_, G_)
    return _case("long_intron_%d" % intron_len, np.concatenate([e1, e2]), np.concatenate([e1, intron, e2, _exon(rng, 10)]), SPLICE, FOR | EXTZ, zdrop=-1)


def long_identity_case(n):
    """ksw_extd2 job: query == target, n bases, band 10, extension-only with exact maximum, map-ont scoring (kswcases format)"""
    s = np.random.default_rng(7008).integers(0, 4, n).astype(np.uint8)
    return dict(q=s, t=s.copy(), a=2, b=4, q_=4, e=2, q2=24, e2=1, w=10, zdrop=-1, end_bonus=0, flag=0x40)
