"""Named, deterministic cases for mm_fix_cigar on the device (csrc/fix_kernel.h; specification csrc/cigar_fix.h; src/align.c:91-167), shared by the emulator and
the GPU tests. A case is (name, raw cigar, q, t, score), the layout of extracases: BAM-encoded ops, both sequences as 0..4 codes of exactly the CIGAR's extent
plus 16 bytes of N padding. Each case is the smallest shape that pins one edge; where an edge needs particular bases, a seed is searched for with fix_py — the
short Python restatement of the loop below, which also counts the events the tests assert their inputs reach."""
import zlib
import numpy as np
import extracases as X

M, I, D, N = X.M, X.I, X.D, X.N
ONT, ASM20, SPLICE, PAD = X.ONT, X.ASM20, X.SPLICE, X.PAD
T = X.T


# ---- the loop, restated ------------------------------------------------------------------------------------------------------------------------
def fix_py(cig, q, t):
    """mm_fix_cigar on a list of BAM ops -> (cigar, qshift, tshift, changed, info). info: l = {k: (shift, prev_len)} of every eligible op, raw = {k: raw length of
    the M in front}, rewrites = starts of pass-2 rewrites, shrink, lead"""
    c = [int(w) for w in cig]
    n = len(c)
    info = {"l": {}, "raw": {}, "rewrites": [], "shrink": False, "lead": False}
    if n <= 1:
        return c, 0, 0, 0, info
    raw = list(c)
    qoff = toff = 0
    shrink = moved = False
    for k in range(n):
        op, ln = c[k] & 0xf, c[k] >> 4
        if ln == 0:
            shrink = True
        if op == 0:
            qoff += ln; toff += ln
        elif op in (1, 2):
            if 0 < k < n - 1 and c[k - 1] & 0xf == 0 and c[k + 1] & 0xf == 0:
                prev = c[k - 1] >> 4
                s, off = (q, qoff) if op == 1 else (t, toff)
                l = 0
                while l < prev and s[off - 1 - l] == s[off + ln - 1 - l]:
                    assert off - 1 - l >= 0
                    l += 1
                if l > 0:
                    c[k - 1] -= l << 4; c[k + 1] += l << 4; qoff -= l; toff -= l; moved = True
                if l == prev:
                    shrink = True
                info["l"][k] = (l, prev); info["raw"][k] = raw[k - 1] >> 4
            if op == 1:
                qoff += ln
            else:
                toff += ln
        elif op == 3:
            toff += ln
    k = 0
    while k + 2 < n:
        if c[k] & 0xf > 0 and (c[k] & 0xf) + (c[k + 1] & 0xf) == 3:
            s = [0, 0, 0]
            l = k
            while l < n and (c[l] & 0xf in (1, 2) or c[l] >> 4 == 0):
                s[c[l] & 0xf] += c[l] >> 4; l += 1
            if s[1] > 0 and s[2] > 0 and l - k > 2:
                info["rewrites"].append(k)
                c[k] = (s[1] << 4 | 1) & 0xffffffff; c[k + 1] = (s[2] << 4 | 2) & 0xffffffff
                for i in range(k + 2, l):
                    c[i] &= 0xf
                shrink = True
            k = l
        k += 1
    if shrink:
        c = [w for w in c if w >> 4]
        out = []
        for k in range(len(c)):
            if k == len(c) - 1 or c[k] & 0xf != c[k + 1] & 0xf:
                out.append(c[k])
            else:
                c[k + 1] = (c[k + 1] + (c[k] >> 4 << 4)) & 0xffffffff
        c = out
    qshift = tshift = 0
    lead = False
    if c and c[0] & 0xf in (1, 2):
        if c[0] & 0xf == 1:
            qshift = c[0] >> 4
        else:
            tshift = c[0] >> 4
        c = c[1:]; lead = True
    info["shrink"] = shrink; info["lead"] = lead
    changed = int(moved or shrink or lead)
    assert changed == int(c != raw)                        # `changed` is exactly "the CIGAR or its count differs"
    return c, qshift, tshift, changed, info


def events(info):
    ls = info["l"]
    return {"past_raw": any(l > info["raw"][k] for k, (l, p) in ls.items()), "over_64": any(l > 64 for l, p in ls.values()),
            "rewrite": bool(info["rewrites"]), "lead": info["lead"], "saturated": any(l == p for l, p in ls.values())}


# ---- builders ---------------------------------------------------------------------------------------------------------------------------------
def enc(ops):
    return np.array([l << 4 | o for o, l in ops], np.uint32)


def offsets(ops):
    """(qoff, toff) at the start of every op of the raw CIGAR"""
    out, qo, to = [], 0, 0
    for o, l in ops:
        out.append((qo, to))
        if o in (M, I):
            qo += l
        if o in (M, D, N):
            to += l
    return out


def set_run(seq, off, ln, r):
    """make exactly r bases match in the compare of an indel of ln bases at off: seq[off - 1 - j] == seq[off + ln - 1 - j] for j < r, not for j == r"""
    for j in range(r):
        seq[off - 1 - j] = seq[off + ln - 1 - j]
    if off - 1 - r >= 0:
        seq[off - 1 - r] = (seq[off + ln - 1 - r] + 1) % 4 if seq[off + ln - 1 - r] < 4 else 0


def padded(a):
    return np.concatenate([np.asarray(a, np.uint8), np.full(PAD, 4, np.uint8)])


def runs_case(name, ops, runs, score=ONT, edit=None):
    """a plausible alignment (the query copies the target along M, 3 % mismatches) in which op k matches exactly runs[k] bases (ops far enough apart)"""
    cig, q, t = X.build(ops, seed=zlib.crc32(name.encode()), mm_rate=0.03)
    at = offsets(ops)
    for k in sorted(runs):
        o, l = ops[k]
        set_run(q if o == I else t, at[k][0] if o == I else at[k][1], l, runs[k])
    if edit:
        edit(q, t)
    return (name, cig, q, t, score)


def letters_case(name, ops, letters, seed=0, score=ONT):
    """both sequences random over `letters` letters (1 = a homopolymer): shifts everywhere"""
    rng = np.random.default_rng(seed)
    at = offsets(ops + [(M, 0)])[-1]
    return (name, enc(ops), padded(rng.integers(0, letters, at[0])), padded(rng.integers(0, letters, at[1])), score)


def search(name, ops, pred, letters=2, score=ONT):
    """the first seed whose random sequences over `letters` letters make pred(info, fixed cigar) true"""
    for seed in range(4000):
        c = letters_case(name, ops, letters, seed, score)
        fixed, qs, ts, ch, info = fix_py(c[1], c[2], c[3])
        if pred(info, fixed):
            return c
    raise AssertionError("no seed for " + name)


def alternating(n_ops, m_len=3, first=M, gaps=(I, D), gap_len=1):
    ops = []
    for i in range(n_ops):
        even = i % 2 == 0
        if (first == M) == even:
            ops.append((M, m_len))
        else:
            ops.append((gaps[(i // 2) % len(gaps)], gap_len))
    return ops


def make_cases():
    C = []
    # ---- counts
    C.append(("n_cigar_0", enc([]), padded([]), padded([]), ONT))
    C.append(runs_case("n_cigar_1_M", [(M, 5)], {}))
    C.append(runs_case("n_cigar_1_5I_alone_is_untouched", [(I, 5)], {}))
    C.append(runs_case("n_cigar_1_5D_alone_is_untouched", [(D, 5)], {}))
    C.append(runs_case("n_cigar_2_M_I", [(M, 5), (I, 2)], {}))
    C.append(runs_case("n_cigar_2_I_M_loses_its_I", [(I, 2), (M, 5)], {}))
    # ---- pass 1
    mid = [(M, 10), (I, 2), (M, 10)]
    C.append(runs_case("I_shifted_partly", mid, {1: 4}))
    C.append(runs_case("I_shifted_fully_zeroes_the_M", mid, {1: 10}))
    C.append(runs_case("I_not_shifted", mid, {1: 0}))
    midd = [(M, 10), (D, 3), (M, 10)]
    C.append(runs_case("D_shifted_partly", midd, {1: 7}))
    C.append(runs_case("D_shifted_fully_zeroes_the_M", midd, {1: 10}))

    def other_says(seq_of, off_of, ln, r):
        def edit(q, t):
            set_run(q if seq_of == "q" else t, off_of, ln, r)
        return edit
    C.append(runs_case("I_decided_by_the_query_the_target_says_0", mid, {1: 5}, edit=other_says("t", 10, 2, 0)))
    C.append(runs_case("I_decided_by_the_query_the_target_says_more", mid, {1: 2}, edit=other_says("t", 10, 2, 8)))
    C.append(runs_case("D_decided_by_the_target_the_query_says_0", midd, {1: 5}, edit=other_says("q", 10, 3, 0)))
    C.append(runs_case("D_decided_by_the_target_the_query_says_more", midd, {1: 2}, edit=other_says("q", 10, 3, 8)))

    def n_both(q, t):
        q[[4, 6, 8, 10]] = 4                               # (an I of 2 bases compares q[9 - j] with q[11 - j]: the Ns meet each other at j = 1, 3, 5)
    def n_one(q, t):
        q[10 - 1 - 1] = 4
    C.append(runs_case("N_equals_N_continues_the_run", mid, {1: 6}, edit=n_both))
    C.append(runs_case("N_against_a_base_stops_the_run", mid, {1: 6}, edit=n_one))
    C.append(letters_case("not_eligible_indel_at_k_0", [(I, 2), (M, 9), (D, 1), (M, 5)], 1))
    C.append(letters_case("not_eligible_indel_at_k_n_minus_1", [(M, 9), (D, 1), (M, 5), (I, 2)], 1))
    C.append(letters_case("not_eligible_next_to_an_N_op", [(M, 9), (I, 2), (N, 30), (M, 5), (N, 20), (D, 2), (M, 5)], 1, score=SPLICE))
    C.append(letters_case("not_eligible_next_to_another_indel", [(M, 9), (I, 2), (D, 3), (M, 5)], 1))
    C.append(letters_case("prev_len_0_sets_to_shrink_without_a_shift", [(M, 4), (M, 0), (I, 2), (M, 5), (M, 3)], 4, seed=3))
    for r in (63, 64, 65):
        C.append(runs_case("I_compare_of_200_first_mismatch_at_%d" % r, [(M, 200), (I, 3), (M, 50)], {1: r}))
        C.append(runs_case("D_compare_of_200_first_mismatch_at_%d" % r, [(M, 200), (D, 2), (M, 50)], {1: r}))
    # ---- chains
    chain = [(M, 10), (I, 1), (M, 2), (I, 1), (M, 10)]
    C.append(search("chain_shift_of_k_minus_2_lets_k_pass_its_raw_M_unsaturated", [(M, 10), (I, 2), (M, 2), (I, 1), (M, 10)], lambda i, f: i["l"][3][0] > 2 and i["l"][3][0] < i["l"][3][1]))
    C.append(search("chain_shift_of_k_minus_2_lets_k_pass_its_raw_M_saturated", chain, lambda i, f: i["l"][3][0] > 2 and i["l"][3][0] == i["l"][3][1] and i["l"][1][0] < 10))
    chd = [(M, 10), (D, 2), (M, 2), (I, 1), (M, 10)]
    C.append(search("chain_D_then_I", chd, lambda i, f: i["l"][1][0] > 0 and i["l"][3][0] > 2))
    C.append(letters_case("chain_1M1I_x70_homopolymer_one_leading_70I", [(M, 1), (I, 1)] * 70 + [(M, 5)], 1))
    C.append(letters_case("chain_1M1D_x70_homopolymer_one_leading_70D", [(M, 1), (D, 1)] * 70 + [(M, 5)], 1))
    C.append(letters_case("chain_extension_of_150_bases", [(M, 150), (D, 2), (M, 1), (D, 2), (M, 20)], 1))
    C.append(letters_case("chain_extension_of_100_bases_I", [(M, 100), (I, 1), (M, 1), (I, 1), (M, 20)], 1))
    # ---- tile edges (64 ops per step)
    for at in (63, 64, 65):
        # an indel at index `at` between two Ms, over two letters: searched so that it shifts; everything in front alternates M / indel
        head = []
        while len(head) < at - 1:
            head.append((M, 3) if len(head) % 2 == 0 else ((I, D)[(len(head) // 2) % 2], 1))
        if head[-1][0] == M:                               # (the M in front of the indel is the one at at - 1)
            head[-1] = (N, 5)
        ops = head + [(M, 6), (I, 2), (M, 9)]
        assert len(ops) - 2 == at
        C.append(search("eligible_op_at_index_%d" % at, ops, lambda i, f, at=at: i["l"][at][0] > 0, score=SPLICE))
    for n in (64, 65, 128):
        ops = []
        while len(ops) < n:
            ops.append((M, 2) if len(ops) % 2 == 0 else ((I, D)[(len(ops) // 2) % 2], 1))
        C.append(search("cigar_of_exactly_%d_ops" % n, ops, lambda i, f: len(i["l"]) > 20 and events(i)["saturated"] and events(i)["past_raw"]))
    head = alternating(62, m_len=4)                        # 62 ops, the last one an indel ...
    head[-1] = (M, 4); head[-2] = (N, 7)                   # ... made ops 60 / 61 = N, M
    C.append(letters_case("pass_2_run_straddles_ops_62_to_66", head + [(I, 2), (D, 3), (I, 1), (D, 2), (I, 4), (M, 8), (D, 1), (M, 3)], 4, score=SPLICE))
    C.append(letters_case("squeeze_straddles_ops_62_to_66", head + [(M, 0), (I, 0), (M, 2), (D, 0), (M, 0), (M, 3), (I, 2), (M, 4)], 4, score=SPLICE))
    C.append(letters_case("merge_straddles_ops_62_to_66", head[:-1] + [(M, 1), (M, 2), (M, 3), (I, 0), (M, 4), (M, 5), (M, 6), (D, 2), (M, 4)], 4, score=SPLICE))
    C.append(letters_case("merge_segment_longer_than_a_tile", [(M, 5), (I, 1)] + [(M, 1)] * 150 + [(D, 0), (I, 3), (I, 2), (M, 4)], 4))
    C.append(letters_case("zero_length_ops_fill_a_whole_tile", [(M, 5), (I, 1)] + [(M, 0)] * 130 + [(I, 3), (M, 4)], 4))
    C.append(letters_case("pass_2_run_longer_than_a_tile", [(M, 5)] + [(I, 1), (D, 2)] * 75 + [(M, 4), (I, 1), (D, 1), (M, 2)], 4))
    C.append(letters_case("pass_2_run_ends_the_cigar_at_a_tile_edge", [(M, 5), (I, 1)] * 30 + [(M, 1), (I, 1), (D, 2), (I, 3)], 4))      # 64 ops
    # ---- pass 2
    C.append(letters_case("pass_2_I_D_I_merged", [(M, 5), (I, 5), (D, 6), (I, 7), (M, 5)], 4))
    C.append(letters_case("pass_2_I_D_left_alone", [(M, 5), (I, 5), (D, 6), (M, 5)], 4))
    C.append(letters_case("pass_2_D_I_D_I", [(M, 5), (D, 1), (I, 2), (D, 3), (I, 4), (M, 5)], 4))
    C.append(letters_case("pass_2_run_ends_the_cigar_start_at_n_minus_3", [(M, 5), (I, 5), (D, 6), (I, 7)], 4))
    C.append(letters_case("pass_2_start_at_n_minus_2_is_no_start", [(M, 5), (D, 1), (M, 4), (I, 5), (D, 6)], 4))
    C.append(letters_case("pass_2_run_followed_by_N", [(M, 5), (I, 5), (D, 6), (I, 7), (N, 40), (M, 5)], 4, score=SPLICE))
    C.append(letters_case("pass_2_5I_6D_2M_7I_pass_1_zeroes_the_2M", [(M, 5), (I, 5), (D, 6), (M, 2), (I, 7), (M, 5)], 1))
    C.append(letters_case("pass_2_5I_6D_2M_7I_the_2M_stays", [(M, 5), (I, 5), (D, 6), (M, 2), (I, 7), (M, 5)], 4, seed=1))
    C.append(letters_case("pass_2_5I_0M_6D_7I_trigger_after_the_zero", [(I, 5), (M, 0), (D, 6), (I, 7)], 4))
    C.append(letters_case("pass_2_N_M_at_the_trigger_test", [(M, 5), (N, 30), (M, 5), (I, 1), (M, 3)], 4, score=SPLICE))
    C.append(letters_case("pass_2_I_I_D_I_starts_at_the_second_I", [(M, 5), (I, 1), (I, 2), (D, 3), (I, 4), (M, 5)], 4))
    C.append(letters_case("pass_2_only_one_kind_of_gap_has_length", [(M, 5), (I, 1), (D, 0), (I, 2), (M, 5)], 4))
    # ---- shrink
    C.append(letters_case("shrink_5M_3M_2I_4M_without_a_zero_stays_unmerged", [(M, 5), (M, 3), (I, 2), (M, 4)], 4, seed=2))
    C.append(letters_case("shrink_5M_3M_2I_4M_with_a_zero_elsewhere_merges", [(M, 5), (M, 3), (I, 2), (M, 4), (D, 0), (M, 2)], 4, seed=2))
    # ---- a zero-length M that has grown by the time the loop reaches it does not ask for the squeeze: the equal neighbours elsewhere stay unmerged
    C.append(runs_case("zero_M_behind_a_partly_shifting_I_is_no_zero_any_more", [(M, 10), (I, 2), (M, 0), (M, 5), (M, 3)], {1: 1}))
    C.append(runs_case("zero_M_behind_a_partly_shifting_D_is_no_zero_any_more", [(M, 10), (D, 3), (M, 0), (I, 1), (M, 2), (M, 2)], {1: 4, 3: 0}))
    C.append(runs_case("zero_M_behind_an_I_that_does_not_shift_is_a_zero", [(M, 10), (I, 2), (M, 0), (M, 5), (M, 3)], {1: 0}))
    edge = alternating(62, m_len=4) + [(M, 9), (I, 1), (M, 0), (M, 2), (M, 2), (D, 1), (M, 6)]          # the I at op 63, the zero M at op 64: the next tile's first lane
    C.append(runs_case("zero_M_behind_a_partly_shifting_I_across_the_tile_edge", edge, dict([(k, 0) for k in range(1, 62, 2)] + [(63, 3), (67, 0)])))
    # ---- leading op
    C.append(letters_case("lead_2I_3D_5M_only_one_op_removed", [(I, 2), (D, 3), (M, 5)], 4))
    C.append(letters_case("lead_D_gives_tshift", [(D, 4), (M, 7), (I, 1), (M, 3)], 4))
    C.append(letters_case("lead_indel_appears_only_after_the_squeeze", [(M, 0), (I, 3), (M, 6), (D, 1), (M, 3)], 4))
    C.append(letters_case("lead_indel_made_by_pass_1", [(M, 3), (I, 2), (M, 8)], 1))
    C.append(letters_case("lead_merged_indels_are_one_op", [(I, 2), (M, 0), (I, 3), (M, 6)], 4))
    # ---- other
    C.append(letters_case("op_codes_4_to_9_with_a_length_are_inert", [(M, 4), (4, 3), (5, 2), (M, 3), (I, 1), (6, 1), (7, 7), (7, 2), (M, 0), (8, 1), (9, 4), (M, 3), (D, 1), (M, 2)], 2))
    ops5000 = []
    rng = np.random.default_rng(5000)
    while len(ops5000) < 4999:
        ops5000.append((M, int(rng.choice([1, 1, 2, 3, 5, 12]))) if len(ops5000) % 2 == 0 else (int(rng.choice([I, D])), int(rng.integers(1, 4))))
    C.append(letters_case("one_job_of_5000_ops", ops5000 + [(M, 7)], 2, seed=5))
    return C


def batch70():
    """70 jobs of mixed sizes in one call (ONT score), n_cigar 0 and 1 among them"""
    rng = np.random.default_rng(70)
    C = []
    for k in range(70):
        C.append(random_case(rng, k, "batch70_%d" % k, n_ops=(0, 1, 2, 3, 64, 65, 129)[k % 10] if k % 10 < 7 else None))
    return C


# ---- random cases: 2 - 200 ops with M on even slots; M lengths from LENS, indels of 1 - 4 bases, about 8 % N ops and 8 % I D I / D I D triples; the alphabet has
# 1, 2, 2 or 4 letters by case index, M mismatch is 3 %, every fifth case loses its first M. A run of this generator (seed 91, the restatement alone) gave, of 300
# cases: a shift past the raw preceding M 172, a shift of more than 64 bases 71, a pass-2 rewrite 270, a removed leading op 124, a saturated op 270. The tests assert the
# floors of FLOORS, about half of those counts.
LENS = (1, 1, 2, 3, 5, 12, 33, 70, 130)
FLOORS = {"past_raw": 90, "over_64": 35, "rewrite": 130, "lead": 55, "saturated": 135}


def random_case(rng, idx, name, n_ops=None, score=ONT, zero_rate=0.0):
    letters = (1, 2, 2, 4)[idx % 4]
    n = int(rng.integers(2, 201)) if n_ops is None else n_ops
    ops = []
    while len(ops) < n:
        if len(ops) % 2 == 0:
            ops.append((M, int(rng.choice(LENS))))
        else:
            r = rng.random()
            if r < 0.08:
                ops.append((N, int(rng.integers(1, 50))))
            elif r < 0.16 and len(ops) + 3 <= n:
                a = int(rng.choice([I, D]))
                ops += [(a, int(rng.integers(1, 5))), (3 - a, int(rng.integers(1, 5))), (a, int(rng.integers(1, 5)))]
            else:
                ops.append((int(rng.choice([I, D])), int(rng.integers(1, 5))))
    ops = ops[:n]
    if idx % 5 == 4 and len(ops) > 2:
        ops = ops[1:]
    if zero_rate:                                          # zero-length M, I and D ops (never N: the reference indexes s[op] out of bounds there)
        ops = [(o, 0) if o != N and rng.random() < zero_rate else (o, l) for o, l in ops]
        if not any(l for o, l in ops):
            ops[0] = (ops[0][0], 1)
    ql = sum(l for o, l in ops if o in (M, I)); tl = sum(l for o, l in ops if o in (M, D, N))
    t = rng.integers(0, letters, tl).astype(np.uint8)
    q = rng.integers(0, letters, ql).astype(np.uint8)
    qi = ti = 0
    for o, l in ops:                                       # the query copies the target along M, 3 % mismatches
        if o == M:
            seg = t[ti:ti + l].copy()
            flip = rng.random(l) < 0.03
            seg[flip] = (seg[flip] + 1) % 4
            q[qi:qi + l] = seg; qi += l; ti += l
        elif o == I:
            qi += l
        else:
            ti += l
    return (name, enc(ops), padded(q), padded(t), score)


def random_cases(n=300, seed=91):
    rng = np.random.default_rng(seed)
    return [random_case(rng, i, "random_%d" % i, score=(ONT, ASM20, SPLICE)[i % 3]) for i in range(n)]


def random_zero_cases(n=100, seed=92):
    """the same generator with 12 % of the M / I / D ops of length 0 (2 - 80 ops): the squeeze, the merge and zero-length ops behind shifting indels"""
    rng = np.random.default_rng(seed)
    return [random_case(rng, i, "random_zero_%d" % i, n_ops=int(rng.integers(2, 81)), score=(ONT, ASM20, SPLICE)[i % 3], zero_rate=0.12) for i in range(n)]


# ---- position form: (name, cigar, read, q_pos, contig, t_pos, score), the layout of extracases.make_pos_cases ------------------------------------------------
LEAD = 37                                # bases in front of the read in the resident buffer of the tests


def make_pos_cases():
    rng = np.random.default_rng(78)
    L = 1000
    read = rng.integers(0, 2, L).astype(np.uint8)          # two letters: shifts everywhere
    read[[5, 333, 334, 700, 999]] = 4
    # homopolymer stretches with one other base each: an I compare that walks down such a stretch stops there. In the resident buffer (behind LEAD bases) the four
    # breaks are the last base of a 32-base word of the packed codes, the first base of one, the last base of a 64-base word of the ambiguity bitmap, the first of one.
    BREAKS = (250, 379, 474, 603)
    assert [(LEAD + b) % 64 for b in BREAKS] == [31, 32, 63, 0]
    for b in BREAKS:
        read[b - 15:b + 75] = 0
        read[b] = 1
    P = []

    def pos_case(name, ops, q_pos, t_pos, contig_len, score=ONT):
        ql = sum(l for o, l in ops if o in (M, I)); tl = sum(l for o, l in ops if o in (M, D, N))
        q = X.two_strand(read, q_pos, ql)
        contig = rng.integers(0, 2, contig_len).astype(np.uint8)
        qi, ti = 0, t_pos
        for o, l in ops:
            if o == M:
                seg = q[qi:qi + l].copy(); seg[seg > 3] = 0
                flip = rng.random(l) < 0.04; seg[flip] = (seg[flip] + 1) % 4
                contig[ti:ti + l] = seg; qi += l; ti += l
            elif o == I:
                qi += l
            else:
                ti += l
        assert t_pos + tl <= contig_len
        P.append((name, enc(ops), read, q_pos, contig, t_pos, score))

    ops = [(M, 40), (I, 2), (M, 3), (D, 1), (M, 50), (I, 1), (D, 2), (I, 1), (M, 30), (D, 3), (M, 2), (D, 1), (M, 60), (I, 3), (M, 25)]
    pos_case("pos_forward_strand", ops, 20, 40, 600)
    pos_case("pos_reverse_strand", ops, L + 100, 11, 600)
    pos_case("pos_q_3_bases_before_strand_1", ops, L - 3, 5, 600)
    pos_case("pos_q_3_bases_before_strand_0_is_padding", ops, -3, 5, 600)
    pos_case("pos_leading_I_on_the_reverse_strand", [(I, 4), (M, 30), (D, 2), (M, 20)], L + 50, 9, 300)
    pos_case("pos_leading_D", [(D, 5), (M, 30), (I, 2), (M, 20)], 60, 9, 300)
    for r in range(8):
        pos_case("pos_t_pos_mod_8_is_%d" % r, ops, 33 + r, 64 + r, 600, score=ASM20)
    for b in BREAKS:                                       # the I sits 70 bases above the break: 69 bases match, the 70th is the break
        pos_case("pos_I_compare_stops_at_read_base_%d" % b, [(M, 85), (I, 2), (M, 30)], b - 15, 3, 200)
    return P


def pos_operands(p):
    """the operands of a position case spelled out as bytes, padded: what the specification reads"""
    name, cig, read, q_pos, contig, t_pos, score = p
    ql = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 1)); tl = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 2, 3))
    return padded(X.two_strand(read, q_pos, ql)), padded(contig[t_pos:t_pos + tl])


def dump(path):
    """every byte-form case in the layout tests/simt_emu/emu_fix_main.cpp reads (the stand-alone driver for sanitizer builds)"""
    cases = make_cases() + batch70() + random_cases() + random_zero_cases()
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes())
        for name, cig, q, t, score in cases:
            f.write(np.array(list(score) + [len(cig), len(q), len(t)], np.int32).tobytes())
            f.write(np.ascontiguousarray(cig, np.uint32).tobytes()); f.write(np.ascontiguousarray(q, np.uint8).tobytes()); f.write(np.ascontiguousarray(t, np.uint8).tobytes())
    return len(cases)


if __name__ == "__main__":
    import sys
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        print(dump(sys.argv[2]), "cases ->", sys.argv[2])
