"""The named cases of ksw_ll_i16 (src/ksw2_ll_sse.c:80-147) shared by the emulator tests (test_ll_emu.py) and the device tests (test_ll_gpu.py), and a pure-Python
restatement of the striped machine IN POSITION TERMS — the closed form the kernel of csrc/ll_kernel.h computes, written with whole-row numpy scans instead of lanes.

The machine (csrc/ksw_ll.h is the specification): the query is padded to n = 8 * slen positions (pads score 0, and H travels into them along the diagonal); H saturates
at 32767, everything clamps at 0; the F of the main loop never crosses one of the 8 segments [l * slen, (l + 1) * slen) and the next row's E is opened from that
main-loop H; the lazy-F rounds add the F that crosses segments to H only; the score is the largest main-loop H, te the LAST row that holds it, qe the position of
that row whose striped slot (p % slen) * 8 + p // slen is largest. A case is a dict: name, q, t (0..4 codes), a, b, ambi (ksw_gen_simple_mat), gapo, gape."""
import numpy as np

REG_MAX_DEFAULT = 64         # csrc/wm_ll.hip: padded queries of at most this many positions run in the register class
SCORINGS = [(2, 4, 4, 2), (1, 4, 6, 1), (1, 1, 1, 1), (2, 4, 120, 7)]      # (a, b, q, e); the last one has gapo + gape = 127
LENGTHS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513)  # 64 | 65 and (under a boundary of 32) 32 | 33 are the two sides of the class boundary


def simple_mat(a, b, ambi):
    """ksw_gen_simple_mat (src/align.c:9-22), m = 5"""
    a, b, ambi = abs(a), -abs(b), -abs(ambi)
    return np.array([ambi if (i == 4 or j == 4) else (a if i == j else b) for i in range(5) for j in range(5)], np.int8)


def restated(q, t, mat, gapo, gape, e_from_corrected=False):
    """(score, qe, te, positions of row te that reach the score, rows that reach the score). e_from_corrected: the machine that is NOT the reference's — E opened
    from the corrected H — for the search of the cases that tell the two apart."""
    q = np.asarray(q, np.int64); t = np.asarray(t, np.int64)
    qlen, tlen = len(q), len(t)
    slen = (qlen + 7) // 8
    n = 8 * slen
    oe, ext = gapo + gape, gape
    m = np.asarray(mat, np.int64).reshape(5, 5)
    S = np.zeros((5, n), np.int64)
    S[:, :qlen] = m[:, q]                                   # S[target code][position]; pads 0
    pos = np.arange(n, dtype=np.int64)
    in_seg = pos % slen if slen else pos

    def f_in(D, p_local):
        """max(0, max over p' < p of D[p'] - oe - (p - p' - 1) * ext) along the last axis: a running maximum of D[p'] + p' * ext"""
        G = D + p_local * ext
        run = np.maximum.accumulate(G, axis=-1)
        M = np.full_like(G, -(1 << 40))
        M[..., 1:] = run[..., :-1]
        return np.maximum(M - oe - (p_local - 1) * ext, 0)

    H = np.zeros(n, np.int64); E = np.zeros(n, np.int64)
    gmax, te, rows, best_row = 0, -1, [], np.zeros(n, np.int64)
    for i in range(tlen):
        Hd = np.concatenate([[0], H[:-1]])
        D = np.maximum(np.minimum(Hd + S[t[i]], 32767), E)
        Fseg = f_in(D.reshape(8, slen), in_seg.reshape(8, slen)).reshape(n)
        Ffull = f_in(D, pos)
        Hmain = np.maximum(D, Fseg)
        H = np.maximum(D, Ffull)
        E = np.maximum(np.maximum(E - ext, (H if e_from_corrected else Hmain) - oe), 0)
        rmax = int(Hmain.max())
        if rmax >= gmax:
            rows = rows + [i] if rmax == gmax else [i]
            gmax, te, best_row = rmax, i, H
    reach = [int(p) for p in np.nonzero(best_row == gmax)[0]]
    qe = max(reach, key=lambda p: (p % slen, p // slen)) if te >= 0 else -1
    return gmax, qe, te, reach, rows


def _rng_seq(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _related(rng, q, tl, sub=0.08, indel=0.03):
    """a target of tl bases that shares a mutated copy of q (substitutions, short indels) somewhere inside random flanks"""
    out = []
    for c in q:
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out.append(int(rng.integers(0, 4)))
        out.append(int(rng.integers(0, 4)) if rng.random() < sub else int(c))
    core = np.array(out[:tl], np.uint8)
    lead = int(rng.integers(0, tl - len(core) + 1))
    return np.concatenate([_rng_seq(rng, lead), core, _rng_seq(rng, tl - len(core) - lead)]).astype(np.uint8)


def case(name, q, t, a=2, b=4, ambi=1, gapo=4, gape=2):
    return dict(name=name, q=np.ascontiguousarray(q, np.uint8), t=np.ascontiguousarray(t, np.uint8), a=a, b=b, ambi=ambi, gapo=gapo, gape=gape)


# E opened from the main-loop H: inputs where opening it from the corrected H would give another triple. search_e_cases() below went over 20000 random small jobs
# (queries of 9..40 bases, match 1..40, mismatch down to -60, gap open 1..30, extension 1..4) and found NONE, so the list is empty and no case pins the rule. Why that
# is plausible: a corrected H that exceeds the main-loop H is the end of a gap that crossed a segment boundary, so an E opened from it is a gap right behind a gap;
# the same two gaps taken in the other order reach the same cell through the E of the gap's first column and the F of the next row, so H never differs — only E and
# the main-loop H of such a cell do, and a cell that two gaps lead to is never the best one of a local alignment. The random jobs of test_ll_emu.py (2000, up to
# 600 x 600) compare the kernel, which opens E from the main-loop H, with the specification all the same.
E_CASES = [
]


def search_e_cases(n_jobs=20000, want=4, seed=5):
    """the search that filled E_CASES: random jobs with a cheap gap and a dear mismatch whose triple changes when E is opened from the corrected H"""
    rng = np.random.default_rng(seed)
    found = []
    for _ in range(n_jobs):
        ql, tl = int(rng.integers(9, 41)), int(rng.integers(4, 41))
        a, b, go, ge = int(rng.integers(1, 41)), int(rng.integers(1, 61)), int(rng.integers(1, 31)), int(rng.integers(1, 5))
        q = _rng_seq(rng, ql)
        t = _related(rng, q, tl, 0.15, 0.1) if tl >= 4 else _rng_seq(rng, tl)
        m = simple_mat(a, b, 1)
        if restated(q, t, m, go, ge)[:3] != restated(q, t, m, go, ge, True)[:3]:
            found.append(("".join("ACGT"[c] for c in q), "".join("ACGT"[c] for c in t), a, b, go, ge))
            if len(found) >= want:
                break
    return found


def _codes(s):
    return np.array(["ACGTN".index(c) for c in s], np.uint8)


def make_cases():
    rng = np.random.default_rng(20261021)
    cs = []
    # ---- lengths: every query length against a related target of 64 rows; the short and the odd targets
    for ql in LENGTHS:
        q = _rng_seq(rng, ql)
        cs.append(case("len_q%d_t64" % ql, q, _related(rng, q, 64) if ql <= 64 else _related(rng, q[:60], 64)))
    for ql, tl in [(1, 1), (9, 1), (64, 1), (65, 1), (64, 63), (64, 65), (65, 63), (65, 65), (513, 130), (33, 200)]:
        q = _rng_seq(rng, ql)
        cs.append(case("len_q%d_t%d" % (ql, tl), q, _related(rng, q[:tl], tl) if tl > 1 else q[:1]))
    # ---- the best cell on a pad slot: the target goes on behind the query's copy, the diagonal carries the score through the 7 pads of a length = 1 (mod 8)
    for ql in (9, 17, 65, 513):
        q = _rng_seq(rng, ql)
        cs.append(case("pad_slot_q%d" % ql, q, np.concatenate([_rng_seq(rng, 5), q, _rng_seq(rng, 12)])))
    # ---- two positions of row te reach the score; the striped order prefers position 10 (slot 1 * 8 + 3) to position 21 (slot 0 * 8 + 7): slen = 3
    u = _codes("ACGTTGCAAGC")
    cs.append(case("tie_qe_tandem", np.concatenate([u, u]), u))
    # ---- several rows reach the score: te is the last
    cs.append(case("tie_te_periodic", u, np.concatenate([u, u, u])))
    # ---- nothing scores: all-A against all-C
    cs.append(case("all_zero_q20_t30", np.zeros(20, np.uint8), np.ones(30, np.uint8)))
    cs.append(case("all_zero_q64_t1", np.zeros(64, np.uint8), np.ones(1, np.uint8)))
    # ---- saturation: 900 x 40 > 32767; 762 x 43 = 32767 - 1 exactly
    q = _rng_seq(rng, 900)
    cs.append(case("saturated_900_a40", q, q, a=40, b=60, gapo=30, gape=5))
    q = _rng_seq(rng, 762)
    cs.append(case("one_below_saturation_762_a43", q, q, a=43, b=60, gapo=30, gape=5))
    # ---- E opened from the main-loop H
    for k, (qs, ts, a, b, go, ge) in enumerate(E_CASES):
        cs.append(case("e_from_hmain_%d" % k, _codes(qs), _codes(ts), a=a, b=b, gapo=go, gape=ge))
    # ---- ambiguous bases in both operands under the three ambiguity scores
    for ambi in (0, 1, 3):
        q = _rng_seq(rng, 70); t = _related(rng, q, 90)
        q[[3, 30, 31, 69]] = 4; t[[0, 40, 41, 42, 89]] = 4
        cs.append(case("ambiguous_sc%d" % ambi, q, t, ambi=ambi))
    # ---- the scoring sets, in either class
    for a, b, go, ge in SCORINGS:
        for ql, tl in ((40, 50), (150, 140)):
            q = _rng_seq(rng, ql)
            cs.append(case("scoring_%d_%d_%d_%d_q%d" % (a, b, go, ge, ql), q, _related(rng, q, tl, 0.1, 0.06), a=a, b=b, gapo=go, gape=ge))
    return cs


def random_jobs(n, max_len, seed):
    """random jobs over SCORINGS: related and unrelated operands, a few ambiguous bases"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        ql, tl = int(rng.integers(1, max_len + 1)), int(rng.integers(1, max_len + 1))
        a, b, go, ge = SCORINGS[int(rng.integers(0, len(SCORINGS)))]
        q = _rng_seq(rng, ql)
        t = _related(rng, q[:tl], tl, 0.1, 0.05) if rng.random() < 0.75 else _rng_seq(rng, tl)
        if rng.random() < 0.2:
            q[rng.integers(0, ql, 2)] = 4; t[rng.integers(0, tl, 2)] = 4
        out.append(case("random_%d" % k, q, t, a=a, b=b, ambi=int(rng.integers(0, 4)), gapo=go, gape=ge))
    return out


def pack(cases, step):
    """the byte form of wm_ll_job_t: operands back to back; step = -1 stores every operand reversed, so that reading it backwards gives the same job"""
    q_off, t_off, at, parts = [], [], 0, []
    for c in cases:
        q_off.append(at); at += len(c["q"]); t_off.append(at); at += len(c["t"])
        parts += [c["q"][::step], c["t"][::step]]
    return (np.array(q_off, np.int64), np.array(t_off, np.int64), np.array([len(c["q"]) for c in cases], np.int32), np.array([len(c["t"]) for c in cases], np.int32),
            np.full(len(cases), step, np.int32), np.ascontiguousarray(np.concatenate(parts), np.uint8))


def pos_layout(cases, step, seed=3):
    """the position form: every query sits in a read of its own (forward strand for even cases, reverse strand for odd ones), every target in one contig. Returns the
    reads' codes, the contig's codes and per job (qwin_off, qwin_len, q_pos, t_pos) — element 0 of either operand, as wm_ll_pos_t wants it."""
    rng = np.random.default_rng(seed)
    reads, ref, jobs = [], [], []
    r_at = t_at = 0
    for k, c in enumerate(cases):
        q, t = c["q"], c["t"]
        lead, tail = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        fwd = k % 2 == 0
        body = q if fwd else np.where(q[::-1] < 4, 3 - q[::-1], 4).astype(np.uint8)      # the read whose reverse strand holds q
        read = np.concatenate([_rng_seq(rng, lead), body, _rng_seq(rng, tail)]).astype(np.uint8)
        L = len(read)
        first = lead if fwd else L + tail                                                # two-strand index of q[0]
        reads.append(read)
        tl = int(rng.integers(0, 5))
        ref += [_rng_seq(rng, tl), t]
        t_first = t_at + tl
        jobs.append((r_at, L, first if step > 0 else first + len(q) - 1, t_first if step > 0 else t_first + len(t) - 1))
        r_at += L; t_at += tl + len(t)
    return np.concatenate(reads).astype(np.uint8), np.concatenate(ref).astype(np.uint8), jobs
