"""Sequences (0..4 codes) and minimizer lists for the -T tests (tests/test_sdust_emu.py on the wavefront emulator, tests/test_sdust_gpu.py on the device):
one list, so that both check the same ground. Everything is seeded."""
import numpy as np

THRESHOLDS = (20, 10, 30, 4)


def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def unit_run(rng, unit, n, sub=0.0):
    s = np.resize(np.array(unit, np.uint8), n).copy()
    if sub > 0 and n > 0:
        hit = rng.random(n) < sub
        s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    return s


def p_list_stress(rng):
    """random, a dinucleotide run, random, one N, a homopolymer, random: after the N the window start stands still while the window still holds the
    triplets from before it, and the list of perfect intervals grows into the thousands (DESIGN.md "-T")"""
    return np.concatenate([rnd(rng, 300), unit_run(rng, (0, 3), 200), rnd(rng, 100), np.array([4], np.uint8), unit_run(rng, (0,), 80), rnd(rng, 200)])


def named_cases():
    rng = np.random.default_rng(20)
    out = [("p_list_stress", p_list_stress(rng))]
    for n in range(6):
        out.append(("len%d" % n, unit_run(rng, (0,), n)))
        out.append(("len%d_rnd" % n, rnd(rng, n)))
    out.append(("only_n", np.full(40, 4, np.uint8)))
    units = {"homo": (2,), "di": (0, 3), "tri": (1, 0, 2)}
    for kind, unit in units.items():
        for n in (10, 23, 64, 65, 130, 300):
            for sub in (0.0, 0.03, 0.10):
                run = unit_run(rng, unit, n, sub)
                out.append(("%s%d_s%d" % (kind, n, int(sub * 100)), np.concatenate([rnd(rng, 70), run, rnd(rng, 90)])))
    for n_n in (1, 2, 3):                                   # a run interrupted by ambiguous bases, at close and at far spacing
        for kind, unit in units.items():
            run = unit_run(rng, unit, 200, 0.02)
            at = np.sort(rng.choice(np.arange(5, 195), n_n, replace=False))
            run[at] = 4
            out.append(("%s_n%d" % (kind, n_n), np.concatenate([rnd(rng, 50), run, rnd(rng, 120)])))
        tight = unit_run(rng, (3,), 90)
        tight[40:40 + n_n] = 4
        out.append(("homo_tight_n%d" % n_n, np.concatenate([rnd(rng, 30), tight, unit_run(rng, (0, 1), 70), rnd(rng, 40)])))
    out.append(("run_at_end", np.concatenate([rnd(rng, 120), unit_run(rng, (0, 2), 75)])))
    out.append(("run_at_start", np.concatenate([unit_run(rng, (1,), 40), rnd(rng, 100)])))
    out.append(("n_then_end", np.concatenate([rnd(rng, 80), unit_run(rng, (0,), 50), np.array([4], np.uint8)])))
    out.append(("all_run", unit_run(rng, (0, 1, 2), 400, 0.01)))
    out.append(("random3k", rnd(rng, 3000)))
    return out


def mixture(seed):
    """a random mixture of random stretches, unit runs with substitutions, and ambiguous bases; at most 1 500 bases"""
    rng = np.random.default_rng(1000 + seed)
    parts, total = [], 0
    want = int(rng.integers(1, 1501))
    while total < want:
        kind = int(rng.integers(0, 6))
        n = int(min(want - total, rng.integers(1, 260)))
        if kind <= 1:
            p = rnd(rng, n)
        elif kind <= 4:
            p = unit_run(rng, rnd(rng, int(rng.integers(1, 5))), n, float(rng.choice([0.0, 0.02, 0.05, 0.1])))
        else:
            p = np.full(min(n, int(rng.integers(1, 4))), 4, np.uint8)
        if rng.random() < 0.15 and len(p) > 2:
            p[int(rng.integers(0, len(p)))] = 4
        parts.append(p)
        total += len(p)
    return np.concatenate(parts)


N_MIXTURES = 300


def long_case():
    """70 000 random bases with three implanted runs: long enough for the chunked sketch"""
    rng = np.random.default_rng(70)
    s = rnd(rng, 70000)
    s[5000:5400] = unit_run(rng, (0, 3), 400, 0.02)
    s[33000:33120] = unit_run(rng, (2,), 120)
    s[33060] = 4
    s[65500:66300] = unit_run(rng, (1, 0, 0), 800, 0.05)
    return s


def minimizers(rng, length, n, hpc=False, k=15):
    """a minimizer list as mm_sketch leaves it: ascending end positions; with hpc the spans vary (15 .. 120), so the starts are not monotone"""
    if length < 130 or n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    pos = np.sort(rng.choice(np.arange(125, length), min(n, length - 125), replace=False)).astype(np.uint64)
    span = rng.integers(k, 121, len(pos)).astype(np.uint64) if hpc else np.full(len(pos), k, np.uint64)
    x = rng.integers(0, 1 << 30, len(pos)).astype(np.uint64) << np.uint64(8) | span
    y = pos << np.uint64(1) | rng.integers(0, 2, len(pos)).astype(np.uint64)
    return x, y


def restated_filter(mx, my, iv):
    """mm_dust_minier's squeeze, src/map.c:51-63, restated: iv = [(start, finish)], returns the kept indices"""
    keep, u = [], 0
    for j in range(len(mx)):
        qpos, span = (int(my[j]) & 0xffffffff) >> 1, int(mx[j]) & 0xff
        s = qpos - (span - 1)
        e = s + span
        while u < len(iv) and iv[u][1] <= s:
            u += 1
        covered, v = 0, u
        while v < len(iv) and iv[v][0] < e:
            covered += min(e, iv[v][1]) - max(s, iv[v][0])
            v += 1
        if covered <= span >> 1:
            keep.append(j)
    return keep


def e2e_inputs(tmp):
    """a 300 kb reference with implanted microsatellites and ~60 reads of 3 .. 12 kb drawn over them: -> (reference FASTA, reads FASTA)"""
    import os
    from winnowmap_amd import synth
    rng = np.random.default_rng(77)
    ref = rnd(rng, 300000)
    units = [(0,), (3,), (0, 1), (0, 3), (1, 0, 2), (2, 2, 1), (0, 0, 0, 3), (0, 2, 1, 3, 3)]
    sites = np.arange(2000, 298000, 4100)
    for p in sites:
        n = int(rng.integers(60, 700))
        ref[p:p + n] = unit_run(rng, units[int(rng.integers(0, len(units)))], n, float(rng.choice([0.0, 0.02, 0.05])))
    reads = []
    for i in range(60):
        n = int(rng.integers(3000, 12001))
        st = int(rng.integers(0, len(ref) - n))
        r = synth.mutate_codes(ref[st:st + n].copy(), rng, 0.03, 0.02, 0.02)
        if i % 2:
            r = synth.revcomp_codes(r)
        if i % 7 == 0:
            r[int(rng.integers(0, len(r)))] = 4
        reads.append(r)
    fa, rq = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
    synth.write_fasta(fa, [ref], prefix="chr")
    with open(rq, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n" % i + synth.codes_to_ascii(r) + b"\n")
    return fa, rq
