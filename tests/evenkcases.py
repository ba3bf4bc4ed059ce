"""Shared inputs of the even-k tests (test_evenk_*.py): sequences on which the palindrome rule of mm_sketch (src/sketch.c:166 — a k-mer that equals its
reverse complement skips the WHOLE step) fires often, also right behind an ambiguous base, and a small Python restatement of that rule which every
fixture uses to assert that its inputs do exercise it. Pure numpy; no reference code involved."""
import numpy as np
from winnowmap_amd import synth

PAIRS = ((50, 14), (10, 16), (5, 6), (50, 28), (3, 4), (5, 2))          # (w, k)
_UNITS = ((0, 3), (3, 0), (1, 2), (2, 1))                               # AT TA CG GC


def _palindrome(rng, half):
    a = synth.random_codes(half, rng)
    return np.concatenate([a, synth.revcomp_codes(a)])


def _satellite(rng, n):
    return np.tile(np.array(_UNITS[int(rng.integers(0, 4))], np.uint8), n // 2 + 1)[:n]


def plant_microsatellites(contigs, rng, n_arrays, lo=30, hi=400):
    """(AT)n / (CG)n arrays written into the contigs (in place)"""
    for _ in range(n_arrays):
        c = contigs[int(rng.integers(0, len(contigs)))]
        n = int(rng.integers(lo, hi))
        p = int(rng.integers(0, len(c) - n))
        c[p:p + n] = _satellite(rng, n)
    return contigs


def make_cases(w, k, seed=1):
    """list of uint8 code arrays (0..3, 4 = ambiguous)"""
    rng = np.random.default_rng(seed * 1000 + 31 * k + w)
    seqs = []
    for it in range(40):                       # random sequences with planted a + revcomp(a) blocks, microsatellite runs and short N runs
        s = synth.random_codes(int(rng.integers(200, 3001)), rng)
        for _ in range(int(rng.integers(1, 5))):
            b = _palindrome(rng, int(rng.integers(max(1, k // 2), 3 * k + 1)))
            if rng.random() < 0.5:             # ... half of them with an N somewhere inside
                b = np.insert(b, int(rng.integers(1, len(b))), 4)
            p = int(rng.integers(0, len(s) - len(b)))
            s[p:p + len(b)] = b
        for _ in range(int(rng.integers(1, 4))):
            r = _satellite(rng, int(rng.integers(k, 201)))
            if rng.random() < 0.5:
                r[int(rng.integers(0, len(r)))] = 4
            p = int(rng.integers(0, len(s) - len(r)))
            s[p:p + len(r)] = r
        for _ in range(int(rng.integers(0, 5))):
            p = int(rng.integers(0, len(s) - 3))
            s[p:p + int(rng.integers(1, 4))] = 4
        seqs.append(s)
    pal = _palindrome(rng, 2 * k)
    # one palindrome split by a single N; an N run longer than w + k in front of a palindrome (and of a microsatellite)
    seqs.append(np.concatenate([synth.random_codes(100, rng), pal[:2 * k], [4], pal[2 * k:], synth.random_codes(100, rng)]).astype(np.uint8))
    seqs.append(np.concatenate([synth.random_codes(150, rng), np.full(w + k + 7, 4), pal, synth.random_codes(3 * (w + k), rng), np.full(w + k + 1, 4),
                                _satellite(rng, 90), synth.random_codes(200, rng)]).astype(np.uint8))
    src = np.concatenate([synth.random_codes(40, rng), pal, _satellite(rng, 60), synth.random_codes(40, rng)]).astype(np.uint8)
    for n in (1, k - 1, k, k + 1, w + k - 1, w + k, 63, 64, 65, 128, 129):
        st = int(rng.integers(0, max(1, len(src) - n)))
        seqs.append(src[st:st + n].copy())
        seqs.append(_satellite(rng, n))        # (the same lengths, every k-mer a palindrome)
    seqs.append(np.full(300, 4, np.uint8))                              # all N
    seqs.append(np.tile(np.array([0, 3], np.uint8), 200))               # all (AT): every step past the first k - 1 bases is skipped
    return [np.ascontiguousarray(s, np.uint8) for s in seqs]


def skip_stats(seq, k, hpc=False):
    """The skip rule restated (src/sketch.c:146-176): (steps, steps skipped, steps skipped while l < k - 1). The two k-mer registers shift on every
    unambiguous base (under hpc: run) and are not reset by an ambiguous one; a skipped step leaves l alone."""
    mask, sh = (1 << 2 * k) - 1, 2 * (k - 1)
    fw = rc = l = steps = skipped = low = 0
    i, n = 0, len(seq)
    while i < n:
        c = int(seq[i])
        steps += 1
        if c < 4:
            if hpc:
                while i + 1 < n and seq[i + 1] == c:
                    i += 1
            fw = (fw << 2 | c) & mask
            rc = rc >> 2 | (3 ^ c) << sh
            if fw == rc:
                skipped += 1
                low += l < k - 1
            else:
                l += 1
        else:
            l = 0
        i += 1
    return steps, skipped, low


def assert_exercises_rule(seqs, k, hpc=False):
    """the condition on the inputs: at least 0.5 % of all steps are skipped, at least 10 of them where l < k - 1"""
    st = np.array([skip_stats(s, k, hpc) for s in seqs]).sum(axis=0)
    assert st[1] >= 0.005 * st[0] and st[2] >= 10, (k, hpc, [int(x) for x in st])
    return [int(x) for x in st]


def reference(seed, n_contigs=2, contig_len=100000, n_arrays=60):
    """a reference with repeat families and planted (AT)n / (CG)n arrays"""
    ref = synth.make_reference(n_contigs, contig_len, seed, repeat_frac=0.1)
    return plant_microsatellites(ref, np.random.default_rng(seed + 77), n_arrays)
