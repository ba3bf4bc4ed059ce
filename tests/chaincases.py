"""Deterministic chain cases shared by the oracle-vs-reference, emulator and GPU tests of the chain fill and extraction (seedchain_kernel.h,
window_kernel.h, the class routing of wm_chain_batch and wm_window_batch). A case is a dict: name, group, x, y (sorted anchors, uint64) and par (the ten
chain parameters of wm_mapopt_t that reach a window job). Nothing here calls the oracle: the tests do, and tests/test_chain_edges_emu.py asserts that
every edge value below changes the oracle's output against its neighbouring value on at least one case (NEIGHBOURS)."""
import numpy as np

DEFAULT = dict(max_dist_x=5000, min_dist_x=1000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, min_cnt=3, min_sc=40, gap_scale=1.0, is_cdna=0)
STAGE2 = dict(DEFAULT, max_dist_x=16000, max_dist_y=16000, bw=2000)          # the re-chaining parameters (src/map.c:818-833): the dense sets use them
OPEN = dict(min_cnt=1, min_sc=0)                                           # the open observer: (almost) every anchor comes back, with its chain's score
FILL_KEYS = ("max_dist_x", "min_dist_x", "max_dist_y", "bw", "max_skip", "max_iter", "gap_scale", "is_cdna")
SPAN = np.uint64(15 << 32)


def par(base=DEFAULT, **kw):
    p = dict(base)
    p.update(kw)
    return p


def observers(p):
    """a case is looked at twice: through its own min_cnt / min_sc and through the open observer"""
    return (p, dict(p, **OPEN))


def _sorted(x, y):
    x = np.asarray(x, np.uint64)
    y = np.asarray(y, np.uint64)
    o = np.lexsort((y, x))
    return np.ascontiguousarray(x[o]), np.ascontiguousarray(y[o])


# ---- generators -------------------------------------------------------------------------------------------------------------------
def colinear(seed, n, step=60, jitter=30, noise=0.2, x0=200_000):
    """sparse: one long colinear chain with jitter, one anchor per `step` bp on average, a fifth of the anchors random noise"""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.integers(0, step * n + 1, n)).astype(np.int64)
    y = (x + rng.integers(-jitter, jitter + 1, n)).clip(0, None)
    nz = rng.random(n) < noise
    y[nz] = rng.integers(0, step * n + 1, int(nz.sum()))
    return _sorted(x + x0, y.astype(np.uint64) | SPAN)


def satellite(seed, n, copies, period=171, gap=(5, 40)):
    """dense: a query crossing a tandem array — every query minimizer hits between copies / 2 and 2 copies neighbouring monomers (as _satellite_anchors
    of tests/test_kernels_emu.py), cut to exactly n anchors"""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    q = 100
    while len(xs) < n:
        q += int(rng.integers(gap[0], gap[1]))
        for k in rng.choice(np.arange(-copies, copies + 1), size=int(rng.integers(max(1, copies // 2), 2 * copies + 1)), replace=False):
            xs.append(1_000_000 + q + int(k) * period + int(rng.integers(-2, 3)))
            ys.append((15 << 32) | q)
    x, y = _sorted(xs[:n], ys[:n])
    return x, y


def uniform(n, spacing, x0=1_000_000):
    """anchors on one diagonal, x exactly `spacing` apart (the density probes count predecessors within max_dist_x: here a matter of division)"""
    x = x0 + spacing * np.arange(n, dtype=np.int64)
    return x.astype(np.uint64), (x - x0 + 50).astype(np.uint64) | SPAN


# ---- the dense rule, written twice in the product ------------------------------------------------------------------------------------
def probe(x, max_dist_x):
    """the 32 sample points of both density probes: anchor k = n * s / 33 (s = 1 .. 32) and the number of anchors in front of it with
    x >= x[k] - max_dist_x. Returns (worst, number of sample points with more than 128)."""
    n = len(x)
    cnt = []
    for s in range(1, 33):
        k = n * s // 33
        lim = int(x[k]) - max_dist_x if int(x[k]) > max_dist_x else 0
        cnt.append(k - int(np.searchsorted(x[:k], np.uint64(lim), side="left")))
    return max(cnt), sum(c > 128 for c in cnt)


def klass_chain_batch(x, max_dist_x):
    """wm_chain_batch (wm_index.hip, "chain.dense_probe" and klass_of): 0 dense | 1 large sparse | 2 n <= 1024 | 3 n <= 256; dense = worst > 900"""
    n = len(x)
    return 3 if n <= 256 else 2 if n <= 1024 else 0 if probe(x, max_dist_x)[0] > 900 else 1


def klass_window(x, max_dist_x):
    """win_plan_wave (window_kernel.h): the same classes; dense = worst > 900, or at least 8 of the 32 sample points with more than 128"""
    n = len(x)
    if n <= 1024:
        return 3 if n <= 256 else 2
    worst, over = probe(x, max_dist_x)
    return 0 if worst > 900 or over >= 8 else 1


# ---- SIZE_EDGES ----------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1087, 1088, 1089, 4095, 4096, 4097, 4160)


def size_edges():
    """the tile (64), the two small windows (256, 1024), the wrapping 1024-anchor window with a full / partial last flush tile (1087 / 1088 / 1089),
    the LDS / global split of sort and extraction and the W = 4096 window of the dense fill (4095 .. 4097), its first flush (4160)"""
    out = []
    for n in SIZES:
        x, y = colinear(100 + n, n)
        out.append(dict(name="size-sparse-%d" % n, group="size", x=x, y=y, par=par()))
        if n > 1024:
            x, y = satellite(200 + n, n, 12)
            out.append(dict(name="size-dense-%d" % n, group="size", x=x, y=y, par=par(STAGE2)))
    return out


# ---- DENSITY_EDGES -------------------------------------------------------------------------------------------------------------------
def clustered(edge_spacing=25):
    """1320 anchors, 1000 bp apart but for eight clusters that end at sample points 4, 8 .. 32 of the probes (anchor 40 s): seven of 135 anchors 5 bp
    apart (137 predecessors within any max_dist_x of 3000 .. 4000) and one, at sample point 16, of 140 anchors 25 bp apart (max_dist_x / 25
    predecessors): with max_dist_x = 3200 / 3225 seven / eight sample points lie over 128, the worst at 137"""
    n = 1320
    d = np.full(n, 1000, np.int64)
    for s in range(4, 33, 4):
        k = 40 * s
        if s == 16:
            d[k - 139:k + 1] = edge_spacing
        else:
            d[k - 134:k + 1] = 5
    x = 1_000_000 + np.cumsum(d)
    return x.astype(np.uint64), (x - 1_000_000 + 50).astype(np.uint64) | SPAN


def density_edges():
    """(case, worst, sample points over 128): the probe is moved across each threshold by max_dist_x alone"""
    out = []
    x, y = uniform(1500, 5)
    for mdx, worst in ((4500, 900), (4505, 901)):            # wm_chain_batch: sparse / dense; the window call: dense both times (every sample point over 128)
        out.append((dict(name="density-uniform-%d" % mdx, group="density", x=x, y=y, par=par(max_dist_x=mdx, max_dist_y=mdx)), worst, 30))
    x, y = clustered()
    for mdx, over in ((3200, 7), (3225, 8)):                 # the window call: sparse / dense; wm_chain_batch: sparse both times
        out.append((dict(name="density-clustered-%d" % mdx, group="density", x=x, y=y, par=par(max_dist_x=mdx, max_dist_y=mdx)), 137, over))
    return out


# ---- PARAM_EDGES ---------------------------------------------------------------------------------------------------------------------
MAX_SKIP = (0, 1, 25, 1000)
MAX_ITER = (0, 1, 63, 64, 65, 300, 5000)
GAP_SCALE = (0.5, 1.0, 2.5)
OBSERVERS = ((1, 0), (3, 40), (10, 200), (2, 20))


def param_sets(base):
    out = [("max_skip=%d" % v, par(base, max_skip=v)) for v in MAX_SKIP]
    out += [("max_iter=%d,min_dist_x=%d" % (v, m), par(base, max_iter=v, min_dist_x=m)) for v in MAX_ITER for m in (0, 1000, base["max_dist_x"])]
    out += [("gap_scale=%g" % v, par(base, gap_scale=v)) for v in GAP_SCALE]
    out += [("is_cdna", par(base, is_cdna=1, max_dist_x=200000, bw=200000)),                  # the splice distances (src/options.c:122)
            ("bw=0", par(base, bw=0)),
            ("max_dist_y=0", par(base, max_dist_y=0))]                                          # no predecessor is valid: f = span, no chains
    out += [("min_cnt=%d,min_sc=%d" % o, par(base, min_cnt=o[0], min_sc=o[1])) for o in OBSERVERS]
    return out


def decoy_block(v, dr_i, off=300, X=3_000_000, Y=50_000):
    """Two chains that cannot see each other (their diagonals lie 600 apart: beyond bw = 500) end in J2 and, one base further, in J; then v - 1 decoys
    (no predecessor of I: their y lies beyond it; none of each other: y falls), then I at dr_i from J, `off` above J's diagonal (300: between the two). J is predecessor i - v of
    I, J2 — twice the score — predecessor i - v - 1. Which of them the window [st, i) still holds is a matter of max_iter and min_dist_x alone."""
    xs = [X - 100 * k for k in range(7, -1, -1)] + [X - 1 - 100 * k for k in range(15, -1, -1)]
    ys = [Y - 100 * k for k in range(7, -1, -1)] + [Y + 599 - 100 * k for k in range(15, -1, -1)]
    dx = np.linspace(1, dr_i - 1, v - 1).astype(np.int64) if v > 1 else np.zeros(0, np.int64)
    assert len(np.unique(dx)) == len(dx)
    xs += [X + int(d) for d in dx]; ys += [Y + dr_i + 30000 - k for k in range(len(dx))]
    for k in range(5):                                                         # I and four anchors behind it: the chain through I outgrows the gap cost of joining it
        xs.append(X + dr_i + 15 * k); ys.append(Y + dr_i + off + 15 * k)
    return _sorted(xs, np.array(ys, np.uint64) | SPAN)


def skip_block(L, step=4, off=600, nk=300, tail=6, X=3_000_000, Y=50_000):
    """a chain K of nk anchors that ends in J, a dense chain of L anchors `step` bp apart on a diagonal `off` away (beyond bw: no anchor of it chains with
    K), then I half way between the two diagonals, and tail - 1 anchors behind it. I's scan improves on the nearest dense anchor, skips the L - 1 others —
    each marked by the one behind it — and reaches J, the better predecessor, only if max_skip >= L - 1."""
    xs = [X - 15 * k for k in range(nk - 1, -1, -1)]; ys = [Y - 15 * k for k in range(nk - 1, -1, -1)]
    xs += [X + 10 + step * k for k in range(L)]; ys += [Y + off + 10 + step * k for k in range(L)]
    for k in range(tail):
        xs.append(X + 10 + step * L + off + 15 * k); ys.append(Y + off // 2 + 10 + step * L + off + 15 * k)
    return _sorted(xs, np.array(ys, np.uint64) | SPAN)


def observer_chains(X=5_000_000, Y=60_000):
    """chains far from everything else whose count and score sit on the observers' thresholds: 14 anchors scoring exactly 200 (13 x 15 + 5), two scoring
    exactly 20 (15 + 5), ten of span 28 scoring 280; and twins one base apart on both axes (the only predecessors that max_dist_y = 1 admits)"""
    xs, ys = [], []
    for k in range(14):
        d = 20 * k if k < 13 else 20 * 12 + 5
        xs.append(X + d); ys.append((15 << 32) | (Y + d))
    xs += [X + 50_000, X + 50_005]; ys += [(15 << 32) | Y, (15 << 32) | (Y + 5)]
    for k in range(10):
        xs.append(X + 100_000 + 30 * k); ys.append((28 << 32) | (Y + 30 * k))
    for k in range(4):
        xs += [X + 150_000 + 20_000 * k, X + 150_001 + 20_000 * k]; ys += [(15 << 32) | (Y + 7 * k), (15 << 32) | (Y + 7 * k + 1)]
    return np.array(xs, np.uint64), np.array(ys, np.uint64)


PARAM_SPARSE = dict(seed=7, n=266)
PARAM_DENSE = dict(seed=11, n=1400, copies=20)
WIDE2 = dict(seed=13, n=7000, copies=40)


def param_edges():
    out = []
    sx, sy = colinear(PARAM_SPARSE["seed"], PARAM_SPARSE["n"], step=40)
    ox, oy = observer_chains()
    sx, sy = _sorted(np.concatenate([sx, ox]), np.concatenate([sy, oy]))                      # 300 anchors
    dx, dy = satellite(PARAM_DENSE["seed"], PARAM_DENSE["n"], PARAM_DENSE["copies"])
    for name, p in param_sets(DEFAULT):
        out.append(dict(name="param-sparse-" + name, group="param", x=sx, y=sy, par=p))
    for name, p in param_sets(STAGE2):
        out.append(dict(name="param-dense-" + name, group="param", x=dx, y=dy, par=p))
    # hand-placed windows: the predecessor that max_iter = v just keeps (v - 1 drops it, v + 1 admits a better one), alone (one wavefront) and behind the dense set
    for v in MAX_ITER[2:]:
        bx, by = decoy_block(v, v + 400)
        base = STAGE2 if v == 5000 else DEFAULT
        out.append(dict(name="param-window-max_iter=%d" % v, group="param", x=bx, y=by, par=par(base, max_iter=v, min_dist_x=0)))
        if v < 5000:
            x, y = _sorted(np.concatenate([dx, bx]), np.concatenate([dy, by]))
            out.append(dict(name="param-dense+window-max_iter=%d" % v, group="param", x=x, y=y, par=par(STAGE2, max_iter=v, min_dist_x=0)))
    # ... and the one that min_dist_x just keeps when max_iter (65) would have dropped it
    for m in (1000, 5000):
        bx, by = decoy_block(121, m, off=-300)                    # (below J's diagonal: dq = m - 300 stays within max_dist_y; J2 is out of the band)
        out.append(dict(name="param-window-min_dist_x=%d" % m, group="param", x=bx, y=by, par=par(max_iter=65, min_dist_x=m)))
    bx, by = skip_block(1001)
    out.append(dict(name="param-skip-1000", group="param", x=bx, y=by, par=par(max_skip=1000)))
    # the same beyond the 4096-anchor LDS window: the break falls on a predecessor whose mark lives in the global slab (st < lo: the far-mark branch)
    bx, by = skip_block(4500, step=2, off=2400, nk=700, tail=16)
    out.append(dict(name="param-skip-far-4400", group="param", x=bx, y=by, par=par(STAGE2, max_skip=4400)))
    return out


def wide_second_step():
    """~7000 anchors within little more than max_dist_x = 16000 bp, max_iter = 8000, max_skip = 1000: predecessor windows beyond NWV * KT * 64 = 5120
    (chain_block_wide takes a second step) and beyond the 4096-anchor LDS window (the global slab and its marks)"""
    x, y = satellite(WIDE2["seed"], WIDE2["n"], WIDE2["copies"], gap=(5, 20))
    return dict(name="param-dense-7000-second-step", group="wide2", x=x, y=y, par=par(STAGE2, max_iter=8000, max_skip=1000))


# ---- SCORE_EDGES ---------------------------------------------------------------------------------------------------------------------
SCORE_PARS = (("bw500", par()),                                                # bw = 500 binds (dd = 500 / 501); distances 5000
              ("y3000", par(max_dist_y=3000, bw=2500)),                        # max_dist_y = 3000 binds (dq = 3000 / 3001), bw = 2500 (dd = 2500 / 2501)
              ("x3000", par(max_dist_x=3000, bw=2500)))                        # max_dist_x = 3000 binds: x[i] - x[st] = 3000 / 3001, and dq = 3001 at dr <= 3000
REV = 1 << 63
RID1 = 1 << 32
TANDEM, SELF = 1 << 42, 1 << 43


def _probes():
    """hand-placed groups, 40 000 bp apart (no group sees another): colinear anchors, then one probe anchor at (dr, dq) from the last of them"""
    rel = [(0, 50), (50, 0), (50, -30)]                                        # dr = 0; dq = 0; dq < 0
    for d in (3000, 5000):                                                     # dq (and dr) at a distance limit and one beyond; dq alone one beyond
        rel += [(d, d), (d + 1, d + 1), (d, d + 1), (d + 1, d), (d, d - 100), (d + 1, d - 99)]
    for b in (500, 2500):                                                      # dd at the band width and one beyond, on either side of the diagonal
        m = 5 if b == 500 else 16                                              # (m anchors of span 28, 30 bp apart, in front: the chain outweighs the gap cost of dd = b)
        rel += [(400 + b, 400, m), (401 + b, 400, m), (400, 400 + b, m), (400, 401 + b, m)]
    xs, ys = [], []
    X = 50_000
    for g, r in enumerate(rel):
        dr, dq = r[:2]
        Y = 20_000 + 97 * g
        if len(r) == 2:
            for k in range(3):
                xs.append(X + 100 * k); ys.append((15 << 32) | (Y + 100 * k))
        else:
            for k in range(r[2]):
                xs.append(X + 200 - 30 * (r[2] - 1 - k)); ys.append((28 << 32) | (Y + 200 - 30 * (r[2] - 1 - k)))
        xs.append(X + 200 + dr); ys.append((15 << 32) | (Y + 200 + dq))
        X += 40_000
    # two predecessors with equal score: A and B do not chain with each other (dq < 0), C scores 28 through either — the first visited (B) must win
    xs += [X, X + 10, X + 110]; ys += [(15 << 32) | 9000, (15 << 32) | 8990, (15 << 32) | 9100]
    X += 40_000
    # mixed spans, steps around them (min(dq, dr, span) takes each of its three arguments), the tandem and SELF bits of y on some
    q = 3000
    for k, (sp, step) in enumerate(((11, 12), (15, 10), (19, 25), (28, 20), (28, 30), (11, 9), (19, 19), (15, 40), (28, 27), (11, 30))):
        X += step; q += step + (k % 3 - 1)
        xs.append(X); ys.append((sp << 32) | q | (TANDEM if k % 3 == 0 else 0) | (SELF if k % 4 == 1 else 0))
    return np.array(xs, np.uint64), np.array(ys, np.uint64)


def score_job(n):
    """the probes on strand 0 / contig 0 — and, where n has room, again on the reverse strand of contig 1 — padded to n anchors with sparse colinear
    anchors on contig 1 and on the reverse strand of contig 0, whose low words of x interleave with the probes' (the fill scores on the low words; st is
    advanced on all 64 bits)"""
    px, py = _probes()
    twice = n >= 2 * len(px) + 100
    n_pad = n - (2 if twice else 1) * len(px)
    assert n_pad >= 100
    ax, ay = colinear(31 + n, n_pad // 2, x0=49_000)
    bx, by = colinear(32 + n, n_pad - n_pad // 2, x0=50_050)
    x = np.concatenate([px, ax | np.uint64(RID1), bx | np.uint64(REV)] + ([px | np.uint64(REV | RID1)] if twice else []))
    y = np.concatenate([py, ay | np.uint64(TANDEM), by | np.uint64(SELF)] + ([py] if twice else []))
    return _sorted(x, y)


def score_edges():
    out = []
    for n in (300, 1100):
        x, y = score_job(n)
        for name, p in SCORE_PARS:
            out.append(dict(name="score-%d-%s" % (n, name), group="score", x=x, y=y, par=p))
    return out


# ---- everything ----------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def all_cases():
    if "all" not in _CACHE:
        _CACHE["all"] = size_edges() + [c for c, _, _ in density_edges()] + param_edges() + [wide_second_step()] + score_edges()
        for c in _CACHE["all"]:
            c["x"].setflags(write=False); c["y"].setflags(write=False)
    return _CACHE["all"]


# (parameter, edge value, neighbouring value): the oracle's output of at least one case that carries the edge value must change when the neighbour
# takes its place — under the case's own observer or the open one (tests/test_chain_edges_emu.py::test_every_edge_value_matters)
NEIGHBOURS = ([("max_skip", 0, 1), ("max_skip", 1, 2), ("max_skip", 25, 26), ("max_skip", 1000, 999), ("max_skip", 4400, 4499)] +
              [("max_iter", v, v + 1) for v in MAX_ITER] + [("max_iter", v, v - 1) for v in MAX_ITER[1:]] +
              [("min_dist_x", 0, 1), ("min_dist_x", 1000, 999), ("min_dist_x", 5000, 4999)] +
              [("gap_scale", 0.5, 0.55), ("gap_scale", 1.0, 1.05), ("gap_scale", 2.5, 2.45), ("is_cdna", 1, 0)] +
              [("bw", 0, 1), ("bw", 500, 499), ("bw", 2500, 2499), ("max_dist_y", 0, 1), ("max_dist_y", 3000, 2999), ("max_dist_y", 5000, 4999),
               ("max_dist_x", 3000, 2999), ("max_dist_x", 5000, 4999)] +
              [("min_cnt", 1, 2), ("min_cnt", 2, 3), ("min_cnt", 3, 4), ("min_cnt", 10, 11), ("min_sc", 0, 16), ("min_sc", 20, 21), ("min_sc", 40, 41), ("min_sc", 200, 201)])
