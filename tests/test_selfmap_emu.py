"""Self / all-vs-all mapping (-D, --dual=no, -X) on the CPU: the name filter of the two seeding kernels (win_seed_wave, seed_wave) on the host wavefront
emulator against skip_seed + collect_seed_hits (src/map.c:132-154, 222-251) restated here with C's own strcmp, and the host's name ranking
(winnowmap_amd/csrc/host/wm_names.h) against the sign of strcmp."""
import ctypes as C
import ctypes.util
import numpy as np
import pytest
import wmtest as W
from winnowmap_amd import build
from test_kernels_emu import _load_emu

NO_DIAG, NO_DUAL, FOR_ONLY, REV_ONLY = 0x1, 0x2, 0x100000, 0x200000
SEED_TANDEM, SEED_SELF = 1 << 42, 1 << 43
M64 = (1 << 64) - 1

libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
libc.strcmp.argtypes = [C.c_char_p, C.c_char_p]
libc.strcmp.restype = C.c_int


def c_strcmp(a, b):
    return libc.strcmp(a, b)


@pytest.fixture(scope="module")
def emus():
    S = C.CDLL(build.build_emu_selfmap())
    u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
    S.emu_names_rank.argtypes = [C.c_int, C.POINTER(C.c_char_p), u32p]
    S.emu_names_key.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, u32p]
    head = [W.u64p, W.u64p, W.u64p, C.c_int, u32p, u32p, W.u64p, W.u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
    S.emu_self_seed.argtypes = head + [W.u64p, W.u64p, C.c_int, W.i32p]
    S.emu_self_win_seed.argtypes = head + [C.c_int, W.u64p, W.u64p, W.u64p, W.u64p, C.c_int, W.i32p]
    E = _load_emu()
    E.emu_win_small.argtypes = [C.c_int, C.c_int, C.c_int, W.u64p, W.u64p] + [C.c_int] * 8 + [C.c_float, C.POINTER(C.c_int), W.u64p]
    return S, E


def _rank(S, names):
    arr = (C.c_char_p * len(names))(*names)
    rank = np.zeros(len(names), np.uint32)
    nd = S.emu_names_rank(len(names), arr, rank)
    return rank, nd


def _key(S, names, q):
    arr = (C.c_char_p * len(names))(*names)
    out = np.zeros(2, np.uint32)
    S.emu_names_key(len(names), arr, q, out)
    return int(out[0]), int(out[1])


def _random_name(rng):
    shape = rng.integers(0, 6)
    i = int(rng.integers(0, 40))
    if shape == 0:
        return b"r%d" % i
    if shape == 1:
        return b"read_%04d" % i
    if shape == 2:
        return b"r%d/ccs" % i
    if shape == 3:
        return b"R%d" % i
    if shape == 4:          # bytes >= 0x80: strcmp compares UNSIGNED chars
        return bytes(rng.integers(1, 256, int(rng.integers(1, 5))).astype(np.uint8).tolist()).replace(b"\0", b"\x01")
    return (b"r%d" % i)[:int(rng.integers(1, 3))]      # prefixes of other names


def test_rank_scheme_reproduces_the_sign_of_strcmp(emus):
    S, _ = emus
    rng = np.random.default_rng(5)
    n_pairs = 0
    for it in range(250):
        names = [_random_name(rng) for _ in range(int(rng.integers(1, 30)))]
        if it % 3 == 0:
            names += [names[0], names[0] + b"x", names[0][:1]]                  # duplicate contig names, names that are prefixes of one another
        if it % 5 == 0:
            names += [b"\x7f", b"\x80", b"\xff", b"a\xe9", b"az"]
        rank, nd = _rank(S, names)
        assert nd == len(set(names)) and rank.max() == nd - 1
        queries = [names[int(rng.integers(0, len(names)))] for _ in range(20)] + [_random_name(rng) for _ in range(20)] + [b"", b"\xff\xff", b"zzzz_absent"]
        for q in queries:
            lo, eq = _key(S, names, q)
            assert eq == (q in names)
            for rid, nm in enumerate(names):
                cmp = c_strcmp(q, nm)
                assert (cmp == 0) == (eq == 1 and rank[rid] == lo), (q, nm)
                assert (cmp > 0) == (rank[rid] < lo), (q, nm)
                n_pairs += 1
    assert n_pairs >= 10000


def _slot(key, hbits):
    return ((key * 0x9E3779B97F4A7C15) & M64) >> (64 - hbits)


def _make_case(rng, qname_mode, max_occ=6):
    """a small flat index (open addressing, as host/wm_index.h) over contigs with awkward names, and the minimizers of one query that is a copy of
    stretches of several contigs — among them contigs that carry the query's name, with and without its length"""
    qlen = int(rng.integers(600, 3000))
    qname = _random_name(rng)
    names, lens = [], []
    for _ in range(int(rng.integers(3, 12))):
        names.append(_random_name(rng)); lens.append(int(rng.integers(qlen + 400, qlen + 3000)))
    if qname_mode != "absent":
        names.append(qname); lens.append(qlen)                                  # the query itself is a contig
        names.append(qname); lens.append(qlen + 7)                              # equal name, different length
        if qname_mode == "dup":
            names.append(qname); lens.append(qlen)                              # duplicate contig name with the same length
        names.append(qname + b"/1"); lens.append(qlen)                          # the query's name is a prefix of this one
        names.append(qname[:-1] or b"!"); lens.append(qlen)                     # ... and this one a prefix of the query's
    else:
        names = [n for n in names if n != qname] or [qname + b"_"]
        lens = lens[:len(names)]
    order = rng.permutation(len(names))
    names = [names[i] for i in order]; lens = [lens[i] for i in order]
    n_ctg = len(names)
    # minimizers: increasing positions, ~1 in 8 repeats the previous key (tandem), both strands
    n_mini = int(rng.integers(20, 150))
    pos = np.sort(rng.choice(np.arange(20, qlen - 1), n_mini, replace=False))
    keys = [int(k) for k in rng.integers(1, 1 << 28, n_mini)]
    for i in range(1, n_mini):
        if rng.random() < 0.12:
            keys[i] = keys[i - 1]
    strand = rng.integers(0, 2, n_mini)
    span = 15
    mx = np.array([k << 8 | span for k in keys], np.uint64)
    my = np.array([int(p) << 1 | int(s) for p, s in zip(pos, strand)], np.uint64)
    # occurrences: every key is found, colinear with the query, on a few contigs at fixed offsets (so that chains exist); on contigs with the query's
    # name at offset 0 (the diagonal) AND at an offset (an off-diagonal self hit); a few keys are over-represented (dropped: rep_len)
    offs = {rid: int(rng.integers(0, 300)) for rid in range(n_ctg)}
    occ = {}
    for k, p, s in zip(keys, pos, strand):
        lst = occ.setdefault(k, [])
        if rng.random() < 0.06:
            for _ in range(max_occ + int(rng.integers(0, 3))):
                rid = int(rng.integers(0, n_ctg)); lst.append(rid << 32 | int(rng.integers(0, lens[rid])) << 1 | int(rng.integers(0, 2)))
            continue
        for rid in range(n_ctg):
            same = names[rid] == qname
            if same or rng.random() < 0.5:
                rs = int(s) if rng.random() < 0.8 else 1 - int(s)
                if same:
                    lst.append(rid << 32 | int(p) << 1 | rs)                    # diagonal position, either strand
                lst.append(rid << 32 | (int(p) + 1 + offs[rid]) << 1 | rs)
    P, table = [], {}
    for k, lst in occ.items():
        lst = sorted(set(lst))
        table[k] = (len(P), len(lst)); P += lst
    hbits = 4
    while (1 << hbits) < 2 * len(table) + 2:
        hbits += 1
    hkey = np.full(1 << hbits, M64, np.uint64); hval = np.zeros(1 << hbits, np.uint64)
    for k, (first, cnt) in table.items():
        s = _slot(k, hbits)
        while int(hkey[s]) != M64:
            s = (s + 1) & ((1 << hbits) - 1)
        hkey[s] = k; hval[s] = first << 32 | cnt
    return dict(qname=qname, qlen=qlen, names=names, lens=np.array(lens, np.uint32), mx=mx, my=my, P=np.array(P + [0], np.uint64), table=table,
                hkey=hkey, hval=hval, hbits=hbits, max_occ=max_occ)


def _skip_seed(flag, r, q_pos, qname, qlen, names, lens):
    """src/map.c:132-154, literally"""
    is_self = 0
    if qname is not None and (flag & (NO_DIAG | NO_DUAL)):
        rid = r >> 32
        cmp = c_strcmp(qname, names[rid])
        if (flag & NO_DIAG) and cmp == 0 and int(lens[rid]) == qlen:
            if (r & 0xffffffff) >> 1 == q_pos >> 1:
                return 1, 0
            if (r & 1) == (q_pos & 1):
                is_self = 1
        if (flag & NO_DUAL) and cmp > 0:
            return 1, is_self
    if flag & (FOR_ONLY | REV_ONLY):
        if (r & 1) == (q_pos & 1):
            if flag & REV_ONLY:
                return 1, is_self
        elif flag & FOR_ONLY:
            return 1, is_self
    return 0, is_self


def _collect_seed_hits(c, flag, qname):
    """src/map.c:97-130, 222-251 before the sort"""
    ex, ey = [], []
    rep_st = rep_en = rep = 0
    mx, my, qlen = c["mx"], c["my"], c["qlen"]
    for i in range(len(mx)):
        x, y = int(mx[i]), int(my[i])
        first, t = c["table"][x >> 8]
        q_pos, span = y & 0xffffffff, x & 0xff
        if t >= c["max_occ"]:
            en = (q_pos >> 1) + 1; st = en - span
            if st > rep_en:
                rep += rep_en - rep_st; rep_st, rep_en = st, en
            else:
                rep_en = en
            continue
        tand = (i > 0 and int(mx[i - 1]) >> 8 == x >> 8) or (i < len(mx) - 1 and int(mx[i + 1]) >> 8 == x >> 8)
        for r in c["P"][first:first + t]:
            r = int(r)
            skip, is_self = _skip_seed(flag, r, q_pos, qname, qlen, c["names"], c["lens"])
            if skip:
                continue
            rpos = (r & 0xffffffff) >> 1
            if (r & 1) == (q_pos & 1):
                X = (r & 0xffffffff00000000) | rpos; Y = span << 32 | q_pos >> 1
            else:
                X = 1 << 63 | (r & 0xffffffff00000000) | rpos; Y = span << 32 | (qlen - ((q_pos >> 1) + 1 - span) - 1)
            if tand:
                Y |= SEED_TANDEM
            if is_self:
                Y |= SEED_SELF
            ex.append(X); ey.append(Y)
    rep += rep_en - rep_st
    return np.array(ex, np.uint64), np.array(ey, np.uint64), rep


def _pairs(x, y):
    return sorted(zip(x.tolist(), y.tolist()))


FLAGS = [0, NO_DIAG, NO_DUAL, NO_DIAG | NO_DUAL]
CHAIN = dict(max_dist_x=5000, min_dist_x=1000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, min_cnt=2, min_sc=20)


@pytest.mark.parametrize("name_flag", FLAGS)
@pytest.mark.parametrize("strand_flag", [0, FOR_ONLY, REV_ONLY])
def test_seeding_kernels_apply_skip_seed(emus, name_flag, strand_flag):
    S, E = emus
    rng = np.random.default_rng(100 + name_flag * 7 + (strand_flag >> 20))
    flag = name_flag | strand_flag
    n_self = n_diag_dropped = n_dual_dropped = n_chains = 0
    for it in range(30):
        c = _make_case(rng, ("self", "dup", "absent")[it % 3])
        rank, _ = _rank(S, c["names"])
        lo, eq = _key(S, c["names"], c["qname"])
        ex, ey, erep = _collect_seed_hits(c, flag, c["qname"])
        bx, by, _ = _collect_seed_hits(c, strand_flag, None)                   # what a job without a key gives
        n_self += int(np.count_nonzero(ey & np.uint64(SEED_SELF)))
        n_diag_dropped += (name_flag == NO_DIAG) * (len(bx) - len(ex))
        n_dual_dropped += (name_flag == NO_DUAL) * (len(bx) - len(ex))
        cap = len(bx) + 16
        head = (c["hkey"], c["hval"], c["P"], c["hbits"], rank, c["lens"], c["mx"], c["my"], len(c["mx"]), c["qlen"], c["max_occ"], flag, lo, eq)
        # seed_wave
        ax, ay, res = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(3, np.int32)
        S.emu_self_seed(*head, ax, ay, cap, res)
        assert res[0] == len(ex) and res[1] == erep, (it, res, len(ex), erep)
        assert _pairs(ax[:res[0]], ay[:res[0]]) == _pairs(ex, ey), it
        # win_seed_wave, with handed-in anchors in front (n_pre > 0 in every other case)
        n_pre = int(rng.integers(1, 9)) if it % 2 else 0
        px = np.sort(rng.integers(0, 1 << 20, n_pre).astype(np.uint64) | np.uint64(int(rng.integers(0, len(c["names"]))) << 32))
        py = (rng.integers(0, c["qlen"], n_pre).astype(np.uint64) | np.uint64(15 << 32))
        wx, wy = np.zeros(cap + n_pre, np.uint64), np.zeros(cap + n_pre, np.uint64)
        S.emu_self_win_seed(*head, n_pre, px if n_pre else np.zeros(1, np.uint64), py if n_pre else np.zeros(1, np.uint64), wx, wy, cap + n_pre, res)
        assert res[2] == 0 and res[0] == n_pre + len(ex) and res[1] == erep, (it, res)
        assert np.array_equal(wx[:n_pre], px) and np.array_equal(wy[:n_pre], py)
        assert _pairs(wx[n_pre:res[0]], wy[n_pre:res[0]]) == _pairs(ex, ey), it
        # ... and a job without a key takes the old path whatever the name tables hold: the two name bits never travel without one
        S.emu_self_win_seed(*head[:11], strand_flag, 0, 0, 0, np.zeros(1, np.uint64), np.zeros(1, np.uint64), wx, wy, cap + n_pre, res)
        assert res[0] == len(bx) and _pairs(wx[:res[0]], wy[:res[0]]) == _pairs(bx, by)
        # sort -> chain fill -> extraction (win_small_wave): bit 43 rides along untouched, the chains are the oracle's on the same anchors
        n = n_pre + len(ex)
        if n == 0 or n > 256:
            continue
        S.emu_self_win_seed(*head, n_pre, px if n_pre else np.zeros(1, np.uint64), py if n_pre else np.zeros(1, np.uint64), wx, wy, cap + n_pre, res)
        sx, sy = W.o_radix_sort_128x(ex, ey)                                    # src/map.c:252 ...
        ox, oy = np.concatenate([px, sx]), np.concatenate([py, sy])
        if n_pre:
            ox, oy = W.o_radix_sort_128x(ox, oy)                                # ... and :833 when anchors were handed in
        eu, evx, evy = W.o_chain_dp(ox, oy, **CHAIN)
        gx, gy = wx[:n].copy(), wy[:n].copy()
        n_u, gu = C.c_int(0), np.zeros(n + 16, np.uint64)
        n_v = E.emu_win_small(n, n_pre, 1, gx, gy, CHAIN["max_dist_x"], CHAIN["min_dist_x"], CHAIN["max_dist_y"], CHAIN["bw"], CHAIN["max_skip"], CHAIN["max_iter"],
                              CHAIN["min_cnt"], CHAIN["min_sc"], 1.0, C.byref(n_u), gu)
        assert n_u.value == len(eu) and np.array_equal(gu[:n_u.value], eu), it
        assert n_v == len(evx) and np.array_equal(gx[:n_v], evx) and np.array_equal(gy[:n_v], evy), it
        n_chains += len(eu)
    assert n_chains > 0
    if (name_flag & NO_DIAG) and strand_flag != REV_ONLY:                       # (MM_SEED_SELF goes to same-strand anchors, which REV_ONLY drops)
        assert n_self > 0                                                       # off-diagonal self anchors carry MM_SEED_SELF
    if name_flag == NO_DIAG:
        assert n_diag_dropped > 0
    if name_flag == NO_DUAL:
        assert n_dual_dropped > 0
