"""--heap-sort=yes (MM_F_HEAP_SORT) on the CPU: the heap-merged seed order of collect_seed_hits_heap (src/map.c:156-220).

The expected list comes from the loop of src/map.c:169-218 restated here and driven by the REFERENCE's own heap (ks_heapmake_heap / ks_heapdown_heap of
KSORT_INIT(heap, mm128_t, heap_lt), exported by oracle/_ref/libwinnowmap_ref.so). Against it: the host restatement (csrc/host/wm_core.cpp: seed_hits_heap) and
the two seeding kernels with the ordering stage of their launchers on the wavefront emulator (tests/simt_emu/emu_heapseed.cpp), bit for bit. The emulator's
event counters say which road a job took: 0 = the sorted list was kept (no two anchors share x), 1 = the heap was replayed, 2 = the heap lived in global memory.

Not covered: a hand-over of giant tied jobs to the host — none was built, a tied job of any size is replayed on the device."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
from winnowmap_amd import build
from test_selfmap_emu import _skip_seed, _collect_seed_hits, _slot, _random_name, _rank, _key, M64, NO_DIAG, NO_DUAL, FOR_ONLY, REV_ONLY, SEED_TANDEM, SEED_SELF

HEAP = 0x400000
SPAN = 15
Z1 = np.zeros(1, np.uint64)


@pytest.fixture(scope="module")
def emus():
    S = C.CDLL(build.build_emu_selfmap())
    S.emu_names_rank.argtypes = [C.c_int, C.POINTER(C.c_char_p), W.u32p]
    S.emu_names_key.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, W.u32p]
    H = C.CDLL(build.build_emu_heapseed())
    head = [W.u64p, W.u64p, W.u64p, C.c_int, W.u32p, W.u32p, W.u64p, W.u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
    H.emu_heap_events.argtypes = [C.POINTER(C.c_long), C.c_int]
    H.emu_host_heapmake.argtypes = [C.c_size_t, W.u64p, W.u64p]
    H.emu_host_heapdown.argtypes = [C.c_size_t, C.c_size_t, W.u64p, W.u64p]
    H.emu_host_seed_heap.argtypes = head + [C.c_int, W.u64p, W.u64p, C.c_int, W.i32p]
    H.emu_heap_seed.argtypes = head + [C.c_int, W.u64p, W.u64p, C.c_int, W.i32p]
    H.emu_heap_window.argtypes = head + [C.c_int, C.c_int, W.u64p, W.u64p, C.c_int, C.c_int, C.c_int, W.u64p, W.u64p, C.c_int, W.i32p]
    return S, H


@pytest.fixture(scope="module")
def refheap():
    """the reference's instantiation of the heap (src/map.c:87-88), on [n, 2] uint64 arrays (mm128_t: x, y)"""
    if not W.have_ref():
        pytest.skip("oracle/_ref/libwinnowmap_ref.so not built")
    L = C.CDLL(W.REF_SO)
    mk, dn = getattr(L, "_Z16ks_heapmake_heapmP7mm128_t"), getattr(L, "_Z16ks_heapdown_heapmmP7mm128_t")
    mk.argtypes = [C.c_size_t, C.c_void_p]; mk.restype = None
    dn.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p]; dn.restype = None
    return mk, dn


def events(H, reset=True):
    out = (C.c_long * 4)()
    H.emu_heap_events(out, 1 if reset else 0)
    return list(out)


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def _index(table):
    """flat index (open addressing, as host/wm_index.h) of {key: [r, ...]}: every list strictly ascending, its entries distinct (src/index.c:239)"""
    P, tab = [], {}
    for k, lst in table.items():
        lst = sorted(set(lst))
        tab[k] = (len(P), len(lst)); P += lst
    hbits = 4
    while (1 << hbits) < 2 * len(tab) + 2:
        hbits += 1
    hkey = np.full(1 << hbits, M64, np.uint64); hval = np.zeros(1 << hbits, np.uint64)
    for k, (first, cnt) in tab.items():
        s = _slot(k, hbits)
        while int(hkey[s]) != M64:
            s = (s + 1) & ((1 << hbits) - 1)
        hkey[s] = k; hval[s] = first << 32 | cnt
    return dict(P=np.array(P + [0], np.uint64), table=tab, hkey=hkey, hval=hval, hbits=hbits)


class _Tab(dict):
    """{key: (first, count)}; a key the index does not hold has no occurrence (mm_idx_get: n = 0)"""
    def __missing__(self, k):
        return (0, 0)


def craft(minis, table, qlen=6000, names=(b"c0",), lens=None, qname=b"q", max_occ=6):
    """minis: [(key, pos, strand)] in query order; table: {key: [rid << 32 | pos << 1 | strand]}"""
    c = _index(table)
    c["table"] = _Tab(c["table"])
    c.update(qname=qname, qlen=qlen, names=list(names), lens=np.array(lens if lens is not None else [1 << 20] * len(names), np.uint32), max_occ=max_occ,
             mx=np.array([k << 8 | SPAN for k, _, _ in minis] or [0], np.uint64)[:len(minis)], my=np.array([p << 1 | s for _, p, s in minis] or [0], np.uint64)[:len(minis)])
    return c


def make_case(rng, qname_mode="absent", tie_p=0.45, n_mini=(20, 150), max_occ=6, n_ctg=None, hit_p=0.5):
    """tests/test_selfmap_emu.py::_make_case with the share of repeated keys raised: a minimizer repeats the key of its predecessor (a tandem seed) or of any
    earlier minimizer with probability tie_p — two minimizers of one key and strand reach every position of the key's list, so their anchors share x.
    tie_p = 0: every key once, no two anchors share x."""
    qlen = int(rng.integers(600, 3000)) + 4 * n_mini[1]
    qname = _random_name(rng)
    names, lens = [], []
    for _ in range(n_ctg or int(rng.integers(2, 8))):
        names.append(_random_name(rng)); lens.append(int(rng.integers(qlen + 400, qlen + 3000)))
    if qname_mode != "absent":
        names += [qname, qname, qname + b"/1", qname[:-1] or b"!"]; lens += [qlen, qlen + 7, qlen, qlen]
    else:
        keep = [i for i, n in enumerate(names) if n != qname]
        names = [names[i] for i in keep] or [qname + b"_"]; lens = [lens[i] for i in keep] or [qlen + 500]
    order = rng.permutation(len(names))
    names = [names[i] for i in order]; lens = [lens[i] for i in order]
    n_ctg = len(names)
    nm = int(rng.integers(n_mini[0], n_mini[1] + 1))
    pos = np.sort(rng.choice(np.arange(20, qlen - 1), nm, replace=False))
    keys = list(dict.fromkeys(rng.integers(1, 1 << 28, 2 * nm + 8).tolist()))[:nm]      # distinct
    assert len(keys) == nm
    strand = rng.integers(0, 2, nm)
    for i in range(1, nm):
        if rng.random() < tie_p:
            j = i - 1 if rng.random() < 0.5 else int(rng.integers(0, i))
            keys[i] = keys[j]
            if rng.random() < 0.7:
                strand[i] = strand[j]
    offs = {rid: int(rng.integers(0, 300)) for rid in range(n_ctg)}
    occ = {}
    for k, p, s in zip(keys, pos, strand):
        if k in occ:
            continue
        lst = occ[k] = []
        u = rng.random()
        if u < 0.05:                                                             # over-represented: dropped, counted in rep_len
            while len(set(lst)) < max_occ + int(rng.integers(0, 3)):
                rid = int(rng.integers(0, n_ctg)); lst.append(rid << 32 | int(rng.integers(0, lens[rid])) << 1 | int(rng.integers(0, 2)))
            continue
        if u < 0.10:                                                             # in the index's key space but without occurrences: never enters the heap
            del occ[k]
            continue
        for rid in range(n_ctg):
            same = names[rid] == qname
            if same or rng.random() < hit_p:
                rs = int(s) if rng.random() < 0.7 else 1 - int(s)
                if same:
                    lst.append(rid << 32 | int(p) << 1 | rs)
                lst.append(rid << 32 | (int(p) + 1 + offs[rid]) << 1 | rs)
                if rng.random() < 0.3 and len(lst) < max_occ - 1:                 # both strands of one reference position: r differs, x can tie across strands
                    lst.append(lst[-1] ^ 1)
        if len(set(lst)) >= max_occ:
            del lst[max_occ - 1:]
    return craft([(int(k), int(p), int(s)) for k, p, s in zip(keys, pos, strand)], occ, qlen=qlen, names=names, lens=lens, qname=qname, max_occ=max_occ)


def has_tie(x):
    return len(np.unique(x)) < len(x)


# ------------------------------------------------------------------------------------------------
# src/map.c:156-220 with the reference's heap
# ------------------------------------------------------------------------------------------------
def ref_heap_list(refheap, c, flag, qname):
    mk, dn = refheap
    mx, my, qlen, P = c["mx"], c["my"], c["qlen"], c["P"]
    m, n_a = [], 0                                                               # collect_matches, :97-130
    rep_st = rep_en = rep = 0
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
        m.append((t, q_pos, span, tand, first)); n_a += t
    rep += rep_en - rep_st
    heap = np.zeros((len(m) + 1, 2), np.uint64)
    hs = 0
    for i, q in enumerate(m):                                                    # :169-175
        if q[0] > 0:
            heap[hs, 0] = P[q[4]]; heap[hs, 1] = i << 32; hs += 1
    hp = heap.ctypes.data
    mk(hs, hp)                                                                   # :176
    a = [None] * n_a
    n_for = n_rev = 0
    while hs > 0:                                                                # :177-205
        r, y = int(heap[0, 0]), int(heap[0, 1])
        t, q_pos, span, tand, first = m[y >> 32]
        skip, is_self = _skip_seed(flag, r, q_pos, qname, qlen, c["names"], c["lens"])
        if not skip:
            rpos = (r & 0xffffffff) >> 1
            if (r & 1) == (q_pos & 1):
                X = (r & 0xffffffff00000000) | rpos; Y = span << 32 | q_pos >> 1
                slot = n_for; n_for += 1
            else:
                X = 1 << 63 | (r & 0xffffffff00000000) | rpos; Y = span << 32 | (qlen - ((q_pos >> 1) + 1 - span) - 1)
                n_rev += 1; slot = n_a - n_rev
            if tand:
                Y |= SEED_TANDEM
            if is_self:
                Y |= SEED_SELF
            a[slot] = (X, Y)
        if (y & 0xffffffff) < t - 1:
            heap[0, 1] = y + 1
            heap[0, 0] = P[first + (y & 0xffffffff) + 1]
        else:
            heap[0] = heap[hs - 1]
            hs -= 1
        dn(0, hs, hp)
    for j in range(n_rev >> 1):                                                  # :210-214
        a[n_a - 1 - j], a[n_a - (n_rev - j)] = a[n_a - (n_rev - j)], a[n_a - 1 - j]
    if n_a > n_for + n_rev:                                                      # :215-218
        a[n_for:n_for + n_rev] = a[n_a - n_rev:n_a]
        n_a = n_for + n_rev
    a = a[:n_a]
    return np.array([p[0] for p in a], np.uint64), np.array([p[1] for p in a], np.uint64), rep


def head_of(S, c, flag, keyed):
    rank, _ = _rank(S, c["names"])
    lo, eq = _key(S, c["names"], c["qname"]) if keyed else (0, 0)
    mx, my = (c["mx"], c["my"]) if len(c["mx"]) else (Z1, Z1)
    return (c["hkey"], c["hval"], c["P"], c["hbits"], rank, c["lens"], mx, my, len(c["mx"]), c["qlen"], c["max_occ"], flag, lo, eq)


def dev_flag(flag, keyed):
    """what the launchers put into a job: the name bits travel only with a key"""
    return flag if keyed else flag & ~(NO_DIAG | NO_DUAL)


def run_seed(H, head, cap, lds_cap=4096):
    ax, ay, res = np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint64), np.zeros(4, np.int32)
    rc = H.emu_heap_seed(*head, lds_cap, ax, ay, cap, res)
    assert rc == 0, rc
    return ax[:res[0]], ay[:res[0]], int(res[1])


def run_window(H, head, cap, n_pre=0, px=None, py=None, seeded=1, lds_cap=4096, sort_cap=4096, nwv=4):
    ax, ay, res = np.zeros(cap + n_pre + 1, np.uint64), np.zeros(cap + n_pre + 1, np.uint64), np.zeros(4, np.int32)
    rc = H.emu_heap_window(*head, seeded, n_pre, px if n_pre else Z1, py if n_pre else Z1, lds_cap, sort_cap, nwv, ax, ay, cap + n_pre, res)
    assert rc == 0 and res[2] == 0, (rc, res)
    return ax[:res[0]], ay[:res[0]], int(res[1]), int(res[3])


def make_pre(rng, c, n_pre, ex):
    """handed-in anchors, sorted by x as stage 2 hands them in; some share x with seeded anchors, so that the union sort has ties of its own"""
    px = rng.integers(0, 1 << 20, n_pre).astype(np.uint64) | np.uint64(int(rng.integers(0, len(c["names"]))) << 32)
    if len(ex):
        for i in range(0, n_pre, 3):
            px[i] = ex[int(rng.integers(0, len(ex)))]
    px = np.sort(px)
    py = rng.integers(0, c["qlen"], n_pre).astype(np.uint64) | np.uint64(SPAN << 32)
    return px, py


def check_case(emus, refheap, c, flag=0, keyed=False, rng=None, n_pre=0, geom=None, tag=""):
    """the reference-driven list against the host restatement, seed_wave + ordering and win_seed_wave + ordering (with and without handed-in anchors)"""
    S, H = emus
    geom = geom or {}
    qn = c["qname"] if keyed else None
    ex, ey, erep = ref_heap_list(refheap, c, flag, qn)
    bx, _, _ = _collect_seed_hits(c, 0, None)
    cap = len(bx) + 16
    head = head_of(S, c, dev_flag(flag, keyed) | HEAP, keyed)
    # host restatement
    hx, hy, res = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(4, np.int32)
    assert H.emu_host_seed_heap(*head, 1 if keyed else 0, hx, hy, cap, res) == 0
    assert res[0] == len(ex) and res[1] == erep, (tag, res, len(ex), erep)
    assert np.array_equal(hx[:res[0]], ex) and np.array_equal(hy[:res[0]], ey), tag
    # seed_wave + seed_heap_kernel
    geom = dict(geom)
    sx, sy, srep = run_seed(H, head, cap, geom.pop("seed_lds", 4096))
    assert srep == erep and np.array_equal(sx, ex) and np.array_equal(sy, ey), tag
    # win_seed_wave + win_heap_kernel + the class's ordering
    wx, wy, wrep, road = run_window(H, head, cap, **geom)
    assert wrep == erep and np.array_equal(wx, ex) and np.array_equal(wy, ey), tag
    if n_pre:
        px, py = make_pre(rng, c, n_pre, ex)
        ox, oy = W.o_radix_sort_128x(np.concatenate([px, ex]), np.concatenate([py, ey]))          # src/map.c:818-833: the union, seeded part in heap order
        wx, wy, wrep, road = run_window(H, head, cap, n_pre, px, py, **geom)
        assert wrep == erep and np.array_equal(wx, ox) and np.array_equal(wy, oy), tag
        # no sequence: the handed-in anchors are chained as they are
        wx, wy, _, _ = run_window(H, head, cap, n_pre, px, py, seeded=0, **geom)
        assert np.array_equal(wx, px) and np.array_equal(wy, py), tag
    return ex, ey


# ------------------------------------------------------------------------------------------------
# 1. the heap primitives are the reference's own; random cases, most of them with tied x
# ------------------------------------------------------------------------------------------------
def test_host_heap_primitives_against_the_reference(emus, refheap):
    _, H = emus
    mk, dn = refheap
    rng = np.random.default_rng(11)
    for it in range(300):
        n = int(rng.integers(0, 140))
        x = rng.integers(0, 6 if it % 2 else 1 << 40, n + 1).astype(np.uint64)  # few distinct keys: ties everywhere
        y = np.arange(n + 1, dtype=np.uint64)
        a = np.stack([x, y], 1).copy()
        hx, hy = x.copy(), y.copy()
        mk(n, a.ctypes.data); H.emu_host_heapmake(n, hx, hy)
        assert np.array_equal(a[:n, 0], hx[:n]) and np.array_equal(a[:n, 1], hy[:n]), it
        if n:
            a[0, 0] = hx[0] = np.uint64(int(rng.integers(0, 8)))
            i0 = int(rng.integers(0, n))
            dn(i0, n, a.ctypes.data); H.emu_host_heapdown(i0, n, hx, hy)
            assert np.array_equal(a[:n, 0], hx[:n]) and np.array_equal(a[:n, 1], hy[:n]), it


@pytest.mark.parametrize("flag,keyed", [(0, False), (FOR_ONLY, False), (REV_ONLY, False), (NO_DIAG, True), (NO_DUAL, True), (NO_DIAG | NO_DUAL | FOR_ONLY, True),
                                        (NO_DIAG | NO_DUAL, False)])
def test_heap_order_random_cases(emus, refheap, flag, keyed):
    _, H = emus
    rng = np.random.default_rng(1000 + flag % 977 + keyed)
    events(H)
    n_tied = n_self = n_cases = 0
    for it in range(60):
        c = make_case(rng, ("self", "absent")[it % 2] if keyed else "absent", tie_p=0.0 if it % 5 == 4 else 0.45)
        ex, ey = check_case(emus, refheap, c, flag, keyed, rng, n_pre=int(rng.integers(1, 9)) if it % 2 else 0, tag=(flag, it))
        n_tied += has_tie(ex); n_cases += 1
        n_self += int(np.count_nonzero(ey & np.uint64(SEED_SELF)))
    ev = events(H)
    assert n_tied * 2 > n_cases, (n_tied, n_cases)                               # most cases have tied x ...
    assert ev[1] > 0 and ev[0] > 0                                               # ... and both roads ran
    if keyed and (flag & NO_DIAG):
        assert n_self > 0


# ------------------------------------------------------------------------------------------------
# 2. the smallest shapes that can go wrong
# ------------------------------------------------------------------------------------------------
def R(rid, pos, strand):
    return rid << 32 | pos << 1 | strand


def _distinct(n, strand_of=lambda i: 0, ref_strand_of=lambda i: 0, dup=()):
    """n matches with one occurrence each; the matches listed in dup repeat the key (and strand) of match 0: tied x"""
    minis, table = [], {}
    for i in range(n):
        k = 1000 + (0 if i in dup else i)
        minis.append((k, 30 + 7 * i, strand_of(0 if i in dup else i)))
        table.setdefault(k, [R(0, 5000 - 11 * i if i % 3 else 100 + 13 * i, ref_strand_of(i))])
    return minis, table


def test_smallest_shapes(emus, refheap):
    S, H = emus
    rng = np.random.default_rng(3)
    events(H)

    def run(minis, table, flag=0, expect_n=None, replay=None, **kw):
        events(H)
        c = craft(minis, table, **kw)
        ex, _ = check_case(emus, refheap, c, flag, False, rng, n_pre=3, tag=(minis[:3], flag))
        ev = events(H)
        if expect_n is not None:
            assert len(ex) == expect_n
        if replay is not None:
            assert (ev[1] > 0) == replay, ev
        return ex

    # no minimizers; minimizers that are all over-represented; one match; matches whose key is absent (n == 0 never enters the heap)
    run([], {}, expect_n=0, replay=False)
    run([(7, 40, 0), (8, 50, 1)], {7: [R(0, 10 * i, 0) for i in range(6)], 8: [R(0, 10 * i + 1, 1) for i in range(9)]}, expect_n=0, replay=False)
    run([(7, 40, 0)], {7: [R(0, 500, 0)]}, expect_n=1, replay=False)
    run([(7, 40, 0), (9, 60, 0)], {7: [R(0, 500, 0), R(0, 900, 1)]}, expect_n=2, replay=False)
    run([(9, 40, 0), (7, 44, 0), (9, 60, 1), (7, 70, 0)], {7: [R(0, 500, 0), R(0, 900, 1)]}, expect_n=4, replay=True)
    # two matches with identical lists: tied on every pop (adjacent: tandem seeds; apart: plain ones)
    lst = [R(0, 300, 0), R(0, 301, 0), R(1, 20, 1), R(1, 800, 0)]
    run([(7, 40, 0), (7, 55, 0)], {7: lst}, expect_n=8, replay=True)
    run([(7, 40, 1), (8, 47, 0), (7, 55, 1)], {7: lst, 8: [R(0, 301, 0)]}, expect_n=9, replay=True)
    # a list exhausted while others remain: the root is replaced by the last entry
    run([(7, 40, 0), (8, 47, 0), (9, 52, 0), (8, 66, 0)], {7: [R(0, 10, 0)], 8: [R(0, 20, 0), R(0, 30, 0), R(0, 40, 0), R(0, 50, 0), R(1, 5, 1)], 9: [R(0, 25, 0), R(1, 2, 0)]},
        expect_n=13, replay=True)
    # both strands of one reference position, reached by minimizers of both strands: equal x from different r
    run([(7, 40, 0), (7, 55, 1)], {7: [R(0, 300, 0), R(0, 300, 1)]}, expect_n=4, replay=True)
    # heap sizes at the tile borders, with and without tied x
    for n in (63, 64, 65, 130):
        run(*_distinct(n), expect_n=n, replay=False)
        run(*_distinct(n, dup=(n // 2, n - 1)), expect_n=n, replay=True)
    # all forward, all reverse, odd and even reverse counts (the reversal loop)
    for n_rev in (0, 1, 2, 5, 6):
        m, t = _distinct(9, strand_of=lambda i: 1 if i < n_rev else 0, dup=(3, 7) if n_rev in (0, 5) else ())
        run(m, t, expect_n=9)
    m, t = _distinct(8, strand_of=lambda i: 1, dup=(2, 5))
    run(m, t, expect_n=8, replay=True)
    # every anchor dropped by skip_seed, and some of them (the closing-up of :215-218)
    m, t = _distinct(12, strand_of=lambda i: i % 2, dup=(4, 6))
    n_fwd = sum(1 for k, _, s in m if s == 0)
    run(m, t, flag=FOR_ONLY, expect_n=n_fwd)
    run(m, t, flag=REV_ONLY, expect_n=12 - n_fwd)
    m, t = _distinct(10, strand_of=lambda i: 1, dup=(4, 6))
    run(m, t, flag=FOR_ONLY, expect_n=0, replay=False)
    m, t = _distinct(10, dup=(4, 6))
    run(m, t, flag=REV_ONLY, expect_n=0, replay=False)


@pytest.mark.parametrize("mode", ["self", "absent"])
@pytest.mark.parametrize("flag", [NO_DIAG, NO_DUAL, NO_DIAG | NO_DUAL | REV_ONLY])
def test_keyed_jobs_drop_and_mark_per_popped_entry(emus, refheap, mode, flag):
    rng = np.random.default_rng(77 + flag)
    n_drop = 0
    for it in range(20):
        c = make_case(rng, mode, tie_p=0.6)
        ex, ey = check_case(emus, refheap, c, flag, True, rng, n_pre=2, tag=(mode, flag, it))
        bx, _, _ = _collect_seed_hits(c, 0, None)
        n_drop += len(bx) - len(ex)
    if mode == "self":
        assert n_drop > 0


def test_size_classes_and_roads(emus, refheap):
    """a job of at most 256 anchors (win_small road), one of a few hundred (win_sort), and — the geometry shrunk through the emulator's parameters — jobs
    beyond the LDS class: sorted by the workgroup in global memory, the heap in global memory, and the workgroup road of win_bigsort_kernel for the union sort"""
    _, H = emus
    rng = np.random.default_rng(5)
    sizes = []
    for lo, hi, geom, want in [((20, 120), 256, None, (1, 0)),
                               ((260, 420), 1500, None, (1, 0)),
                               ((260, 420), 1500, dict(seed_lds=64), (1, 1)),                            # seed op beyond "LDS": global sort + global heap
                               ((260, 420), 1500, dict(seed_lds=64, lds_cap=128, sort_cap=128, nwv=4), (1, 1)),      # ... and the window op beyond "LDS" as well, the union on the workgroup road
                               ((260, 420), 1500, dict(lds_cap=4096, sort_cap=128, nwv=3), (1, 0))]:     # workgroup road for the union only (seeded part served before)
        events(H)
        for it in range(3):
            c = make_case(rng, tie_p=0.4, n_mini=lo, n_ctg=2, hit_p=0.6)
            ex, _ = check_case(emus, refheap, c, 0, False, rng, n_pre=5, geom=geom, tag=(lo, geom, it))
            assert lo[0] // 2 < len(ex) <= hi and has_tie(ex)
            sizes.append(len(ex))
            # the same geometry on a job without equal x: the sorted list is kept
            c = make_case(rng, tie_p=0.0, n_mini=lo, n_ctg=2, hit_p=0.6)
            ex, _ = check_case(emus, refheap, c, 0, False, rng, n_pre=5, geom=geom, tag=("free", lo, geom, it))
        ev = events(H)
        assert ev[0] > 0 and (ev[1] > 0) == bool(want[0]) and (ev[2] > 0) == bool(want[1]), (geom, ev)
    assert min(sizes) <= 256 < max(sizes)


# ------------------------------------------------------------------------------------------------
# 3. bit off: nothing changes   4. no equal x: both orders coincide
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag,keyed", [(0, False), (REV_ONLY, False), (NO_DIAG | NO_DUAL, True)])
def test_bit_off_is_the_radix_path(emus, flag, keyed):
    S, H = emus
    rng = np.random.default_rng(21 + flag % 977)
    events(H)
    n_tied = 0
    for it in range(30):
        c = make_case(rng, "self" if keyed else "absent")
        ex, ey, erep = _collect_seed_hits(c, flag, c["qname"] if keyed else None)
        n_tied += has_tie(ex)
        sx, sy = W.o_radix_sort_128x(ex, ey)                                    # src/map.c:252
        head = head_of(S, c, dev_flag(flag, keyed), keyed)
        cap = len(ex) + 16
        gx, gy, grep = run_seed(H, head, cap)
        assert grep == erep and np.array_equal(gx, sx) and np.array_equal(gy, sy), it
        for n_pre in (0, 4):
            px, py = make_pre(rng, c, n_pre, ex)
            ox, oy = (np.concatenate([px, sx]), np.concatenate([py, sy]))
            if n_pre:
                ox, oy = W.o_radix_sort_128x(ox, oy)                            # :833
            for geom in (dict(), dict(sort_cap=64, nwv=4)):
                wx, wy, wrep, _ = run_window(H, head, cap, n_pre, px, py, **geom)
                assert wrep == erep and np.array_equal(wx, ox) and np.array_equal(wy, oy), (it, n_pre, geom)
    assert n_tied > 10
    assert events(H) == [0, 0, 0, 0]                                             # nothing of the heap path ran


def test_without_equal_x_both_orders_coincide(emus):
    S, H = emus
    rng = np.random.default_rng(31)
    events(H)
    for it in range(30):
        c = make_case(rng, tie_p=0.0)
        for flag in (0, FOR_ONLY):
            ex, ey, _ = _collect_seed_hits(c, flag, None)
            assert not has_tie(ex)
            cap = len(ex) + 16
            rx, ry, rrep = run_seed(H, head_of(S, c, flag, False), cap)
            hx, hy, hrep = run_seed(H, head_of(S, c, flag | HEAP, False), cap)
            assert hrep == rrep and np.array_equal(hx, rx) and np.array_equal(hy, ry), it
            for geom in (dict(), dict(lds_cap=64, sort_cap=64, nwv=4)):
                a = run_window(H, head_of(S, c, flag, False), cap, **geom)
                b = run_window(H, head_of(S, c, flag | HEAP, False), cap, **geom)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (it, geom)
    ev = events(H)
    assert ev[1] == 0 and ev[2] == 0 and ev[0] > 0
