"""CPU: the fold of mm_update_extra's scan (csrc/extra_kernel.h; src/align.c:240-286) on the wavefront emulator — prefix pass, both classes (one wavefront
per job / one per tile + combine), tile sizes 64 and the default, byte form and position form over wm_pack_codes data — against wm_extra_walk
(csrc/cigar_walk.h, through the harness's generic walk) field by field, and against the reference's own mm_update_extra where oracle/_ref is built."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import extracases as X
from winnowmap_amd import build
from test_host_simd import random_alignment

i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
i64p = np.ctypeslib.ndpointer(np.int64, flags="C")
ALL_SHORT, ALL_LONG = 1 << 30, 1               # long_min_cols that force either class (a job without columns has no tiles: it is short by definition)
ROUTES = [(ALL_SHORT, 64), (ALL_SHORT, X.T), (ALL_LONG, 64), (ALL_LONG, X.T)]


@pytest.fixture(scope="module")
def E():
    L = C.CDLL(build.build_emu_extra())
    L.emu_extra_compose.argtypes = [i32p, i32p, i32p]
    L.emu_extra_wave_fold.argtypes = [i32p, i32p]
    L.emu_extra_batch.argtypes = [C.c_int, i32p, W.u32p, W.u32p, W.u32p, i32p, W.u8p, C.c_size_t, W.u32p, C.c_size_t, C.c_int, C.c_int, i32p, i32p]
    L.emu_extra_batch_pos.argtypes = [C.c_int, i32p, i64p, i32p, i32p, i64p, W.u32p, i32p, W.u8p, C.c_size_t, W.u8p, C.c_size_t, W.u32p, C.c_size_t,
                                      C.c_int, C.c_int, i32p, i32p]
    return L


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    L.h_extra_walk_both.argtypes = [C.c_void_p, C.c_void_p, W.u32p, C.c_int] + [C.c_int] * 5 + [i32p, i32p]
    return L


def walk(H, cig, q, t, sc):
    """wm_extra_walk: { dp_max, mlen, blen, n_ambi, qoff, toff }"""
    f, g = np.zeros(6, np.int32), np.zeros(6, np.int32)
    cg = np.ascontiguousarray(cig, np.uint32) if len(cig) else np.zeros(1, np.uint32)
    H.h_extra_walk_both(q.ctypes.data, t.ctypes.data, cg, len(cig), *[int(v) for v in sc], f, g)
    return g


def pack(cases):
    """cases of one score -> the arrays of a byte-form call"""
    q_off, t_off, cig_off, n_cig, seqs, cigs = [], [], [], [], [], []
    at = ops = 0
    for _, cig, q, t, _ in cases:
        q_off.append(at); seqs.append(q); at += len(q)
        t_off.append(at); seqs.append(t); at += len(t)
        cig_off.append(ops); n_cig.append(len(cig)); cigs.append(cig); ops += len(cig)
    cigs = np.concatenate(cigs + [np.zeros(1, np.uint32)]).astype(np.uint32)
    return (np.array(q_off, np.uint32), np.array(t_off, np.uint32), np.array(cig_off, np.uint32), np.array(n_cig, np.int32),
            np.ascontiguousarray(np.concatenate(seqs)), cigs, ops)


def run_bytes(E, cases, long_min, tile):
    """all cases share one score"""
    sc = np.array(cases[0][4], np.int32)
    q_off, t_off, cig_off, n_cig, seqs, cigs, ops = pack(cases)
    out = np.full((len(cases), 6), -7, np.int32); n_long = np.zeros(1, np.int32)
    assert E.emu_extra_batch(len(cases), sc, q_off, t_off, cig_off, n_cig, seqs, len(seqs), cigs, ops, long_min, tile, out, n_long) == 0
    return out, int(n_long[0])


def by_score(cases):
    groups = {}
    for c in cases:
        groups.setdefault(tuple(c[4]), []).append(c)
    return list(groups.values())


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_every_named_case_equals_wm_extra_walk(E, H, long_min, tile):
    n = 0
    for group in by_score(X.make_cases() + X.batch70()):
        out, n_long = run_bytes(E, group, long_min, tile)
        with_cols = sum(1 for c in group if any((int(w) & 0xf) <= 2 and ((int(w) & 0xf) != 0 or int(w) >> 4) for w in c[1]))
        assert n_long == (with_cols if long_min == ALL_LONG else 0)
        for c, got in zip(group, out):
            want = walk(H, c[1], c[2], c[3], c[4])
            assert np.array_equal(got, want), (c[0], long_min, tile, got, want)
            n += 1
    assert n > 130


def test_the_cases_pin_what_their_names_say(H):
    """all mismatches give dp_max 0, the exact-zero cases reach s == 0 without a clamp below, the maximum sits where the name puts it"""
    by = {c[0]: c for c in X.make_cases()}
    assert walk(H, *by["all_mismatches"][1:])[0] == 0
    assert walk(H, *by["all_matches"][1:])[0] == 2 * (X.T + 70)
    assert walk(H, *by["max_on_first_column"][1:])[0] == 2 and walk(H, *by["max_on_last_column"][1:])[0] == 2
    assert walk(H, *by["max_attained_twice"][1:])[0] == 4
    assert walk(H, *by["D_5000_with_N_in_the_deleted_target"][1:])[3] == 9 and walk(H, *by["I_300_with_N_in_the_query"][1:])[3] == 7
    assert len(X.batch70()) == 70 and X.T % 64 == 0


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_300_random_alignments_equal_wm_extra_walk(E, H, long_min, tile):
    rng = np.random.default_rng(11)
    for score in ((2, -4, -1, 4, 2), (1, -9, -2, 16, 2), (5, -4, 0, 24, 1)):
        cases = []
        for it in range(100):
            cig, q, t = random_alignment(rng, int(rng.integers(1, 60)), 0.0 if it % 3 else 0.02)
            cases.append(("random_%d" % it, cig, np.concatenate([q, np.full(16, 4, np.uint8)]), np.concatenate([t, np.full(16, 4, np.uint8)]), score))
        out, _ = run_bytes(E, cases, long_min, tile)
        for c, got in zip(cases, out):
            want = walk(H, c[1], c[2], c[3], c[4])
            assert np.array_equal(got, want), (c[0], score, long_min, tile, got, want)


def pos_arrays(P):
    """position cases -> one read buffer / one reference buffer behind leads that are no multiple of the word sizes, and the expected operands"""
    reads = [np.full(37, 4, np.uint8)]; ref = [np.full(13, 4, np.uint8)]
    qwin, qlen, qpos, tbase, cig_off, n_cig, cigs, want_ops = [], [], [], [], [], [], [], []
    rn, fn, ops = 37, 13, 0
    for name, cig, read, q_pos, contig, t_pos, score in P:
        qwin.append(rn); qlen.append(len(read)); qpos.append(q_pos); reads.append(read); rn += len(read)
        tbase.append(fn + t_pos); ref.append(contig); fn += len(contig)
        cig_off.append(ops); n_cig.append(len(cig)); cigs.append(cig); ops += len(cig)
        ql = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 1)); tl = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 2, 3))
        want_ops.append((np.concatenate([X.two_strand(read, q_pos, ql), np.full(16, 4, np.uint8)]), np.concatenate([contig[t_pos:t_pos + tl], np.full(16, 4, np.uint8)])))
    return (np.array(qwin, np.int64), np.array(qlen, np.int32), np.array(qpos, np.int32), np.array(tbase, np.int64), np.array(cig_off, np.uint32),
            np.array(n_cig, np.int32), np.ascontiguousarray(np.concatenate(reads)), np.ascontiguousarray(np.concatenate(ref)),
            np.concatenate(cigs).astype(np.uint32), ops, want_ops)


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_position_form_over_packed_reads_and_nibbles_equals_wm_extra_walk(E, H, long_min, tile):
    P = X.make_pos_cases()
    for score in sorted(set(tuple(p[6]) for p in P)):
        G = [p for p in P if tuple(p[6]) == score]
        qwin, qlen, qpos, tbase, cig_off, n_cig, reads, ref, cigs, ops, want_ops = pos_arrays(G)
        out = np.full((len(G), 6), -7, np.int32); n_long = np.zeros(1, np.int32)
        assert E.emu_extra_batch_pos(len(G), np.array(score, np.int32), qwin, qlen, qpos, tbase, cig_off, n_cig, reads, len(reads), ref, len(ref), cigs, ops,
                                     long_min, tile, out, n_long) == 0
        for p, (q, t), got in zip(G, want_ops, out):
            want = walk(H, p[1], q, t, score)
            assert np.array_equal(got, want), (p[0], long_min, tile, got, want)


@pytest.mark.skipif(not W.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("long_min,tile", [(ALL_SHORT, X.T), (ALL_LONG, 64)])
def test_final_cigars_equal_the_references_own_mm_update_extra(E, long_min, tile):
    """the raw alignment goes through the reference's mm_update_extra (with its mm_fix_cigar, rev = 0); the kernels get the CIGAR it leaves and the
    sequences shifted by its qs / rs, and must give its blen, mlen, n_ambi, dp_max"""
    cases, wants = X.through_the_reference(W.ref(), X.raw_alignments_for_the_reference())
    assert len(cases) > 250
    for score in sorted(set(c[4] for c in cases)):
        G = [(c, w) for c, w in zip(cases, wants) if c[4] == score]
        out, _ = run_bytes(E, [c for c, _ in G], long_min, tile)
        for (c, w), got in zip(G, out):
            assert (int(got[2]), int(got[1]), int(got[3]), int(got[0])) == w, (c[0], score, got, w)


def compose(L, R):
    """the four-line composition, restated: left, then right"""
    a1, b1, m1, c1 = L; a2, b2, m2, c2 = R
    return (a1 + a2, max(b1 + a2, b2), max(m1, a1 + m2), max(c1, b1 + m2, c2))


def run_of(ds):
    """the tuple of a run of elements, from its definition: s_in -> (max(s_in + a, b), max(s_in + m, c))"""
    s = pk = 0; tot = 0; m = -(1 << 30)
    for d in ds:
        tot += d; m = max(m, tot); s = max(0, s + d); pk = max(pk, s)
    return (tot, s, m, pk)


def test_the_operator_is_associative_and_is_what_the_kernels_compile(E):
    rng = np.random.default_rng(5)
    ident = (0, 0, -(1 << 30), 0)
    for it in range(1000):
        runs = [[int(d) for d in rng.integers(-9, 6, int(rng.integers(0, 12)))] for _ in range(3)]
        x, y, z = (run_of(r) for r in runs)
        assert compose(compose(x, y), z) == compose(x, compose(y, z)) == run_of(runs[0] + runs[1] + runs[2]), (it, runs)
        assert compose(ident, x) == x == compose(x, ident)
        out = np.zeros(4, np.int32)
        E.emu_extra_compose(np.array(x, np.int32), np.array(y, np.int32), out)
        assert tuple(int(v) for v in out) == compose(x, y)
    # not commutative: the ordered wave reduction must equal the left-to-right fold of its 64 tuples (and differs from the reversed one)
    n_asym = 0
    for it in range(50):
        tup = [run_of([int(d) for d in rng.integers(-9, 6, int(rng.integers(0, 5)))]) for _ in range(64)]
        acc = ident
        for t in tup:
            acc = compose(acc, t)
        rev = ident
        for t in tup[::-1]:
            rev = compose(rev, t)
        out = np.zeros(4, np.int32)
        E.emu_extra_wave_fold(np.array(tup, np.int32).reshape(-1), out)
        assert tuple(int(v) for v in out) == acc, (it, out, acc)
        n_asym += acc != rev
    assert n_asym > 25
