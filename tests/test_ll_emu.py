"""CPU: ksw_ll_i16 (src/ksw2_ll_sse.c:80-147) — the specification (csrc/ksw_ll.h, what the host mapper compiles) against the Python restatement of the striped machine
in position terms (llcases.restated) and, where oracle/_ref is built, against the reference itself; and the kernel of csrc/ll_kernel.h on the wavefront emulator
(register class and LDS class, under three settings of the class boundary, both read directions, byte form and position form over wm_pack_codes data and reference
nibbles) against the specification: score, qe and te, job for job."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import llcases as Q
from winnowmap_amd import build

i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
i64p = np.ctypeslib.ndpointer(np.int64, flags="C")
BOUNDARIES = (Q.REG_MAX_DEFAULT, 32, 0)          # the default; a lower boundary (jobs of 33..64 positions change class); every job in the LDS class


@pytest.fixture(scope="module")
def E():
    L = C.CDLL(build.build_emu_ll())
    L.emu_ll_spec.argtypes = [C.c_int, W.u8p, C.c_int, W.u8p, W.i8p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.emu_ll_batch.argtypes = [C.c_int, i64p, i64p, i32p, i32p, i32p, W.u8p, C.c_size_t, W.i8p, C.c_int, C.c_int, C.c_int, i32p]
    L.emu_ll_batch.restype = None
    L.emu_ll_batch_pos.argtypes = [C.c_int, i64p, i32p, i32p, i64p, i32p, i32p, i32p, W.u8p, C.c_size_t, W.u8p, C.c_size_t, W.i8p, C.c_int, C.c_int, C.c_int, i32p]
    L.emu_ll_batch_pos.restype = None
    return L


def mat_of(c):
    return Q.simple_mat(c["a"], c["b"], c["ambi"])


def spec(E, c, rev=False):
    q, t = (np.ascontiguousarray(c["q"][::-1]), np.ascontiguousarray(c["t"][::-1])) if rev else (c["q"], c["t"])
    qe, te = C.c_int(), C.c_int()
    s = E.emu_ll_spec(len(q), q, len(t), t, mat_of(c), c["gapo"], c["gape"], C.byref(qe), C.byref(te))
    return s, qe.value, te.value


def groups(cases):
    """the emulator entry points take one scoring per call, as the C ABI does"""
    g = {}
    for i, c in enumerate(cases):
        g.setdefault((c["a"], c["b"], c["ambi"], c["gapo"], c["gape"]), []).append(i)
    return g


def run_bytes(E, cases, step, reg_max):
    got = [None] * len(cases)
    for idx in groups(cases).values():
        part = [cases[i] for i in idx]
        q_off, t_off, ql, tl, st, seqs = Q.pack(part, step)
        out = np.full((len(part), 3), -9, np.int32)
        E.emu_ll_batch(len(part), q_off, t_off, ql, tl, st, seqs, len(seqs), mat_of(part[0]), part[0]["gapo"], part[0]["gape"], reg_max, out)
        for i, o in zip(idx, out):
            got[i] = tuple(int(v) for v in o)
    return got


def run_pos(E, cases, step, reg_max):
    got = [None] * len(cases)
    for idx in groups(cases).values():
        part = [cases[i] for i in idx]
        reads, ref, jobs = Q.pos_layout(part, step)
        j = np.array(jobs, np.int64)
        out = np.full((len(part), 3), -9, np.int32)
        E.emu_ll_batch_pos(len(part), np.ascontiguousarray(j[:, 0]), np.ascontiguousarray(j[:, 1], np.int32), np.ascontiguousarray(j[:, 2], np.int32),
                           np.ascontiguousarray(j[:, 3]), np.array([len(c["q"]) for c in part], np.int32), np.array([len(c["t"]) for c in part], np.int32),
                           np.full(len(part), step, np.int32), reads, len(reads), ref, len(ref), mat_of(part[0]), part[0]["gapo"], part[0]["gape"], reg_max, out)
        for i, o in zip(idx, out):
            got[i] = tuple(int(v) for v in o)
    return got


@pytest.fixture(scope="module")
def CASES(E):
    """computed once: the named cases with what the specification gives"""
    cases = Q.make_cases()
    return cases, [spec(E, c) for c in cases]


def test_the_case_list_is_what_the_issue_asks_for():
    cases = Q.make_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for ql in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513):
        assert "len_q%d_t64" % ql in names
    lens = {(len(c["q"]), len(c["t"])) for c in cases}
    assert {(1, 1), (64, 1), (64, 63), (64, 65), (65, 63), (65, 65)} <= lens
    # both sides of the class boundary, at its default and at the lower setting: padded lengths 64 | 72 and 32 | 40
    padded = {(len(c["q"]) + 7) // 8 * 8 for c in cases}
    assert {32, 40, 64, 72} <= padded and Q.REG_MAX_DEFAULT == 64 and 32 in BOUNDARIES
    assert any(c["gapo"] + c["gape"] == 127 for c in cases) and {(c["a"], c["b"], c["gapo"], c["gape"]) for c in cases} >= set(Q.SCORINGS)
    assert {c["ambi"] for c in cases if c["name"].startswith("ambiguous")} == {0, 1, 3}
    assert Q.E_CASES == []                                                  # (the search found none: llcases says why)


def test_the_restatement_equals_the_specification_and_the_reference(E, CASES):
    cases, want = CASES
    for c, w in zip(cases, want):
        assert Q.restated(c["q"], c["t"], mat_of(c), c["gapo"], c["gape"])[:3] == w, c["name"]
        assert W.o_ksw_ll(c["q"], c["t"], mat_of(c), c["gapo"], c["gape"]) == w, c["name"]
        if W.have_ref():
            assert W.r_ksw_ll(c["q"], c["t"], mat_of(c), c["gapo"], c["gape"]) == w, c["name"]
    for c in Q.random_jobs(150, 120, 11):
        assert Q.restated(c["q"], c["t"], mat_of(c), c["gapo"], c["gape"])[:3] == spec(E, c), c["name"]


def test_the_cases_pin_what_their_names_say(E, CASES):
    cases, want = CASES
    by = {c["name"]: (c, w) for c, w in zip(cases, want)}

    def full(name):
        c = by[name][0]
        return Q.restated(c["q"], c["t"], mat_of(c), c["gapo"], c["gape"])
    for ql in (9, 17, 65, 513):                                             # the best cell on a pad slot: 7 pads behind a length = 1 (mod 8)
        c, (s, qe, te) = by["pad_slot_q%d" % ql]
        assert s == 2 * ql and qe == ql + 6 and qe >= len(c["q"]) and te == 5 + ql - 1 + 7
    s, qe, te, reach, rows = full("tie_qe_tandem")
    assert reach == [10, 21] and qe == 10 and by["tie_qe_tandem"][1] == (22, 10, 10)        # the striped order does not pick the larger position
    s, qe, te, reach, rows = full("tie_te_periodic")
    # every copy's last row reaches the score (and so do the rows behind a copy, on the 5 pad slots): te is the last of them
    assert {10, 21, 32} <= set(rows) and len(rows) > 3 and rows[-1] == 32 and by["tie_te_periodic"][1] == (22, 10, 32)
    assert by["all_zero_q20_t30"][1] == (0, 23, 29) and by["all_zero_q64_t1"][1] == (0, 63, 0)      # (0, n - 1, tlen - 1)
    assert by["saturated_900_a40"][1][0] == 32767 and by["one_below_saturation_762_a43"][1] == (32766, 761, 761)
    assert len({by["ambiguous_sc%d" % a][1] for a in (0, 1, 3)}) == 3                         # the ambiguity score matters in each
    # E opened from the corrected H is another machine, though not on these inputs (llcases.E_CASES): the restatement can at least be asked
    c = by["scoring_2_4_4_2_q150"][0]
    assert Q.restated(c["q"], c["t"], mat_of(c), 4, 2, e_from_corrected=True)[0] == by["scoring_2_4_4_2_q150"][1][0]


@pytest.mark.parametrize("reg_max", BOUNDARIES)
@pytest.mark.parametrize("step", [1, -1])
def test_the_emulated_kernel_equals_the_specification_on_every_named_case(E, CASES, step, reg_max):
    cases, want = CASES
    got = run_bytes(E, cases, step, reg_max)
    for c, w, g in zip(cases, want, got):
        assert g == w, (c["name"], step, reg_max, g, w)


@pytest.mark.parametrize("reg_max", [Q.REG_MAX_DEFAULT, 32])
@pytest.mark.parametrize("step", [1, -1])
def test_the_position_form_over_packed_reads_and_reference_nibbles(E, CASES, step, reg_max):
    cases, want = CASES
    cases = [c for c in cases if len(c["q"]) <= 520]
    got = run_pos(E, cases, step, reg_max)
    for c, g in zip(cases, got):
        assert g == spec(E, c, rev=step < 0), (c["name"], step, reg_max, g)          # (step -1 reads the stored operands back to front: another job)


def test_2000_random_jobs_up_to_600_x_600(E):
    jobs = Q.random_jobs(2000, 600, 77)
    want = [spec(E, c) for c in jobs]
    assert sum(1 for c, w in zip(jobs, want) if w[1] >= len(c["q"])) > 50           # qe on a pad slot is common
    got = run_bytes(E, jobs, 1, Q.REG_MAX_DEFAULT)
    bad = [(c["name"], g, w) for c, g, w in zip(jobs, got, want) if g != w]
    assert not bad, bad[:5]
    got = run_bytes(E, jobs[:300], -1, 0)
    bad = [(c["name"], g, w) for c, g, w in zip(jobs, got, want) if g != w]
    assert not bad, bad[:5]


def test_one_5000_x_5000_job_in_the_lds_class(E):
    """map-ont's largest inversion test: 79 passes, each handing its last column to the next through the in-place LDS rows"""
    rng = np.random.default_rng(5)
    q = rng.integers(0, 4, 5000).astype(np.uint8)
    c = Q.case("big", q, Q._related(rng, q, 5000, 0.1, 0.04))
    assert run_bytes(E, [c], 1, Q.REG_MAX_DEFAULT)[0] == spec(E, c)
