"""CPU: the cs:Z / MD:Z bodies (write_cs_core / write_MD_core, src/format.c:141-218) — the specification (csrc/cigar_cs.h) against the Python restatement of its
rules (cscases.restated), and the kernels of csrc/cs_kernel.h on the wavefront emulator (prefix, count pass, scan over jobs, write pass; one wavefront per job / one
per tile + combine; tile sizes 64 and the default; byte form and position form over wm_pack_codes data) against the specification, byte for byte, in all three
modes. The emulator's output pool has exactly the reported size plus a guard byte (tests/simt_emu/emu_cs.cpp)."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import extracases as X
import cscases as Q
from winnowmap_amd import build
from test_host_simd import random_alignment
from test_eqx_emu import pos_arrays

i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
i64p = np.ctypeslib.ndpointer(np.int64, flags="C")
ALL_SHORT, ALL_LONG, DEFAULT_LONG_MIN = 1 << 30, 1, 32768
ROUTES = [(ALL_SHORT, 64), (ALL_SHORT, Q.T), (ALL_LONG, 64), (ALL_LONG, Q.T), (DEFAULT_LONG_MIN, Q.T)]      # the four forced routes and the default
BIG = ("long_40k", "run_of_100000")


@pytest.fixture(scope="module")
def E():
    L = C.CDLL(build.build_emu_cs())
    L.emu_cs_spec.argtypes = [C.c_int, W.u32p, C.c_int, W.u8p, W.u8p, W.u8p]
    L.emu_cs_spec.restype = C.c_longlong
    L.emu_cs_bound.argtypes = [W.u32p, C.c_int]
    L.emu_cs_bound.restype = C.c_longlong
    L.emu_cs_check.argtypes = [C.c_int, W.u32p, C.c_int]
    L.emu_cs_batch.argtypes = [C.c_int, C.c_int, W.u32p, W.u32p, W.u32p, i32p, W.u8p, C.c_size_t, W.u32p, C.c_int, C.c_int, W.u8p, C.c_size_t, i32p]
    L.emu_cs_batch.restype = C.c_longlong
    L.emu_cs_batch_pos.argtypes = [C.c_int, C.c_int, i64p, i32p, i32p, i64p, W.u32p, i32p, W.u8p, C.c_size_t, W.u8p, C.c_size_t, W.u32p, C.c_int, C.c_int, W.u8p, C.c_size_t, i32p]
    L.emu_cs_batch_pos.restype = C.c_longlong
    return L


def spec(E, mode, cig, q, t):
    cg = np.ascontiguousarray(cig, np.uint32) if len(cig) else np.zeros(1, np.uint32)
    b = E.emu_cs_bound(cg, len(cig))
    assert b == Q.bound(cig)
    out = np.full(b + 1, 0xee, np.uint8)
    n = E.emu_cs_spec(mode, cg, len(cig), np.ascontiguousarray(q), np.ascontiguousarray(t), out)
    assert 0 <= n <= b and out[b] == 0xee
    return out[:n].tobytes()


@pytest.fixture(scope="module")
def CASES():
    """computed once: every byte-form case with what the restatement gives in the three modes"""
    cases = Q.make_cases() + Q.batch70() + [Q.long_40k()]
    return [(c, [Q.restated(m, c[1], c[2], c[3]) for m in Q.MODES]) for c in cases]


def run_bytes(E, mode, cases, long_min, tile, cap=None):
    q_off, t_off, cig_off, n_cig, seqs, cigs, ops = Q.pack(cases)
    bound = sum(Q.bound(c[1]) for c in cases)
    out = np.zeros(bound + 1, np.uint8); res = np.full((len(cases), 4), -7, np.int32)
    total = E.emu_cs_batch(mode, len(cases), q_off, t_off, cig_off, n_cig, seqs, len(seqs), cigs, long_min, tile, out, bound if cap is None else cap, res)
    return total, out, res


def check(cases, wants, total, out, res, tag):
    at = 0
    for i, (c, want) in enumerate(zip(cases, wants)):
        off, hi, n, pad = (int(v) for v in res[i])
        assert hi == 0 and pad == 0 and off == at, (c[0], tag, off, at)                      # back to back, in job order
        got = out[off:off + n].tobytes()
        assert got == want, (c[0], tag, got[:200], want[:200])
        at += n
    assert total == at


def test_the_case_list_is_what_the_issue_asks_for():
    cases = Q.make_cases()
    assert len(cases) > 70 and len(set(c[0] for c in cases)) == len(cases)
    assert len(Q.batch70()) == 70 and sum(int(w) >> 4 for w in Q.long_40k()[1] if int(w) & 0xf == 0) == 40000 and Q.T % 64 == 0


def test_specification_equals_the_restatement(E, CASES):
    for c, wants in CASES:
        for mode in Q.MODES:
            assert spec(E, mode, c[1], c[2], c[3]) == wants[mode], (c[0], mode)


def test_the_cases_pin_what_their_names_say(CASES):
    by = {c[0]: tuple(w.decode() for w in wants) for c, wants in CASES}
    assert by["single_M_all_match"][0] == ":100" and by["single_M_all_match"][2] == "100" and by["single_M_all_match"][1][0] == "=" and len(by["single_M_all_match"][1]) == 101
    assert by["single_M_all_mismatch"][0].count("*") == 70 and ":" not in by["single_M_all_mismatch"][0] and by["single_M_all_mismatch"][2].count("0") == 70
    assert by["single_M_one_mismatch_first_column"][0][0] == "*" and by["single_M_one_mismatch_first_column"][0].endswith(":99") and by["single_M_one_mismatch_first_column"][2][0] == "0"
    assert by["single_M_one_mismatch_last_column"][0].startswith(":99*") and by["single_M_one_mismatch_last_column"][2].startswith("99") and len(by["single_M_one_mismatch_last_column"][2]) == 3
    assert by["cs_flushes_at_an_op_boundary"] == (":10:10", by["cs_flushes_at_an_op_boundary"][1], "20") and by["cs_flushes_at_an_op_boundary"][1].count("=") == 2
    s = by["cs_flushes_at_an_op_boundary_under_eqx_ops"]
    assert s[0].startswith(":10*") and s[0].endswith(":9") and s[2].startswith("10") and s[2].endswith("9")
    s = by["X_op_over_equal_bases_and_EQ_op_over_unequal_ones"]
    assert s[0].startswith(":8:1*") and s[0].endswith(":3:5") and s[0].count("*") == 2
    s = by["md_mismatch_right_after_a_D"][2]
    assert s.startswith("5^") and s[4] == "0" and s.endswith("8") and len(s) == 7                          # 5^AC0T8
    s = by["md_zero_before_a_first_column_mismatch_and_between_adjacent_ones"][2]
    assert s[0] == "0" and s[2] == "0" and s[4] == "0" and s[6] == "7" and s[8] == "0" and s.endswith("18")
    assert by["md_trailing_run_of_0_not_printed"][2][:2] == "11" and len(by["md_trailing_run_of_0_not_printed"][2]) == 3
    assert by["md_trailing_D"][2].startswith("4") and by["md_trailing_D"][2][-4] == "^"
    assert by["only_I_and_D"][0][0] == "+" and by["only_I_and_D"][0][6] == "-" and by["only_I_and_D"][2].startswith("0^") and len(by["only_I_and_D"][2]) == 11
    assert by["empty_cigar_between_two_real_jobs"] == ("", "", "")
    assert "+-" in by["zero_length_M_I_D"][0] and by["zero_length_M_I_D"][0].endswith("-+") and by["zero_length_M_I_D"][2].startswith("20^5") and by["zero_length_M_I_D"][2].endswith("14^")
    assert by["N_against_N"] == (":40", "=" + by["N_against_N"][1][1:], "40") and by["N_against_N"][1][12:14] == "NN"
    assert "*n" in by["N_against_a_base"][0] and "N" in by["N_against_a_base"][2]
    assert "~" in by["intron_100000_on_a_tile_edge_64"][0] and "100000" in by["intron_100000_on_a_tile_edge_64"][0] and "~" not in by["intron_100000_on_a_tile_edge_64"][2]
    assert ":100000*" in by["run_of_100000"][0] and by["run_of_100000"][2].startswith("7") and "100000" in by["run_of_100000"][2]
    for e in Q.TILES:
        for w in (10, 100, 1000):
            s = by["run_%d_to_%d_completed_across_a_tile_edge_%d" % (w - 1, w, e)]
            assert (":%d*" % w) in s[0] and ("%d" % w) in s[2]
        s = by["run_spans_three_tiles_middle_one_without_a_break_%d" % e]
        assert (":%d*" % (e + 10)) in s[0]
        s = by["md_run_carried_across_I_%d" % e]
        assert s[2].startswith("1") and ("%d" % (2 * e - 2)) in s[2] and "+" in s[0]
        s = by["md_run_carried_across_an_op_boundary_on_a_tile_edge_%d" % e]
        assert s[0].startswith(":3*") and (":%d:%d:2*" % (e - 4, e)) in s[0] and ("%d" % (2 * e - 2)) in s[2]


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_emulated_kernels_equal_the_specification_on_every_named_case(E, CASES, long_min, tile, mode):
    pick = [(c, w) for c, w in CASES if c[0] not in BIG or tile == Q.T]            # (the two big ones at the default tile only: short, long and default routing)
    cases = [c for c, _ in pick]
    total, out, res = run_bytes(E, mode, cases, long_min, tile)
    check(cases, [w[mode] for _, w in pick], total, out, res, (mode, long_min, tile))


def test_the_default_routing_uses_both_classes(CASES):
    cols = {c[0]: Q.columns(Q.SHORT, c[1]) for c, _ in CASES}
    assert cols["long_40k"] >= DEFAULT_LONG_MIN and cols["run_of_100000"] >= DEFAULT_LONG_MIN and cols["mixed_shapes_mismatch_rate_0.1"] < DEFAULT_LONG_MIN


@pytest.mark.parametrize("mode", Q.MODES)
def test_a_pool_one_byte_too_small_reports_the_needed_size_and_writes_nothing(E, CASES, mode):
    pick = [(c, w) for c, w in CASES if c[0].startswith("cs_batch70")]
    cases = [c for c, _ in pick]
    needed = sum(len(w[mode]) for _, w in pick)
    total, out, res = run_bytes(E, mode, cases, ALL_SHORT, 64, cap=needed - 1)
    assert total == needed and not out.any()
    assert [int(r[2]) for r in res] == [len(w[mode]) for _, w in pick]             # res is already filled
    total, out, res = run_bytes(E, mode, cases, ALL_SHORT, 64, cap=needed)
    check(cases, [w[mode] for _, w in pick], total, out, res, "exact capacity")


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_300_random_alignments_equal_the_specification(E, long_min, tile, mode):
    rng = np.random.default_rng(13)
    cases = []
    for it in range(300):
        cig, q, t = random_alignment(rng, int(rng.integers(1, 60)), 0.0 if it % 3 else 0.02)
        cases.append(("random_%d" % it, Q.no_short_introns(cig), np.concatenate([q, np.full(16, 4, np.uint8)]), np.concatenate([t, np.full(16, 4, np.uint8)])))
    wants = [spec(E, mode, c[1], c[2], c[3]) for c in cases]
    for c, want in zip(cases, wants):
        assert Q.restated(mode, c[1], c[2], c[3]) == want, c[0]
    total, out, res = run_bytes(E, mode, cases, long_min, tile)
    check(cases, wants, total, out, res, (mode, long_min, tile))


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_position_form_over_packed_reads_and_nibbles_equals_the_specification(E, long_min, tile, mode):
    """extracases' position cases: forward and reverse strand, a query that starts in front of its strand (the other strand's tail, or N padding) and one that runs
    off the end of two-strand space (N), every target alignment mod 8"""
    P = X.make_pos_cases()
    qwin, qlen, qpos, tbase, cig_off, n_cig, reads, ref, cigs, ops, operands = pos_arrays(P)
    bound = sum(Q.bound(p[1]) for p in P)
    out = np.zeros(bound + 1, np.uint8); res = np.full((len(P), 4), -7, np.int32)
    total = E.emu_cs_batch_pos(mode, len(P), qwin, qlen, qpos, tbase, cig_off, n_cig, reads, len(reads), ref, len(ref), cigs, long_min, tile, out, bound, res)
    cases = [(p[0], p[1], q, t) for p, (q, t) in zip(P, operands)]
    wants = [Q.restated(mode, c[1], c[2], c[3]) for c in cases]
    assert any(b"N" in w or b"n" in w for w in wants)
    check(cases, wants, total, out, res, (mode, long_min, tile))


def test_the_specification_names_the_op_the_reference_asserts_against(E):
    cig = np.array([10 << 4, 3 << 4 | 4, 5 << 4], np.uint32)
    assert [E.emu_cs_check(m, cig, 3) for m in Q.MODES] == [1, 1, 1] and E.emu_cs_check(3, cig, 3) == -2
    cig = np.array([10 << 4, 1 << 4 | 3, 5 << 4], np.uint32)
    assert [E.emu_cs_check(m, cig, 3) for m in Q.MODES] == [1, 1, -1]
    q = np.zeros(40, np.uint8); out = np.zeros(100, np.uint8)
    assert E.emu_cs_spec(Q.SHORT, cig, 3, q, q, out) == -2 and not out.any()
    cig = np.array([10 << 4, 2 << 4 | 3, 5 << 4 | 7, 2 << 4 | 8], np.uint32)
    assert [E.emu_cs_check(m, cig, 4) for m in Q.MODES] == [-1, -1, -1]


def test_bytes_above_4_are_clamped_to_N(E):
    cig = np.array([4 << 4], np.uint32)
    q = np.array([0, 9, 4, 200] + [4] * 16, np.uint8); t = np.array([0, 4, 7, 1] + [4] * 16, np.uint8)
    assert [spec(E, m, cig, q, t) for m in Q.MODES] == [b":3*cn", b"=ANN*cn", b"3C"]
    assert [Q.restated(m, cig, q, t) for m in Q.MODES] == [b":3*cn", b"=ANN*cn", b"3C"]
