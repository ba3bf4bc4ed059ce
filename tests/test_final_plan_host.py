"""The batch planner of the final-CIGAR device calls on its own (winnowmap_amd/csrc/host/wm_final_plan.h), on the CPU: tests/host_harness/harness.cpp:
wmh_final_plan_selftest plans small batches with a recorder in place of the library's error function and a measure that only adds up M / I / D lengths, and compares
with literal tables
  * the split into the short and the long class at the threshold (columns 0, 127, 128, 129, 64 at long_min = 128, tiles of 64; long_min = 0), tile0, the tile and
    job maps, and the prefix slots for one and for two slots per job, also for two jobs on one CIGAR range,
  * every accepted edge of the operand rules (two-strand position -16, 2 L + 16, the contig's end, the end of the resident reads, the end of seqs, an empty CIGAR
    with nonsense positions) and the refusal one step past each, with WM_EINVAL, the job named, and nothing planned behind it,
  * that a refusal of the pass's own measure comes after the CIGAR range check and before the operand checks,
  * that 2^28 tiles are refused before a job's tiles go into the map.
The self-test prints the condition that failed and returns minus its line."""
import ctypes as C

from winnowmap_amd import build


def test_final_plan_selftest():
    L = C.CDLL(build.build_harness())
    L.wmh_final_plan_selftest.argtypes = []
    L.wmh_final_plan_selftest.restype = C.c_int
    assert L.wmh_final_plan_selftest() == 0
