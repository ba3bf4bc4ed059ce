"""The batching hub on its own (winnowmap_amd/csrc/host/wm_fiber.h), on the CPU: tests/host_harness/harness.cpp: wmh_hub_selftest runs fibers that file one request
of every kind against device ops that only record what they are handed, and checks
  * that every filed request reaches exactly one batch call of the right kind (the three alignment queues all reach ksw_batch; under splice everything goes through
    OP_KSW to exts2_batch),
  * that a fiber resumes only when ALL the operations it waited for have returned (ksw() over normal + heavy + huge units, fix_extra() with both lists, with extras
    only, with nothing),
  * that a request over max_sw_mat never reaches the ops and comes back z-dropped with score -0x40000000 and no CIGAR,
  * n_reqs[op] / n_batches[op] per operation, and that the run ends at all (the drain rule),
  * that a batch call which throws still releases its waiters and leaves a message in the call's ErrorSink,
  * the scheduling defaults against a literal 12 x 4 table, and the four WM_<STEM>_* variables of every operation.
The self-test prints the failed condition and returns minus its line."""
import ctypes as C
import os

import pytest

from winnowmap_amd import build

STEMS = ("SKETCH", "SEED", "CHAIN", "KSW", "KSWH", "KSWX", "WINDOW", "WINDOWB", "EXTRA", "FIX", "EQX", "CS")
KNOBS = ("MIN_MORE", "MAX", "MIN_BATCH", "MAX_WAIT_MS")


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    L.wmh_hub_selftest.argtypes = [C.c_int, C.c_int, C.c_int]
    L.wmh_hub_selftest.restype = C.c_int
    return L


@pytest.fixture()
def plain_env(monkeypatch):
    """the defaults are what is compared: nothing of the hub's environment may be set by the caller"""
    for s in STEMS:
        for k in KNOBS:
            monkeypatch.delenv("WM_%s_%s" % (s, k), raising=False)
    for v in ("WM_KSW_HEAVY_UNITS", "WM_KSW_HUGE_UNITS", "WM_TRACE"):
        monkeypatch.delenv(v, raising=False)
    assert not any(k.startswith("WM_") and k.endswith(KNOBS) for k in os.environ)


@pytest.mark.parametrize("splice", [0, 1])
@pytest.mark.parametrize("n_threads", [1, 2, 4])
def test_hub_selftest(H, plain_env, n_threads, splice):
    assert H.wmh_hub_selftest(n_threads, 64, splice) == 0
