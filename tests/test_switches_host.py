"""CPU: the host mapper over the oracle's operations with ALL FIVE opt-in switches on (wm_set_fix_device, wm_set_extra_device, wm_set_eqx_device, wm_set_cs_device,
wm_set_ll_device; each request served here by the default DeviceOps::*_batch, i.e. the host forms behind the batching hub) against the same mapper with all five off,
on the two inputs that file ksw_ll_i16 jobs (the inversion reads and the splice set of tests/test_ll_gpu.py), under CIGAR with --eqx, --cs, --eqx --cs and --eqx --MD,
with 1 and 4 hub threads: the same hits, CIGARs, first-hit table and text, and every pass that the flags and the input call for did defer its requests."""
import ctypes as C
import os
import tempfile
import numpy as np
import pytest
import wmtest as W
from winnowmap_amd import build
from test_ll_gpu import inversion_input, splice_input

SWITCHES = ("fix", "extra", "eqx", "cs", "ll")
F_CIGAR, F_CG, F_CS, F_MD, F_EQX = 0x4, 0x20, 0x40, 0x1000000, 0x4000000
FLAGS = {"eqx": F_EQX, "cs": F_CS, "eqx_cs": F_EQX | F_CS, "eqx_md": F_EQX | F_MD}


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    L.h_index_build.restype = C.c_void_p
    L.h_index_build.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.h_map_many.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.POINTER(C.c_char_p), W.i32p, C.c_int, W.i32p, C.c_int, C.POINTER(C.c_int64), W.u32p, C.c_int64, C.POINTER(C.c_int64)]
    L.h_map_text.restype = C.c_int64
    L.h_map_text.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), W.i32p, C.c_int, C.c_char_p, C.c_int64]
    for s in SWITCHES:
        f = getattr(L, "wm_set_%s_device" % s)
        f.argtypes = [C.c_int]; f.restype = None
        g = getattr(L, "wm_%s_stats" % s)
        g.argtypes = [W.u64p, C.c_int]; g.restype = None
    return L


def set_all(H, on):
    for s in SWITCHES:
        getattr(H, "wm_set_%s_device" % s)(on)


def deferred(H, reset=False):
    """regions / jobs deferred per switch (the first counter of every account)"""
    out = {}
    for s in SWITCHES:
        a = np.zeros(8, np.uint64)
        getattr(H, "wm_%s_stats" % s)(a, 1 if reset else 0)
        out[s] = int(a[0])
    return out


@pytest.fixture(autouse=True)
def switches_back(H):
    keys = ["WM_%s_DEV" % s.upper() for s in SWITCHES]
    saved = {k: os.environ.pop(k, None) for k in keys}
    set_all(H, -1)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        set_all(H, -1)
        deferred(H, True)


@pytest.fixture(scope="module")
def INPUTS(H):
    """computed once: both inputs with their index"""
    tmp = tempfile.mkdtemp()
    made = {}
    for name, make in (("inversion", inversion_input), ("splice", splice_input)):
        preset, fa, k, w, reads = make(tmp)
        made[name] = dict(preset=preset, reads=reads, h=H.h_index_build(fa.encode(), b"", k, w, 4))
        assert made[name]["h"]
    return made


def map_all(H, run, flag, threads):
    """(hits, CIGARs, first) of h_map_many and the text of h_map_text"""
    reads = run["reads"]
    n = len(reads)
    seqs = (C.c_char_p * n)(*reads)
    lens = np.array([len(r) for r in reads], np.int32)
    ho = np.zeros(16 * 1024, np.int32); co = np.zeros(4000000, np.uint32); hf = (C.c_int64 * (n + 1))(); nc = C.c_int64()
    nh = H.h_map_many(run["h"], run["preset"].encode(), flag, n, seqs, lens, threads, ho, 1024, hf, co, len(co), C.byref(nc))
    assert nh > 0 and nc.value <= len(co)
    names = (C.c_char_p * n)(*[b"read%d" % i for i in range(n)])
    buf = C.create_string_buffer(64 << 20)
    m = H.h_map_text(run["h"], run["preset"].encode(), flag, n, names, seqs, lens, threads, buf, len(buf))
    assert m > 0
    return ho[:16 * nh].reshape(-1, 16).copy(), co[:nc.value].copy(), np.array(list(hf), np.int64), buf.raw[:m]


@pytest.fixture(scope="module")
def OFF(H, INPUTS):
    """computed once per (input, flags): the run with all five switches off (2 hub threads), and that it filed nothing"""
    made = {}

    def get(name, fl):
        if (name, fl) not in made:
            set_all(H, 0)
            deferred(H, True)
            made[name, fl] = map_all(H, INPUTS[name], F_CIGAR | F_CG | FLAGS[fl], 2)
            assert not any(deferred(H).values())
        return made[name, fl]
    return get


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("fl", sorted(FLAGS))
@pytest.mark.parametrize("name", ["inversion", "splice"])
def test_all_five_switches_on_give_the_hits_cigars_first_and_text_of_all_five_off(H, INPUTS, OFF, name, fl, threads):
    hits0, cigs0, first0, text0 = OFF(name, fl)
    set_all(H, 1)
    deferred(H, True)
    hits1, cigs1, first1, text1 = map_all(H, INPUTS[name], F_CIGAR | F_CG | FLAGS[fl], threads)
    d = deferred(H)
    assert np.array_equal(hits1, hits0) and np.array_equal(cigs1, cigs0) and np.array_equal(first1, first0)
    assert text1 == text0
    # what the flags ask for is in the output at all
    flag = FLAGS[fl]
    assert (b"\tcs:Z:" in text1) == bool(flag & F_CS) and (b"\tMD:Z:" in text1) == bool(flag & F_MD)
    assert bool(((cigs1 & 0xf) == 8).any()) == bool(flag & F_EQX) and (not flag & F_EQX or not ((cigs1 & 0xf) == 0).any())
    # every pass with something to do deferred it; a pass whose flag is not set filed nothing
    assert d["ll"] > 0 and d["fix"] > 0, d
    assert (d["eqx"] > 0) == bool(flag & F_EQX) and (d["cs"] > 0) == bool(flag & (F_CS | F_MD)), (fl, d)
