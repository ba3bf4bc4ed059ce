"""The two seeding bodies share their probe, kept count and tile expansion (winnowmap_amd/csrc/seedchain_kernel.h: seed_probe, seed_kept, seed_expand_tile); what they
keep to themselves — the caching between the passes, the pool allocation, the slot bound, the two rep_len forms — must not show: the same job through seed_wave and
through win_seed_wave (no handed-in anchors) gives the same anchors in the same order, the same count and the same rep_len. On the host wavefront emulator, with the
fixtures of test_selfmap_emu.py, whose restated collect_seed_hits is a third opinion on every job."""
import numpy as np
import pytest
from test_selfmap_emu import emus, _make_case, _rank, _key, _collect_seed_hits, NO_DIAG, NO_DUAL, FOR_ONLY, REV_ONLY, SEED_TANDEM  # noqa: F401 (emus: the fixture)

ALL = NO_DIAG | NO_DUAL | FOR_ONLY | REV_ONLY
# (flag, with a name key): each of the four filter bits, all of them, none; without a key the two name bits do not travel (src/map.c:135), as the host strips them
MODES = [(0, True), (NO_DIAG, True), (NO_DUAL, True), (FOR_ONLY, True), (REV_ONLY, True), (ALL, True), (0, False), (FOR_ONLY, False), (REV_ONLY, False), (FOR_ONLY | REV_ONLY, False)]
JOBS = ["n0", "n1", "n64", "n65", "whole", "all_dropped", "tandem_63_64"]


def _cut(c, n):
    return dict(c, mx=c["mx"][:n].copy(), my=c["my"][:n].copy())


@pytest.fixture(scope="module")
def jobs():
    """one index and query per job; the minimizer lists are cut to the tile edge, reduced to over-represented keys, or given a tandem pair across the edge"""
    rng = np.random.default_rng(41)
    c = _make_case(rng, "dup", max_occ=24)
    while len(c["mx"]) < 100:                          # (more than one tile, and room behind the edge)
        c = _make_case(rng, "dup", max_occ=24)
    out = {"n0": _cut(c, 0), "n1": _cut(c, 1), "n64": _cut(c, 64), "n65": _cut(c, 65), "whole": c}
    # every minimizer at or above max_occ: the keys that have occurrences, with max_occ = 1 — nothing is emitted, rep_len alone speaks
    has = np.array([c["table"][int(x) >> 8][1] >= 1 for x in c["mx"]])
    out["all_dropped"] = dict(c, mx=c["mx"][has].copy(), my=c["my"][has].copy(), max_occ=1)
    assert len(out["all_dropped"]["mx"]) > 64
    # minimizers 63 and 64 share a key that is expanded (0 < occurrences < max_occ); their other neighbours do not, so the bit can only come across the tile edge
    t = dict(c, mx=c["mx"].copy())
    key = next(k for k, (_, cnt) in c["table"].items() if 0 < cnt < c["max_occ"] and all(int(t["mx"][i]) >> 8 != k for i in (62, 65)))
    t["mx"][63] = t["mx"][64] = np.uint64(key << 8 | 15)
    out["tandem_63_64"] = t
    return out


def _both(S, c, flag, keyed, cap):
    rank, _ = _rank(S, c["names"])
    lo, eq = _key(S, c["names"], c["qname"]) if keyed else (0, 0)
    n = len(c["mx"])
    mx, my = (c["mx"], c["my"]) if n else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    head = (c["hkey"], c["hval"], c["P"], c["hbits"], rank, c["lens"], mx, my, n, c["qlen"], c["max_occ"], flag, lo, eq)
    ax, ay, ares = np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint64), np.zeros(3, np.int32)
    S.emu_self_seed(*head, ax, ay, cap, ares)
    full = sum(cnt for _, cnt in c["table"].values()) * 2 + 80          # (the window body is handed a pool that holds whatever the job can emit)
    wx, wy, wres = np.zeros(full, np.uint64), np.zeros(full, np.uint64), np.zeros(3, np.int32)
    S.emu_self_win_seed(*head, 0, np.zeros(1, np.uint64), np.zeros(1, np.uint64), wx, wy, full, wres)
    assert wres[2] == 0
    return (ax, ay, ares), (wx, wy, wres)


@pytest.mark.parametrize("flag,keyed", MODES)
@pytest.mark.parametrize("job", JOBS)
def test_both_seed_bodies_give_the_same_anchors(emus, jobs, job, flag, keyed):
    S, _ = emus
    c = jobs[job]
    ex, ey, erep = _collect_seed_hits(c, flag, c["qname"] if keyed else None)
    (ax, ay, ares), (wx, wy, wres) = _both(S, c, flag, keyed, len(ex) + 16)
    n = int(ares[0])
    assert n == int(wres[0]) and int(ares[1]) == int(wres[1])
    assert np.array_equal(ax[:n], wx[:n]) and np.array_equal(ay[:n], wy[:n])          # the same anchors in the same (minimizer) order
    assert n == len(ex) and int(ares[1]) == erep and np.array_equal(ax[:n], ex) and np.array_equal(ay[:n], ey)
    if job in ("n0", "all_dropped"):
        assert n == 0 and (job == "n0") == (erep == 0)
    if job == "tandem_63_64" and flag == 0:
        cnt = [c["table"][int(x) >> 8][1] for x in c["mx"]]                              # without a filter every occurrence below max_occ is an anchor
        first = sum(k for k in cnt[:63] if k < c["max_occ"])
        assert cnt[63] == cnt[64] > 0 and all(int(y) & SEED_TANDEM for y in ay[first:first + 2 * cnt[63]])
    # a slot smaller than the job: seed_wave still reports the whole count and fills the slot with the first anchors; the window body knows no slot
    if n >= 2:
        (bx, by, bres), _ = _both(S, c, flag, keyed, n // 2)
        assert int(bres[0]) == n and int(bres[1]) == erep and np.array_equal(bx[:n // 2], wx[:n // 2]) and np.array_equal(by[:n // 2], wy[:n // 2])
