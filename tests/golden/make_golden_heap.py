"""Generates tests/golden/e2e_ont_heap.npz: the REAL reference (oracle/_ref, built from /root/reference) with --heap-sort=yes (MM_F_HEAP_SORT) on reads that
carry a tandem duplication inside the read (winnowmap_amd/synth.py: make_dup_reads) — the reads on which the heap-merged seed order and the radix-sorted one
give different records. Run in the build container:  python tests/golden/make_golden_heap.py
Same layout as the fixtures of make_golden.py (hits, cigars, first; MAPQ zeroed for reads of the MCAS path). The test regenerates the inputs from the seeds."""
import ctypes as C
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wmtest as W  # noqa: E402
from winnowmap_amd import synth  # noqa: E402

NAME = "ont_heap"
PRESET, K, HEAP_SORT = "map-ont", 15, 0x400000


def inputs(tmpdir):
    """-> (preset, fasta, k, reads): 14 duplicated reads below the 10-kb MCAS gate and 2 above it, against one random 300-kb contig"""
    ref = synth.make_reference(1, 300000, 45)
    fa = os.path.join(tmpdir, NAME + ".fa")
    synth.write_fasta(fa, ref)
    reads = synth.make_dup_reads(ref, 14, 46) + synth.make_dup_reads(ref, 2, 47, host=(11000, 13000))
    return PRESET, fa, K, [synth.codes_to_ascii(r) for r in reads]


def reference_hits(flag_extra, tmpdir):
    R = W.ref()
    R.refshim_idx_build_flag.restype = C.c_void_p
    R.refshim_idx_build_flag.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    preset, fa, k, reads = inputs(tmpdir)
    mi = R.refshim_idx_build_flag(fa.encode(), b"", k, 50, 0, 4)
    opt = R.refshim_mapopt(preset.encode(), 0x4 | 0x20 | flag_extra, mi)
    hits, cigs, first = [], [], [0]
    for i, s in enumerate(reads):
        h = np.zeros(16 * 256, np.int32)
        c = np.zeros(2000000, np.uint32)
        nc = C.c_int64()
        n = R.refshim_map(mi, opt, s, len(s), ("read%d" % i).encode(), h, 256, c, len(c), C.byref(nc))
        hh = h[:16 * n].reshape(-1, 16).copy()
        if len(s) >= 10000:
            hh[:, 6] = 0
        hits.append(hh)
        cigs.append(c[:nc.value].copy())
        first.append(first[-1] + n)
    return np.concatenate(hits), np.concatenate(cigs), np.array(first, np.int64)


def main():
    tmp = tempfile.mkdtemp()
    hits, cigs, first = reference_hits(HEAP_SORT, tmp)
    plain = reference_hits(0, tmp)
    differs = not (np.array_equal(hits, plain[0]) and np.array_equal(cigs, plain[1]))
    np.savez_compressed(os.path.join(HERE, "e2e_%s.npz" % NAME), hits=hits, cigars=cigs, first=first)
    print(NAME, "reads", len(first) - 1, "hits", int(first[-1]), "cigar ops", len(cigs), "differs from --heap-sort=no:", differs)


if __name__ == "__main__":
    main()
