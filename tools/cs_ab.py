#!/usr/bin/env python3
"""A/B of the mapper's switch for the cs:Z / MD:Z bodies under MM_F_OUT_CS (wm_set_cs_device, DESIGN.md "--cs / --MD on the device"): synthetic reads of
bench config 2's kind (15 kb ONT-profile, 1 % with a structural variant) against a synthetic reference, MM_F_CIGAR | MM_F_OUT_CG | MM_F_OUT_CS, the switch off
and on alternately, --runs runs each after one warm-up run of either. One JSON line per run on stdout: mapped Gbp/s (read bases over the wall time of the
mapping call, which ends in a device synchronise), wall time, host CPU-seconds of the process during the call, wm_cs_stats, and the SHA-256 of the text — the
same in every run (the switch must not change it)."""
import argparse
import hashlib
import json
import os
import resource
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from winnowmap_amd import gpu, synth      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--ref-mb", type=float, default=40.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", 16)))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    n_contigs = max(1, int(round(args.ref_mb / 10.0)))
    ref = synth.make_reference(n_contigs, int(args.ref_mb * 1e6 / n_contigs), 3, repeat_frac=0.10)
    fa = os.path.join(tmp, "ref.fa")
    synth.write_fasta(fa, ref, prefix="ctg")
    kf = os.path.join(tmp, "repetitive_k15.txt")
    gpu.write_repetitive_kmers(fa, 15, kf)
    reads, _ = synth.make_reads(ref, args.reads, args.read_len, 4, profile="ont", sv_frac=0.01)
    seqs = [synth.codes_to_ascii(r) for r in reads]
    bases = sum(len(s) for s in seqs)
    ctx = gpu.Context(0, 8 << 30)
    idx = gpu.Index(fa, kf, k=15, w=50, n_threads=args.threads)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, "map-ont", gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG | gpu.MM_F_OUT_CS)
    m.set_threads(args.threads, 0)
    batch = gpu.Mapper.marshal(["r%d" % i for i in range(len(seqs))], seqs)
    first = None

    def one(on, tag):
        nonlocal first
        gpu.set_cs_device(on)
        gpu.cs_stats(reset=True)
        r0 = resource.getrusage(resource.RUSAGE_SELF)
        t0 = time.perf_counter()
        text, hits, cigars, _ = m.map(batch)
        dt = time.perf_counter() - t0
        r1 = resource.getrusage(resource.RUSAGE_SELF)
        digest = hashlib.sha256(text).hexdigest()
        if first is None:
            first = digest
        return {"run": tag, "cs_device": on, "metric": "mapped Gbp/s", "value": bases / dt / 1e9, "wall_s": round(dt, 4),
                "host_cpu_s": round((r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime), 3), "cs_stats": gpu.cs_stats(),
                "reads": len(seqs), "read_len": args.read_len, "ref_mb": args.ref_mb, "host_threads": args.threads, "hits": int(len(hits)),
                "cigar_ops": int(len(cigars)), "text_bytes": len(text), "text_sha256": digest, "same_output_as_first_run": digest == first}

    try:
        for on in (0, 1):
            one(on, "warm-up")
        for k in range(args.runs):
            for on in (0, 1):
                print(json.dumps(one(on, "%s (%d)" % ("WM_CS_DEV=1" if on else "off", k + 1))), flush=True)
    finally:
        gpu.set_cs_device(-1)
        m.close(); idx.close(); ctx.close()


if __name__ == "__main__":
    main()
