"""Process body of tests/test_chain_edges_gpu.py::test_fill_switches_read_once_per_process: the dense cases of tests/chaincases.py through wm_chain_batch
and / or wm_window_batch in a process of its own, because WM_CHAIN_WIDE (and, in the window call, WM_CHAIN_WIDE_FIRST) is read once per process. The
parent sets the switch in the environment; this prints one line, "VERDICT ok ..." or "VERDICT MISMATCH ...", and exits 0 / 1.
   python tests/chain_edges_child.py chain+window | chain | window"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(mode):
    from winnowmap_amd import gpu, synth
    import test_chain_edges_gpu as T
    jobs = T.dense_jobs()
    ctx = gpu.Context(0, 2 << 30)
    bad = []
    if "chain" in mode:
        bad += [("chain", c["name"], p["min_cnt"]) for (c, p), g in zip(jobs, T.chain_batch(ctx, jobs)) if not T.same(g, T.want(c, p))]
    if "window" in mode:
        tmp = tempfile.mkdtemp()                       # the window call takes k and w from an uploaded index, however small
        synth.write_fasta(tmp + "/ref.fa", synth.make_reference(1, 20000, 3, repeat_frac=0.0))
        idx = gpu.Index(tmp + "/ref.fa", None, k=15, w=50)
        idx.upload(ctx)
        bad += [("window", c["name"], p["min_cnt"]) for (c, p), g in zip(jobs, T.window_batch(ctx, jobs)[1]) if not T.same(g, T.want(c, p))]
        idx.close()
    ctx.close()
    switches = " ".join("%s=%s" % (k, os.environ[k]) for k in ("WM_CHAIN_WIDE", "WM_CHAIN_WIDE_GEOM", "WM_CHAIN_WIDE_FIRST") if k in os.environ)
    print("VERDICT %s mode=%s jobs=%d %s %s" % ("MISMATCH" if bad else "ok", mode, len(jobs), switches, bad[:6] if bad else ""), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "chain+window"))
