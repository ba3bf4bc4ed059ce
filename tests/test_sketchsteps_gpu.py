"""GPU: long sequences sketched chunk by chunk under -H and at an even k (csrc/wm_index.hip: sketch_steps_* kernels) — wm_sketch_batch, the window call and the
device index build against the oracle / the host build, and against the one-wavefront-per-sequence routing in the same process (wm_sketch_set_step_chunks).
Default thresholds: WM_SKETCH_LONG = 65 536, WM_SKETCH_CHUNK = 16 384. The oracle's sketch is pinned to the reference's at these k and under -H by
tests/test_evenk_emu.py and tests/test_oracle_vs_ref.py."""
import tempfile

import numpy as np
import pytest

import evenkcases as EK
import wmtest as W
from winnowmap_amd import gpu, synth
from test_evenk_gpu import win14, _bind, _sketch_batch, _jobs, _per_job  # noqa: F401  (win14: a fixture)

pytestmark = pytest.mark.gpu
CHUNK = 16384
AT = np.array([0, 3], np.uint8)


def long_sequence(seed=3):
    """120 000 codes: a 40 000-base poly-A run, a 40 000-base (AT)n array with a two-base N inside, a three-base N elsewhere, random otherwise"""
    s = synth.random_codes(120000, np.random.default_rng(seed))
    s[10000:50000] = 0
    s[60000:100000] = np.tile(AT, 20000)
    s[80000:80002] = 4                                     # (the array keeps its phase behind the N)
    s[110000:110003] = 4
    return np.ascontiguousarray(s, np.uint8)


@pytest.fixture(scope="module")
def small_ref():
    tmp = tempfile.mkdtemp()
    ref = EK.reference(5, 2, 40000, 30)
    fa = tmp + "/ref.fa"
    synth.write_fasta(fa, ref)
    out = dict(fa=fa, ref=ref)
    for k in (14, 15):
        km, cnt = synth.repetitive_kmers(ref, k)
        synth.write_kmer_list(tmp + "/rep%d.txt" % k, km, cnt, k)
        out[k] = (tmp + "/rep%d.txt" % k, W.o_bloom(km))
    return out


class _Sketcher:
    """a context that sketches at (k, w): through an uploaded -H index (as test_evenk_gpu does) or, without -H, through wm_sketch_set_filter with no -W list"""

    def __init__(self, D, k, w, hpc):
        self.L = _bind(gpu.lib())
        self.ctx = gpu.Context(0, 2 << 30)
        self.idx = None
        self.k, self.w, self.hpc, self.bloom = k, w, hpc, None
        if hpc:
            self.idx = gpu.Index(D["fa"], D[k][0], k=k, w=w, hpc=True)
            self.idx.upload(self.ctx)
            self.bloom = D[k][1]
        else:
            assert self.L.wm_sketch_set_filter(self.ctx._h, None, 0, 0, 0, 0, k, w) == 0, self.L.wm_last_error()

    def sketch(self, seqs):
        return _sketch_batch(self.L, self.ctx, seqs)

    def oracle(self, s):
        return W.o_sketch(bytes(s), self.w, self.k, rid=0, bloom=self.bloom, hpc=self.hpc)

    def close(self):
        if self.idx is not None:
            self.idx.close()
        self.ctx.close()


def _same(g, e, what):
    assert len(g) == len(e[0]) and np.array_equal(g["x"], e[0]) and np.array_equal(g["y"], e[1]), what + (len(g), len(e[0]))


MODES = [(15, True), (14, False), (14, True)]                # (k, -H)


@pytest.mark.parametrize("k,hpc", MODES)
def test_sketch_batch_of_a_long_sequence_in_chunks(small_ref, k, hpc):
    S = _Sketcher(small_ref, k, 50, hpc)
    try:
        s, short = long_sequence(), synth.random_codes(30000, np.random.default_rng(8))
        short[5000:6000] = 2
        short[20000:20600] = np.tile(AT, 300)
        es, eshort = S.oracle(s), S.oracle(short)
        assert len(es[0]) > 500 and len(eshort[0]) > 500
        gpu.set_sketch_step_chunks(1)
        g = S.sketch([s])[0]
        n_chunks = S.ctx.last_sketch_chunks()
        _same(g, es, (k, hpc, "chunked"))
        assert n_chunks == -(-len(s) // CHUNK) and n_chunks > 1, n_chunks
        # a sequence below the threshold beside it: both right, only the long one's chunks are counted
        g2 = S.sketch([short, s])
        _same(g2[0], eshort, (k, hpc, "short, mixed")); _same(g2[1], es, (k, hpc, "long, mixed"))
        assert S.ctx.last_sketch_chunks() == n_chunks
        assert len(S.sketch([short])[0]) == len(eshort[0]) and S.ctx.last_sketch_chunks() == 0
        # the switch off: one wavefront per sequence, byte for byte the same
        gpu.set_sketch_step_chunks(0)
        g0 = S.sketch([s])[0]
        assert S.ctx.last_sketch_chunks() == 0
        assert g0.tobytes() == g.tobytes()
    finally:
        gpu.set_sketch_step_chunks(-1)
        S.close()


@pytest.mark.parametrize("k,hpc", [(14, False), (15, True)])
def test_capacity_overflow_repeats_the_job_on_one_wavefront(small_ref, k, hpc):
    """w = 3: one base in two is a minimizer, the job's slot of len / 8 + 16 and the chunks' slots of len / 4 + 64 overflow, and the job comes back through the
    repeat with a full-size slot"""
    S = _Sketcher(small_ref, k, 3, hpc)
    try:
        s = synth.random_codes(70000, np.random.default_rng(9))
        s[30000:30500] = 1
        e = S.oracle(s)
        assert len(e[0]) > len(s) // 4 + 64
        gpu.set_sketch_step_chunks(1)
        g = S.sketch([s])[0]
        _same(g, e, (k, hpc, "overflow"))
        assert S.ctx.last_sketch_chunks() == -(-len(s) // CHUNK)       # (the first round ran in chunks)
    finally:
        gpu.set_sketch_step_chunks(-1)
        S.close()


@pytest.mark.parametrize("k", [15, 14])
def test_window_batch_on_an_H_index_with_long_jobs(win14, k):
    """two jobs of 70 000 bases, one staged and one resident packed, beside short ones: per job the counts, the sorted anchors and the chains are the same bytes
    with the chunked sketch and with one wavefront per sequence, and n_mini is the oracle's count"""
    D = win14
    ref = D["ref"]
    km, cnt = synth.repetitive_kmers(ref, k)
    kf = D["tmp"] + "/rep_steps%d.txt" % k
    synth.write_kmer_list(kf, km, cnt, k)
    bloom = W.o_bloom(km)
    longs = [ref[0][20000:90000].copy(), ref[1][50000:120000].copy()]
    longs[0][30000:31000] = 3
    longs[0][40000:42000] = np.tile(AT, 1000)
    longs[0][41000:41002] = 4
    longs[1][10000:10003] = 4
    longs[1][60000:64000] = 1
    seqs = [np.ascontiguousarray(s, np.uint8) for s in longs] + D["seqs"][:12]
    ctx = gpu.Context(0, 4 << 30)
    idx = gpu.Index(D["fa"], kf, k=k, w=50, n_threads=8, hpc=True)
    idx.upload(ctx)
    try:
        flat = np.concatenate(seqs)
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])[:-1]])
        ctx.reads_upload(flat)
        J = _jobs(len(seqs))
        for j, s in enumerate(seqs):
            J[j]["len"] = len(s)
            if j % 2:
                J[j]["seq_off"] = int(off[j])                  # resident
            else:
                J[j]["seq_off"], J[j]["stage_off"] = -1, int(off[j])
        out = {}
        for on in (1, 0):
            gpu.set_sketch_step_chunks(on)
            out[on] = _per_job(ctx.window_batch_dust(J, None, flat, np.zeros((1, 2), np.uint64), 200, 0, 0, 1 << 22, 1 << 22))
            assert ctx.last_sketch_chunks() == (2 * -(-70000 // CHUNK) if on else 0)
        for j, s in enumerate(seqs):
            assert out[1][j] == out[0][j], (k, j, len(s), out[1][j][:3], out[0][j][:3])
            assert out[1][j][2] == len(W.o_sketch(bytes(s), 50, k, rid=0, bloom=bloom, hpc=True)[0]), (k, j, len(s))
        assert out[1][0][0] > 1000 and out[1][1][0] > 1000 and len(out[1][0][3]) > 0 and len(out[1][1][3]) > 0      # (anchors and chains of the long jobs)
    finally:
        gpu.set_sketch_step_chunks(-1)
        W.oracle().wmo_bloom_free(bloom)
        idx.close(); ctx.close()


@pytest.mark.parametrize("k", [15, 14])
def test_device_index_build_with_H_and_a_long_contig(k):
    """wm_index_build_gpu_flag(MM_I_HPC) on contigs of 150 000 and 20 000 bases with planted homopolymers and microsatellites: bit-identical to the host build,
    the long contig sketched in chunks"""
    tmp = tempfile.mkdtemp()
    rng = np.random.default_rng(50 + k)
    ref = [synth.random_codes(150000, rng), synth.random_codes(20000, rng)]
    for c in ref:
        for _ in range(len(c) // 2500):
            n = int(rng.integers(10, 400)); p = int(rng.integers(0, len(c) - n))
            c[p:p + n] = rng.integers(0, 4)
    EK.plant_microsatellites(ref, rng, 60)
    ref[0][70000:90000] = 2                                    # a run longer than a chunk
    ref[0][100000:118000] = np.tile(AT, 9000)
    ref[0][109000:109002] = 4
    fa, kf = tmp + "/ref.fa", tmp + "/rep.txt"
    synth.write_fasta(fa, ref)
    km, cnt = synth.repetitive_kmers(ref, k)
    synth.write_kmer_list(kf, km, cnt, k)
    host = gpu.Index(fa, kf, k=k, w=50, n_threads=8, hpc=True)
    hs, ha = host.export_arrays()
    c = gpu.Context(0, 2 << 30)
    try:
        gpu.set_sketch_step_chunks(1)
        dev, st = gpu.Index.build_on_device(c, fa, kf, k=k, w=50, n_threads=8, hpc=True)
        assert c.last_sketch_chunks() == -(-150000 // CHUNK)
        ds, da = dev.export_arrays()
        assert np.array_equal(hs, ds), (hs, ds)
        for a, b in zip(ha, da):
            assert np.array_equal(a, b)
        assert st["minimizers"] == host.n_minimizers and st["minimizers"] > 2000
        dev.close()
    finally:
        gpu.set_sketch_step_chunks(-1)
        host.close(); c.close()
