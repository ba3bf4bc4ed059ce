"""ctypes binding of libwmgpu.so (include/wm_gpu.h). No fallback: if the HIP library is missing or no
device is usable, every call raises."""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WM_LIBWMGPU") or os.path.join(HERE, "libwmgpu.so")      # (WM_LIBWMGPU: a variant build for A/B runs, winnowmap_amd/build.py)


class WmError(RuntimeError):
    pass


class KswScore(C.Structure):
    _fields_ = [("match", C.c_int8), ("mismatch", C.c_int8), ("sc_ambi", C.c_int8),
                ("q", C.c_int8), ("e", C.c_int8), ("q2", C.c_int8), ("e2", C.c_int8)]


KSW_JOB_DTYPE = np.dtype([("q_off", np.uint32), ("t_off", np.uint32), ("qlen", np.int32), ("tlen", np.int32),
                          ("w", np.int32), ("zdrop", np.int32), ("end_bonus", np.int32), ("flag", np.int32)])
KSW_RES_DTYPE = np.dtype([("max", np.int32), ("zdropped", np.int32), ("max_q", np.int32), ("max_t", np.int32),
                          ("mqe", np.int32), ("mqe_t", np.int32), ("mte", np.int32), ("mte_q", np.int32),
                          ("score", np.int32), ("reach_end", np.int32), ("n_cigar", np.int32), ("cig_off", np.uint32)])

KSW_F_ZDWALK = 0x10000        # wm_ksw_batch_pos_zd: run the z-drop scan on this job's alignment
KSW_POS_DTYPE = np.dtype([("qwin_off", np.int64), ("qwin_len", np.int32), ("q_pos", np.int32), ("rid", np.int32), ("t_pos", np.int32),
                          ("qlen", np.int32), ("tlen", np.int32), ("w", np.int32), ("zdrop", np.int32), ("end_bonus", np.int32), ("flag", np.int32),
                          ("step", np.int8), ("has_n", np.int8), ("pad", np.int8, (6,))])      # wm_ksw_pos_t

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WmError("libwmgpu.so is not built (run `python -m winnowmap_amd.build`); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.wm_last_error.restype = C.c_char_p
        L.wm_ctx_create.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.wm_ctx_destroy.argtypes = [C.c_void_p]
        L.wm_last_kernel_ms.restype = C.c_float
        L.wm_last_kernel_ms.argtypes = [C.c_void_p]
        L.wm_ksw_batch.argtypes = [C.c_void_p, C.POINTER(KswScore), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.wm_ksw_dev_prepare.argtypes = [C.c_void_p, C.POINTER(KswScore), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.wm_ksw_dev_run.argtypes = [C.c_void_p, C.c_void_p]
        L.wm_ksw_dev_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.wm_ksw_dev_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.wm_ksw_dev_free.argtypes = [C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise WmError("libwmgpu error %d: %s" % (rc, lib().wm_last_error().decode()))


class Context:
    """One GPU context (HIP device + stream + HBM arena)."""

    def __init__(self, device=0, arena_bytes=0):
        self._h = C.c_void_p()
        _chk(lib().wm_ctx_create(device, arena_bytes, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().wm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_sketch_chunks(self):
        """wm_last_sketch_chunks: chunks the last sketch, window or index-sketch call on this context ran as wavefronts of their own (0: one wavefront per sequence)"""
        lib().wm_last_sketch_chunks.argtypes = [C.c_void_p]
        lib().wm_last_sketch_chunks.restype = C.c_int
        return int(lib().wm_last_sketch_chunks(self._h))

    # ---- ksw -------------------------------------------------------------------------------------
    def ksw_batch(self, score, jobs, seqs):
        """jobs: structured array KSW_JOB_DTYPE; seqs: uint8 codes. Returns (results KSW_RES_DTYPE, cigar pool)."""
        jobs = np.ascontiguousarray(jobs, KSW_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        res = np.zeros(len(jobs), KSW_RES_DTYPE)
        cap = int((jobs["qlen"].astype(np.int64) + jobs["tlen"] + 2).sum()) + 16
        pool = np.zeros(cap, np.uint32)
        used = C.c_size_t(0)
        _chk(lib().wm_ksw_batch(self._h, C.byref(score), len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes,
                                res.ctypes.data, pool.ctypes.data, cap, C.byref(used)))
        return res, pool[:used.value]

    def ksw_exts2_batch(self, score, noncan, junc_bonus, jobs, seqs, junc=None):
        """wm_ksw_exts2_batch: the splice-aware extension (ksw_exts2_sse); junc = None or uint8 array parallel to seqs"""
        jobs = np.ascontiguousarray(jobs, KSW_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        jn = None if junc is None else np.ascontiguousarray(junc, np.uint8)
        assert jn is None or jn.nbytes == seqs.nbytes
        res = np.zeros(len(jobs), KSW_RES_DTYPE)
        cap = int((jobs["qlen"].astype(np.int64) + jobs["tlen"] + 2).sum()) + 16
        pool = np.zeros(cap, np.uint32)
        used = C.c_size_t(0)
        lib().wm_ksw_exts2_batch.argtypes = [C.c_void_p, C.POINTER(KswScore), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _chk(lib().wm_ksw_exts2_batch(self._h, C.byref(score), noncan, junc_bonus, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes,
                                      None if jn is None else jn.ctypes.data, res.ctypes.data, pool.ctypes.data, cap, C.byref(used)))
        return res, pool[:used.value]

    def reads_upload(self, codes):
        """0..4 codes of the current mini-batch, kept resident for position jobs (wm_reads_upload)"""
        codes = np.ascontiguousarray(codes, np.uint8)
        lib().wm_reads_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        _chk(lib().wm_reads_upload(self._h, codes.ctypes.data, codes.nbytes))

    def ksw_batch_pos(self, score, jobs):
        """jobs: structured array KSW_POS_DTYPE (operands as positions in the resident reads / packed reference, wm_ksw_batch_pos)"""
        jobs = np.ascontiguousarray(jobs, KSW_POS_DTYPE)
        assert KSW_POS_DTYPE.itemsize == 56
        res = np.zeros(len(jobs), KSW_RES_DTYPE)
        cap = int((np.maximum(jobs["qlen"], 0).astype(np.int64) + np.maximum(jobs["tlen"], 0) + 2).sum()) + 16
        pool = np.zeros(cap, np.uint32)
        used = C.c_size_t(0)
        lib().wm_ksw_batch_pos.argtypes = [C.c_void_p, C.POINTER(KswScore), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _chk(lib().wm_ksw_batch_pos(self._h, C.byref(score), len(jobs), jobs.ctypes.data, res.ctypes.data, pool.ctypes.data, cap, C.byref(used)))
        return res, pool[:used.value]

    def ksw_batch_pos_zd(self, score, jobs):
        """wm_ksw_batch_pos_zd: as ksw_batch_pos, plus the z-drop scan (mm_test_zdrop's walk, src/align.c:32-66) of every job whose flag carries
        KSW_F_ZDWALK, run on the device over the finished CIGARs -> (results, pool, zd[n, 5] = max_zdrop, t0, t1, q0, q1)"""
        jobs = np.ascontiguousarray(jobs, KSW_POS_DTYPE)
        res = np.zeros(len(jobs), KSW_RES_DTYPE)
        cap = int((np.maximum(jobs["qlen"], 0).astype(np.int64) + np.maximum(jobs["tlen"], 0) + 2).sum()) + 16
        pool = np.zeros(cap, np.uint32)
        zd = np.zeros((len(jobs), 5), np.int32)
        used = C.c_size_t(0)
        lib().wm_ksw_batch_pos_zd.argtypes = [C.c_void_p, C.POINTER(KswScore), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        _chk(lib().wm_ksw_batch_pos_zd(self._h, C.byref(score), len(jobs), jobs.ctypes.data, res.ctypes.data, pool.ctypes.data, cap, C.byref(used), zd.ctypes.data))
        return res, pool[:used.value], zd

    # ---- ksw_ll_i16: the local-alignment score with the striped machine's end coordinates -----------------
    def ksw_ll_batch(self, mat5x5, gapo, gape, jobs, seqs, out=None):
        """wm_ksw_ll_batch: jobs: structured array LL_JOB_DTYPE (operands as 0..4 codes inside seqs, step = 1 / -1). Returns int32 [n, 3] = score, qe, te per job,
        exactly what wm_ksw_ll_i16 returns (in `out` if one is given: a refused call leaves it untouched)."""
        jobs = np.ascontiguousarray(jobs, LL_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        mat = np.ascontiguousarray(mat5x5, np.int8)
        assert LL_JOB_DTYPE.itemsize == 20 and mat.shape == (25,)
        out = np.zeros((len(jobs), 3), np.int32) if out is None else out
        assert out.dtype == np.int32 and out.flags.c_contiguous and out.size >= 3 * len(jobs)
        lib().wm_ksw_ll_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        _chk(lib().wm_ksw_ll_batch(self._h, mat.ctypes.data, int(gapo), int(gape), len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, out.ctypes.data))
        return out

    def ksw_ll_batch_pos(self, mat5x5, gapo, gape, jobs, out=None):
        """wm_ksw_ll_batch_pos: jobs: structured array LL_POS_DTYPE (operands as positions in the resident reads, two-strand space, and the uploaded reference)"""
        jobs = np.ascontiguousarray(jobs, LL_POS_DTYPE)
        mat = np.ascontiguousarray(mat5x5, np.int8)
        assert LL_POS_DTYPE.itemsize == 40 and mat.shape == (25,)
        out = np.zeros((len(jobs), 3), np.int32) if out is None else out
        assert out.dtype == np.int32 and out.flags.c_contiguous and out.size >= 3 * len(jobs)
        lib().wm_ksw_ll_batch_pos.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _chk(lib().wm_ksw_ll_batch_pos(self._h, mat.ctypes.data, int(gapo), int(gape), len(jobs), jobs.ctypes.data, out.ctypes.data))
        return out

    # ---- the scan of mm_update_extra over final CIGARs ----------------------------------------------
    def extra_batch(self, score, jobs, seqs, cigars):
        """wm_extra_batch: score = (match, mismatch, ambi, q, e) as literal values; jobs: structured array EXTRA_JOB_DTYPE (operands as 0..4 codes inside
        seqs); cigars: uint32 BAM ops. Returns int32 [n, 6] = dp_max, mlen, blen, n_ambi, qoff, toff per job."""
        jobs = np.ascontiguousarray(jobs, EXTRA_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        cigars = np.ascontiguousarray(cigars, np.uint32)
        sc = np.array(score, np.int32)
        assert EXTRA_JOB_DTYPE.itemsize == 16 and sc.shape == (5,)
        out = np.zeros((len(jobs), 6), np.int32)
        lib().wm_extra_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        _chk(lib().wm_extra_batch(self._h, sc.ctypes.data, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, cigars.ctypes.data, len(cigars), out.ctypes.data))
        return out

    def extra_batch_pos(self, score, jobs, cigars):
        """wm_extra_batch_pos: jobs: structured array EXTRA_POS_DTYPE (operands as positions in the resident reads, two-strand space, and the uploaded reference)"""
        jobs = np.ascontiguousarray(jobs, EXTRA_POS_DTYPE)
        cigars = np.ascontiguousarray(cigars, np.uint32)
        sc = np.array(score, np.int32)
        assert EXTRA_POS_DTYPE.itemsize == 32 and sc.shape == (5,)
        out = np.zeros((len(jobs), 6), np.int32)
        lib().wm_extra_batch_pos.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        _chk(lib().wm_extra_batch_pos(self._h, sc.ctypes.data, len(jobs), jobs.ctypes.data, cigars.ctypes.data, len(cigars), out.ctypes.data))
        return out

    # ---- mm_fix_cigar on stitched CIGARs, fused with that scan ------------------------------------------
    def fix_extra_batch(self, score, jobs, seqs, cigars):
        """wm_fix_extra_batch: cigars = the stitched CIGARs; score = (match, mismatch, ambi, q, e) or None for the fix alone. Returns (cigars_out, fix, extra):
        job i's fixed CIGAR is cigars_out[cig_off : cig_off + fix[i, 0]]; fix = int32 [n, 4] = n_cigar, qshift, tshift, changed; extra = int32 [n, 6] as
        extra_batch gives for the fixed CIGAR with the operands advanced by both shifts (None without a score)."""
        jobs = np.ascontiguousarray(jobs, EXTRA_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        cigars = np.ascontiguousarray(cigars, np.uint32)
        sc = None if score is None else np.array(score, np.int32)
        assert sc is None or sc.shape == (5,)
        out = np.zeros(len(cigars), np.uint32); fix = np.zeros((len(jobs), 4), np.int32)
        extra = None if sc is None else np.zeros((len(jobs), 6), np.int32)
        lib().wm_fix_extra_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(lib().wm_fix_extra_batch(self._h, None if sc is None else sc.ctypes.data, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, cigars.ctypes.data,
                                      len(cigars), out.ctypes.data, fix.ctypes.data, None if extra is None else extra.ctypes.data))
        return out, fix, extra

    def fix_extra_batch_pos(self, score, jobs, cigars):
        """wm_fix_extra_batch_pos: jobs: structured array EXTRA_POS_DTYPE (operands as positions in the resident reads, two-strand space, and the uploaded reference)"""
        jobs = np.ascontiguousarray(jobs, EXTRA_POS_DTYPE)
        cigars = np.ascontiguousarray(cigars, np.uint32)
        sc = None if score is None else np.array(score, np.int32)
        assert sc is None or sc.shape == (5,)
        out = np.zeros(len(cigars), np.uint32); fix = np.zeros((len(jobs), 4), np.int32)
        extra = None if sc is None else np.zeros((len(jobs), 6), np.int32)
        lib().wm_fix_extra_batch_pos.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(lib().wm_fix_extra_batch_pos(self._h, None if sc is None else sc.ctypes.data, len(jobs), jobs.ctypes.data, cigars.ctypes.data, len(cigars), out.ctypes.data,
                                          fix.ctypes.data, None if extra is None else extra.ctypes.data))
        return out, fix, extra

    # ---- mm_update_cigar_eqx over final CIGARs: M -> runs of = / X ----------------------------------------
    def _eqx(self, fn, head, cigars, n_jobs, out_cap):
        cigars = np.ascontiguousarray(cigars, np.uint32)
        assert EQX_RES_DTYPE.itemsize == 16
        if out_cap is None:          # every op, and one more per M column: what a CIGAR can become at most
            out_cap = len(cigars) + int((cigars[(cigars & 0xf) == 0] >> 4).astype(np.int64).sum())
        pool = np.zeros(max(int(out_cap), 1), np.uint32)
        res = np.zeros(n_jobs, EQX_RES_DTYPE)
        used = C.c_size_t(0)
        rc = fn(*head, cigars.ctypes.data, len(cigars), pool.ctypes.data, int(out_cap), C.byref(used), res.ctypes.data)
        if rc != 0:
            e = WmError("libwmgpu error %d: %s" % (rc, lib().wm_last_error().decode()))
            e.rc, e.needed, e.res = rc, used.value, res       # (WM_ENOMEM = -3: `needed` ops, res is already filled)
            raise e
        return pool[:used.value], res

    def eqx_batch(self, jobs, seqs, cigars, out_cap=None):
        """wm_eqx_batch: jobs: structured array EXTRA_JOB_DTYPE (operands as 0..4 codes inside seqs, advanced by mm_fix_cigar's shifts); cigars: the FINAL CIGARs.
        Returns (pool, res): res = EQX_RES_DTYPE per job, job i's new CIGAR is pool[off : off + n_cigar], in_place = the branch of src/align.c:195-201 ran.
        out_cap: ops the pool holds (None = a safe bound); too small raises WmError with .rc == -3, .needed and .res set."""
        jobs = np.ascontiguousarray(jobs, EXTRA_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        lib().wm_eqx_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        return self._eqx(lib().wm_eqx_batch, (self._h, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes), cigars, len(jobs), out_cap)

    def eqx_batch_pos(self, jobs, cigars, out_cap=None):
        """wm_eqx_batch_pos: jobs: structured array EXTRA_POS_DTYPE (operands as positions in the resident reads, two-strand space, and the uploaded reference)"""
        jobs = np.ascontiguousarray(jobs, EXTRA_POS_DTYPE)
        lib().wm_eqx_batch_pos.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        return self._eqx(lib().wm_eqx_batch_pos, (self._h, len(jobs), jobs.ctypes.data), cigars, len(jobs), out_cap)

    # ---- the bodies of the cs:Z / MD:Z tags over final CIGARs ---------------------------------------------------
    def _cs(self, fn, head, cigars, n_jobs, out_cap):
        cigars = np.ascontiguousarray(cigars, np.uint32)
        assert CS_RES_DTYPE.itemsize == 16
        if out_cap is None:          # wm_cigar_cs_bound over all ops: 3 bytes per M column, 1 per gap base, 12 per op, 16 per N, 11 per job
            op, ln = cigars & 0xf, (cigars >> 4).astype(np.int64)
            out_cap = int(np.where((op == 1) | (op == 2), ln + 12, np.where(op == 3, 16, 3 * ln + 12)).sum()) + 11 * n_jobs
        pool = np.zeros(max(int(out_cap), 1), np.uint8)
        res = np.zeros(n_jobs, CS_RES_DTYPE)
        used = C.c_size_t(0)
        rc = fn(*head, cigars.ctypes.data, len(cigars), pool.ctypes.data, int(out_cap), C.byref(used), res.ctypes.data)
        if rc != 0:
            e = WmError("libwmgpu error %d: %s" % (rc, lib().wm_last_error().decode()))
            e.rc, e.needed, e.res = rc, used.value, res       # (WM_ENOMEM = -3: `needed` bytes, res is already filled)
            raise e
        return pool[:used.value], res

    def cs_batch(self, mode, jobs, seqs, cigars, out_cap=None):
        """wm_cs_batch: mode = CS_SHORT / CS_LONG / CS_MD; jobs: structured array EXTRA_JOB_DTYPE (operands as 0..4 codes inside seqs); cigars: the FINAL CIGARs.
        Returns (text, res): res = CS_RES_DTYPE per job, job i's tag body is text[off : off + len] (uint8, no prefix, no terminator).
        out_cap: bytes the pool holds (None = a safe bound); too small raises WmError with .rc == -3, .needed and .res set."""
        jobs = np.ascontiguousarray(jobs, EXTRA_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        lib().wm_cs_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        return self._cs(lib().wm_cs_batch, (self._h, int(mode), len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes), cigars, len(jobs), out_cap)

    def cs_batch_pos(self, mode, jobs, cigars, out_cap=None):
        """wm_cs_batch_pos: jobs: structured array EXTRA_POS_DTYPE (operands as positions in the resident reads, two-strand space, and the uploaded reference)"""
        jobs = np.ascontiguousarray(jobs, EXTRA_POS_DTYPE)
        lib().wm_cs_batch_pos.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        return self._cs(lib().wm_cs_batch_pos, (self._h, int(mode), len(jobs), jobs.ctypes.data), cigars, len(jobs), out_cap)

    def seed_batch_keyed(self, mini, mini_off, n_mini, qlen, keys, max_occ, flag, out_cap):
        """wm_seed_batch_keyed: collect_seed_hits with skip_seed's name comparison (src/map.c:132-154). mini: uint64 [n_total, 2]; keys: uint32 [n, 2]
        from Index.query_keys (None = wm_seed_batch: MM_F_NO_DIAG / MM_F_NO_DUAL are ignored). Returns (anchors uint64 [out_cap, 2], out_off, n_anchors, rep_len)."""
        L = lib()
        L.wm_seed_batch_keyed.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
        n = len(n_mini)
        mini = np.ascontiguousarray(mini, np.uint64)
        mini_off, n_mini, qlen = np.ascontiguousarray(mini_off, np.uint64), np.ascontiguousarray(n_mini, np.int32), np.ascontiguousarray(qlen, np.int32)
        keys = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(n, 2)
        out = np.zeros((out_cap, 2), np.uint64)
        out_off, n_a, rep_len = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _chk(L.wm_seed_batch_keyed(self._h, n, mini.ctypes.data, mini_off.ctypes.data, n_mini.ctypes.data, qlen.ctypes.data, None if keys is None else keys.ctypes.data,
                                   max_occ, flag, out.ctypes.data, out_cap, out_off.ctypes.data, n_a.ctypes.data, rep_len.ctypes.data))
        return out, out_off, n_a, rep_len

    def _window(self, fn, extra, jobs, keys, seqs, pre, max_occ, flag, u_cap, a_cap):
        """the two window calls below: fn = the C symbol, extra = what it takes between `flag` and the results ((ctypes type, value) pairs)"""
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int64] + [t for t, _ in extra] + \
                      [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        n = len(jobs)
        jobs = np.ascontiguousarray(jobs, WINDOW_JOB)
        keys = None if keys is None else np.ascontiguousarray(keys, np.uint32).reshape(n, 2)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        pre = np.ascontiguousarray(pre, np.uint64).reshape(-1, 2)
        res = np.zeros(n, WINDOW_RES)
        u_pool, a_pool = np.zeros(u_cap + 1, np.uint64), np.zeros((a_cap + 1, 2), np.uint64)
        uu, au = C.c_size_t(), C.c_size_t()
        _chk(fn(self._h, n, jobs.ctypes.data, None if keys is None else keys.ctypes.data, seqs.ctypes.data, seqs.nbytes, pre.ctypes.data, len(pre),
                max_occ, flag, *[v for _, v in extra], res.ctypes.data, u_pool.ctypes.data, u_cap, C.byref(uu), a_pool.ctypes.data, a_cap, C.byref(au)))
        return res, u_pool[:uu.value], a_pool[:au.value]

    def window_batch_keyed(self, jobs, keys, seqs, pre, max_occ, flag, u_cap, a_cap):
        """wm_window_batch_keyed. jobs: structured array WINDOW_JOB; keys: uint32 [n, 2] or None (= wm_window_batch); seqs: uint8 staging codes; pre: uint64 [n_pre, 2].
        Returns (res WINDOW_RES [n], u_pool, a_pool [.., 2])."""
        return self._window(lib().wm_window_batch_keyed, (), jobs, keys, seqs, pre, max_occ, flag, u_cap, a_cap)

    def window_batch_dust(self, jobs, keys, seqs, pre, max_occ, flag, sdust_thres, u_cap, a_cap):
        """wm_window_batch_dust: window_batch_keyed with the -T threshold — with sdust_thres > 0 every job's minimizers are squeezed by the SDUST intervals of
        its sequence before the seeding (mm_dust_minier, src/map.c:43-67); 0 = window_batch_keyed. Same arguments and results otherwise."""
        return self._window(lib().wm_window_batch_dust, ((C.c_int, sdust_thres),), jobs, keys, seqs, pre, max_occ, flag, u_cap, a_cap)

    def sdust_batch(self, seqs, seq_off, lens, thres, resident=None):
        """wm_sdust_batch: the SDUST intervals (sdust_core with W = 64, src/sdust.c:134-164) of n sequences of 0..4 codes. seqs: uint8 staging codes; sequence i
        is lens[i] codes at seq_off[i] of seqs, or of the resident reads where resident[i] != 0 (reads_upload). Returns (list of int32 [n_i, 2] arrays of
        (start, finish), high int32 [n] = the largest list of perfect intervals each sequence needed)."""
        L = lib()
        L.wm_sdust_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        seqs = np.ascontiguousarray(seqs, np.uint8)
        seq_off, lens = np.ascontiguousarray(seq_off, np.uint64), np.ascontiguousarray(lens, np.int32)
        n = len(lens)
        res = None if resident is None else np.ascontiguousarray(resident, np.uint8)
        cap = int((lens.astype(np.int64) // 4 + 24).sum()) + 1
        iv = np.zeros((cap, 2), np.int32)
        iv_off, n_iv, high = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _chk(L.wm_sdust_batch(self._h, n, seqs.ctypes.data, seqs.nbytes, seq_off.ctypes.data, lens.ctypes.data, None if res is None else res.ctypes.data, thres,
                              iv.ctypes.data, cap, iv_off.ctypes.data, n_iv.ctypes.data, high.ctypes.data))
        return [iv[int(iv_off[i]):int(iv_off[i]) + int(n_iv[i])].copy() for i in range(n)], high

    def kernel_stats(self):
        """wm_ctx_kernel_stats: {class id: (ms, cells, launches)} of this context's own ksw launches since it was created (classes: csrc/ksw_plan.h) — which
        kernel a batch ran on, for a context used without a mapper"""
        lib().wm_ksw_n_classes.restype = C.c_int
        out = np.zeros(3 * lib().wm_ksw_n_classes(), np.float64)
        n = C.c_int()
        lib().wm_ctx_kernel_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        _chk(lib().wm_ctx_kernel_stats(self._h, out.ctypes.data, len(out), C.byref(n)))
        return {k: (float(out[3 * k]), float(out[3 * k + 1]), int(out[3 * k + 2])) for k in range(n.value)}

    def ksw_prepare(self, score, jobs, seqs):
        jobs = np.ascontiguousarray(jobs, KSW_JOB_DTYPE)
        seqs = np.ascontiguousarray(seqs, np.uint8)
        h = C.c_void_p()
        _chk(lib().wm_ksw_dev_prepare(self._h, C.byref(score), len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, C.byref(h)))
        return KswDevBatch(self, h, jobs)


class KswDevBatch:
    def __init__(self, ctx, h, jobs):
        self.ctx, self._h, self.jobs = ctx, h, jobs

    def run(self):
        _chk(lib().wm_ksw_dev_run(self.ctx._h, self._h))

    def stats(self):
        cells, tbb, dp, bt = C.c_uint64(), C.c_uint64(), C.c_float(), C.c_float()
        lib().wm_ksw_dev_stats(self._h, C.byref(cells), C.byref(tbb), C.byref(dp), C.byref(bt))
        return dict(cells=cells.value, tb_bytes=tbb.value, dp_ms=dp.value, bt_ms=bt.value)

    def fetch(self):
        res = np.zeros(len(self.jobs), KSW_RES_DTYPE)
        cap = int((self.jobs["qlen"].astype(np.int64) + self.jobs["tlen"] + 2).sum()) + 16
        pool = np.zeros(cap, np.uint32)
        used = C.c_size_t(0)
        _chk(lib().wm_ksw_dev_fetch(self.ctx._h, self._h, res.ctypes.data, pool.ctypes.data, cap, C.byref(used)))
        return res, pool[:used.value]

    def free(self):
        if self._h:
            lib().wm_ksw_dev_free(self.ctx._h, self._h)
            self._h = None


def _device_switch(stem, stat_names, set_doc, stats_doc):
    """the three wrappers of one opt-in switch of the mapper: wm_set_<stem>_device, wm_<stem>_device_enabled and wm_<stem>_stats (one counter per name)"""
    def set_device(on):
        f = getattr(lib(), "wm_set_%s_device" % stem)
        f.argtypes = [C.c_int]
        f.restype = None
        f(int(on))

    def device_enabled():
        f = getattr(lib(), "wm_%s_device_enabled" % stem)
        f.restype = C.c_int
        return bool(f())

    def stats(reset=False):
        out = np.zeros(len(stat_names), np.uint64)
        f = getattr(lib(), "wm_%s_stats" % stem)
        f.argtypes = [C.c_void_p, C.c_int]
        f.restype = None
        f(out.ctypes.data, 1 if reset else 0)
        return dict(zip(stat_names, (int(x) for x in out)))

    set_device.__doc__, stats.__doc__ = set_doc, stats_doc
    for fn, name in ((set_device, "set_%s_device"), (device_enabled, "%s_device_enabled"), (stats, "%s_stats")):
        fn.__name__ = fn.__qualname__ = name % stem
    return set_device, device_enabled, stats


EXTRA_JOB_DTYPE = np.dtype([("q_off", np.uint32), ("t_off", np.uint32), ("cig_off", np.uint32), ("n_cigar", np.int32)])                       # wm_extra_job_t
EXTRA_POS_DTYPE = np.dtype([("qwin_off", np.int64), ("qwin_len", np.int32), ("q_pos", np.int32), ("rid", np.int32), ("t_pos", np.int32),
                            ("cig_off", np.uint32), ("n_cigar", np.int32)])                                                                      # wm_extra_pos_t
EXTRA_MAX_ABS = 1 << 30                                                                                                                          # WM_EXTRA_MAX_ABS
EXTRA_STAT_NAMES = ("deferred", "on_device", "on_host", "calls", "columns", "device_us")


def set_extra_routing(long_min_cols=-1, tile_cols=-1):
    """wm_extra_set_routing: from how many columns a final CIGAR is spread over one wavefront per tile, and the tile size (results never depend on it)"""
    lib().wm_extra_set_routing.argtypes = [C.c_int, C.c_int]
    lib().wm_extra_set_routing.restype = None
    lib().wm_extra_set_routing(long_min_cols, tile_cols)


def extra_tile_cols():
    lib().wm_extra_tile_cols.restype = C.c_int
    return int(lib().wm_extra_tile_cols())


set_extra_device, extra_device_enabled, extra_stats = _device_switch("extra", EXTRA_STAT_NAMES,
    """wm_set_extra_device: the mapper defers its regions' final scans (mm_update_extra's walk) to one batched device call per read (off by default;
    on < 0: back to what WM_EXTRA_DEV in the environment says). Read when a mapping call starts; results never depend on it.""",
    """wm_extra_stats: regions deferred / walked on the device / walked on the host while the switch was on, batched device calls, columns, microseconds""")


FIX_STAT_NAMES = ("deferred", "on_device", "on_host", "early_on_host", "calls", "device_us", "columns")


set_fix_device, fix_device_enabled, fix_stats = _device_switch("fix", FIX_STAT_NAMES,
    """wm_set_fix_device: the mapper defers BOTH halves of mm_update_extra — mm_fix_cigar and the scan — to one batched wm_fix_extra_batch_pos per read (off by
    default; on < 0: back to what WM_FIX_DEV in the environment says). Read when a mapping call starts; results never depend on it.""",
    """wm_fix_stats: regions whose fix was deferred / fixed on the device / fixed on the host by the batched request / fixed on the host early because an inversion
    test read them, batched device calls, microseconds, alignment columns walked by those calls""")


EQX_RES_DTYPE = np.dtype([("off", np.uint64), ("n_cigar", np.int32), ("in_place", np.int32)])                                                 # wm_eqx_res_t
EQX_STAT_NAMES = ("deferred", "on_device", "on_host", "calls", "columns", "device_us")


set_eqx_device, eqx_device_enabled, eqx_stats = _device_switch("eqx", EQX_STAT_NAMES,
    """wm_set_eqx_device: under MM_F_EQX the mapper defers the = / X rewriting of final CIGARs (mm_update_cigar_eqx) to one batched wm_eqx_batch_pos per read (off
    by default; on < 0: back to what WM_EQX_DEV in the environment says). Read when a mapping call starts; results never depend on it.""",
    """wm_eqx_stats: regions deferred / rewritten on the device / rewritten on the host by the batched request, batched device calls, M columns, microseconds""")


CS_RES_DTYPE = np.dtype([("off", np.uint64), ("len", np.uint32), ("pad", np.int32)])                                                       # wm_cs_res_t
CS_SHORT, CS_LONG, CS_MD = 0, 1, 2                                                                                                          # WM_CS_SHORT / _LONG / _MD
CS_STAT_NAMES = ("deferred", "on_device", "on_host", "calls", "bytes", "device_us")


set_cs_device, cs_device_enabled, cs_stats = _device_switch("cs", CS_STAT_NAMES,
    """wm_set_cs_device: under MM_F_OUT_CS / MM_F_OUT_MD the mapper has the bodies of a read's cs:Z / MD:Z tags produced by one batched wm_cs_batch_pos per read (off
    by default; on < 0: back to what WM_CS_DEV in the environment says). Read when a mapping call starts; results never depend on it.""",
    """wm_cs_stats: regions deferred / served on the device / served on the host by the batched request, batched device calls, bytes produced, microseconds""")


LL_JOB_DTYPE = np.dtype([("q_off", np.uint32), ("t_off", np.uint32), ("qlen", np.int32), ("tlen", np.int32), ("step", np.int8), ("pad", np.int8, 3)])      # wm_ll_job_t
LL_POS_DTYPE = np.dtype([("qwin_off", np.int64), ("qwin_len", np.int32), ("q_pos", np.int32), ("rid", np.int32), ("t_pos", np.int32), ("qlen", np.int32),
                         ("tlen", np.int32), ("step", np.int8), ("pad", np.int8, 7)])                                                           # wm_ll_pos_t
LL_MAX_LEN = 16384                                                                                                                          # WM_LL_MAX_LEN
LL_STAT_NAMES = ("deferred", "on_device", "on_host", "calls", "cells", "device_us")


def set_ksw_ll_routing(reg_max):
    """wm_ksw_ll_set_routing: up to how many positions of the padded query a ksw_ll job keeps its state in registers, 0..64 (results never depend on it)"""
    lib().wm_ksw_ll_set_routing.argtypes = [C.c_int]
    lib().wm_ksw_ll_set_routing.restype = None
    lib().wm_ksw_ll_set_routing(int(reg_max))


def ksw_ll_reg_max():
    lib().wm_ksw_ll_reg_max.restype = C.c_int
    return int(lib().wm_ksw_ll_reg_max())


set_ll_device, ll_device_enabled, ll_stats = _device_switch("ll", LL_STAT_NAMES,
    """wm_set_ll_device: the mapper files its ksw_ll_i16 jobs (inversion test, mm_align1_inv, splice end filter) with the batching hub, which serves them with batched
    wm_ksw_ll_batch_pos calls (off by default; on < 0: back to what WM_LL_DEV in the environment says). Read when a mapping call starts; results never depend on it.""",
    """wm_ll_stats: jobs deferred / served on the device / served on the host by the batched request, batched device calls, DP cells, microseconds""")


def set_ksw_routing(on=-1, rows4=-1, rows8=-1):
    """wm_ksw_set_routing: which alignments run on the stripe-pipelined multi-wave kernels (results never depend on it)"""
    lib().wm_ksw_set_routing.argtypes = [C.c_int, C.c_int, C.c_int]
    lib().wm_ksw_set_routing.restype = None
    lib().wm_ksw_set_routing(on, rows4, rows8)


def set_ksw_chain_routing(mode=-1, min_rows_exact=-1, bp=-1):
    """wm_ksw_set_chain_routing: which alignments run on the chained-workgroup kernels (results never depend on it)"""
    lib().wm_ksw_set_chain_routing.argtypes = [C.c_int, C.c_int, C.c_int]
    lib().wm_ksw_set_chain_routing.restype = None
    lib().wm_ksw_set_chain_routing(mode, min_rows_exact, bp)


def set_ksw_dual(on):
    """wm_ksw_set_dual: two alignments per wavefront for the gap-fill classes (results never depend on it)"""
    lib().wm_ksw_set_dual.argtypes = [C.c_int]
    lib().wm_ksw_set_dual.restype = None
    lib().wm_ksw_set_dual(int(on))


def ksw_dual_enabled():
    lib().wm_ksw_dual_enabled.restype = C.c_int
    return bool(lib().wm_ksw_dual_enabled())


def set_even_k(on):
    """wm_set_even_k: let mappers made from now on serve an index with an even k (off by default; on < 0: back to what WM_EVEN_K in the environment says)"""
    lib().wm_set_even_k.argtypes = [C.c_int]
    lib().wm_set_even_k.restype = None
    lib().wm_set_even_k(int(on))


def even_k_enabled():
    lib().wm_even_k_enabled.restype = C.c_int
    return bool(lib().wm_even_k_enabled())


def set_sketch_step_chunks(on):
    """wm_sketch_set_step_chunks: sketch long sequences chunk by chunk under -H / at an even k as well (1), or keep them on one wavefront each (0); on < 0: back
    to what WM_SKETCH_STEP_CHUNKS in the environment says. Results never depend on it."""
    lib().wm_sketch_set_step_chunks.argtypes = [C.c_int]
    lib().wm_sketch_set_step_chunks.restype = None
    lib().wm_sketch_set_step_chunks(int(on))


def sdust_stats(reset=False):
    """wm_sdust_stats: the -T filter's process-wide account since the last reset"""
    out = np.zeros(5, np.float64)
    lib().wm_sdust_stats.argtypes = [C.c_void_p, C.c_int]
    lib().wm_sdust_stats.restype = None
    lib().wm_sdust_stats(out.ctypes.data, 1 if reset else 0)
    return {"window_calls": int(out[0]), "kernel_ms": float(out[1]), "jobs": int(out[2]), "host_jobs": int(out[3]), "list_high": int(out[4])}


def exts2_stats(reset=False):
    """wm_exts2_stats: splice mode's alignment calls of the mapper and the groups they were split into, process-wide since the last reset"""
    out = np.zeros(2, np.uint64)
    lib().wm_exts2_stats.argtypes = [C.c_void_p, C.c_int]
    lib().wm_exts2_stats.restype = None
    lib().wm_exts2_stats(out.ctypes.data, 1 if reset else 0)
    return {"calls": int(out[0]), "groups": int(out[1])}


def arena_split_stats(reset=False):
    """wm_arena_split_stats: (batched calls of the mapper, or parts of one, refused for the arena and halved; parts finally issued), process-wide since the last reset"""
    out = np.zeros(2, np.uint64)
    lib().wm_arena_split_stats.argtypes = [C.c_void_p, C.c_int]
    lib().wm_arena_split_stats.restype = None
    lib().wm_arena_split_stats(out.ctypes.data, 1 if reset else 0)
    return int(out[0]), int(out[1])


def build_defines():
    """the kernel-variant defines the loaded library was compiled with (wm_build_defines)"""
    lib().wm_build_defines.restype = C.c_char_p
    return lib().wm_build_defines().decode()


STRIPE_TIMING_FIELDS = ("scan", "epoch", "cells", "wait_left", "book", "wait_right", "publish", "rows", "epochs", "total", "waves")


def stripe_timing(reset=True):
    """per-phase shader-clock cycles of the stripe-pipelined ksw kernel, summed over wavefronts since the last reset (wm_debug_stripe_timing; only in a
    library built with WM_KERNEL_DEFINES="WM_STRIPE_TIMING=1", WmError otherwise)"""
    out = np.zeros(16, np.uint64)
    lib().wm_debug_stripe_timing.argtypes = [C.c_void_p, C.c_int]
    _chk(lib().wm_debug_stripe_timing(out.ctypes.data, 1 if reset else 0))
    return {k: int(out[i]) for i, k in enumerate(STRIPE_TIMING_FIELDS)}


def pack_jobs(pairs, w=751, zdrop=400, end_bonus=-1, flag=0):
    """pairs: list of (query codes, target codes[, dict overrides]). Returns (jobs, seqs)."""
    jobs = np.zeros(len(pairs), KSW_JOB_DTYPE)
    chunks, off = [], 0
    for i, p in enumerate(pairs):
        q, t = np.asarray(p[0], np.uint8), np.asarray(p[1], np.uint8)
        o = dict(w=w, zdrop=zdrop, end_bonus=end_bonus, flag=flag)
        if len(p) > 2:
            o.update(p[2])
        jobs[i] = (off, off + len(q), len(q), len(t), o["w"], o["zdrop"], o["end_bonus"], o["flag"])
        chunks += [q, t]
        off += len(q) + len(t)
    seqs = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    return jobs, seqs


# ---- index + mapper ------------------------------------------------------------------------------------
# wm_window_job_t / wm_window_res_t of include/wm_gpu.h
WINDOW_JOB = np.dtype([("seq_off", "<i8"), ("stage_off", "<u8"), ("pre_off", "<u8"), ("len", "<i4"), ("n_pre", "<i4"),
                       ("max_dist_x", "<i4"), ("min_dist_x", "<i4"), ("max_dist_y", "<i4"), ("bw", "<i4"), ("max_skip", "<i4"), ("max_iter", "<i4"), ("min_cnt", "<i4"), ("min_sc", "<i4"),
                       ("gap_scale", "<f4"), ("is_cdna", "<i4")])
WINDOW_RES = np.dtype([("n_anchors", "<i4"), ("rep_len", "<i4"), ("n_mini", "<i4"), ("n_u", "<i4"), ("n_v", "<i4"), ("u_off", "<u4"), ("a_off", "<u4")])


def _bind_map(L):
    if getattr(L, "_wm_map_bound", False):
        return
    L.wm_index_build.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.wm_index_destroy.argtypes = [C.c_void_p]
    L.wm_index_upload.argtypes = [C.c_void_p, C.c_void_p]
    L.wm_index_n_seq.argtypes = [C.c_void_p]
    L.wm_index_seq_name.restype = C.c_char_p
    L.wm_index_seq_name.argtypes = [C.c_void_p, C.c_int]
    L.wm_index_seq_len.argtypes = [C.c_void_p, C.c_int]
    L.wm_index_n_minimizers.restype = C.c_uint64
    L.wm_index_n_minimizers.argtypes = [C.c_void_p]
    L.wm_mapper_create.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_void_p)]
    L.wm_mapper_destroy.argtypes = [C.c_void_p]
    L.wm_mapper_set_threads.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.wm_map_reads.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p,
                               C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.wm_map_reads_slot.argtypes = [C.c_void_p, C.c_int] + list(L.wm_map_reads.argtypes[1:])
    L.wm_mapper_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.wm_sam_header.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
    L.wm_last_aux_ms.restype = C.c_float
    L.wm_last_aux_ms.argtypes = [C.c_void_p]
    L.wm_write_repetitive_kmers.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_char_p, C.POINTER(C.c_uint64)]
    L.wm_index_export.argtypes = [C.c_void_p] + [C.c_void_p] * 8
    L.wm_index_import.argtypes = [C.c_void_p] * 8 + [C.POINTER(C.c_void_p)]
    L._wm_map_bound = True


def write_repetitive_kmers(fasta, k, out_path, distinct=0.9998):
    """Write the -W list of `fasta` (see include/wm_gpu.h). Returns the number of k-mers written."""
    L = lib()
    _bind_map(L)
    n = C.c_uint64()
    _chk(L.wm_write_repetitive_kmers(os.fsencode(fasta), k, distinct, os.fsencode(out_path), C.byref(n)))
    return int(n.value)


def write_repetitive_kmers_gpu(ctx, fasta, k, out_path, distinct=0.9998):
    """The -W list counted on the device (wm_write_repetitive_kmers_gpu). Returns (number of k-mers written, stats dict)."""
    L = lib()
    L.wm_write_repetitive_kmers_gpu.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_char_p, C.POINTER(C.c_uint64), C.c_void_p]
    n = C.c_uint64()
    st = np.zeros(4, np.float64)
    _chk(L.wm_write_repetitive_kmers_gpu(ctx._h, os.fsencode(fasta), k, distinct, os.fsencode(out_path), C.byref(n), st.ctypes.data))
    return int(n.value), {"read_encode_s": float(st[0]), "device_s": float(st[1]), "write_s": float(st[2]), "distinct_kmers": int(st[3])}


_EXPORT_DTYPES = (np.uint32, np.uint64, np.uint64, np.uint64, np.uint8, np.uint64, np.uint8)


class MapOpt(C.Structure):
    """wm_mapopt_t (include/wm_gpu.h) = the mirrored fields of mm_mapopt_t, in that order"""
    _fields_ = [("flag", C.c_int64)] + [(n, C.c_int32) for n in ("seed", "sdust_thres", "max_qlen", "bw", "max_gap", "max_gap_ref", "min_gap_ref", "max_frag_len",
                                                                  "max_chain_skip", "max_chain_iter", "min_cnt", "min_chain_score")] + \
               [("chain_gap_scale", C.c_float)] + [(n, C.c_int32) for n in ("SVaware", "SVawareMinReadLength", "suffixSampleOffset", "min_mapq")] + [("min_qcov", C.c_float)] + \
               [(n, C.c_int32) for n in ("minPrefixLength", "maxPrefixLength")] + [("prefixIncrementFactor", C.c_float)] + \
               [(n, C.c_int32) for n in ("stage2_bw", "stage2_zdrop_inv", "stage2_max_gap")] + [("mask_level", C.c_float), ("mask_len", C.c_int32), ("pri_ratio", C.c_float), ("best_n", C.c_int32)] + \
               [(n, C.c_int32) for n in ("max_join_long", "max_join_short", "min_join_flank_sc")] + [("min_join_flank_ratio", C.c_float), ("alt_drop", C.c_float)] + \
               [(n, C.c_int32) for n in ("a", "b", "q", "e", "q2", "e2", "sc_ambi", "zdrop", "zdrop_inv", "end_bonus", "min_dp_max", "min_ksw_len")] + \
               [("max_clip_ratio", C.c_float), ("mid_occ_frac", C.c_float)] + [(n, C.c_int32) for n in ("min_mid_occ", "mid_occ", "max_occ")] + [("mini_batch_size", C.c_int64), ("max_sw_mat", C.c_int64)] + \
               [(n, C.c_int32) for n in ("noncan", "junc_bonus", "anchor_ext_len", "anchor_ext_shift")]


def mapopt_preset(preset):
    """wm_mapopt_preset = mm_set_opt(0) + mm_set_opt(preset): -> (MapOpt, k, w)"""
    L = lib()
    L.wm_mapopt_preset.argtypes = [C.c_char_p, C.POINTER(MapOpt), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    o = MapOpt(); k = C.c_int(); w = C.c_int()
    _chk(L.wm_mapopt_preset((preset or "").encode(), C.byref(o), C.byref(k), C.byref(w)))
    return o, k.value, w.value


def build_index_parts(fasta, kmer_file, k, w, batch_bases, n_threads=8):
    """wm_index_build_parts: the reference indexed in parts of `batch_bases` (the reference's -I) -> list of Index"""
    L = lib()
    _bind_map(L)
    L.wm_index_build_parts.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]
    cap = 4096
    arr = (C.c_void_p * cap)()
    n = C.c_int()
    _chk(L.wm_index_build_parts(os.fsencode(fasta), os.fsencode(kmer_file) if kmer_file else None, k, w, n_threads, batch_bases, arr, cap, C.byref(n)))
    return [Index(_handle=C.c_void_p(arr[i])) for i in range(n.value)]


def map_file_multi(mappers, reads_path, out_path, mini_batch_bases=0):
    """wm_map_file_multi: the file loop over several mappers (one per GPU), two lanes each, records in input order"""
    L = lib()
    L.wm_map_file_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int64, C.c_void_p]
    arr = (C.c_void_p * len(mappers))(*[m._h for m in mappers])
    st = np.zeros(6, np.float64)
    _chk(L.wm_map_file_multi(arr, len(mappers), os.fsencode(reads_path), os.fsencode(out_path), mini_batch_bases, st.ctypes.data))
    return dict(zip(("reads", "bases", "batches", "t_read", "t_map", "t_write"), (float(x) for x in st)))


def map_file_split(ctx, parts, opt, n_threads, reads_path, out_path, mini_batch_bases=0):
    """wm_map_file_split: the reads against every index part in turn, hits merged like `--split-prefix` (mm_split_merge)"""
    L = lib()
    L.wm_map_file_split.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(MapOpt), C.c_int, C.c_char_p, C.c_char_p, C.c_int64, C.c_void_p]
    arr = (C.c_void_p * len(parts))(*[p._h for p in parts])
    st = np.zeros(6, np.float64)
    _chk(L.wm_map_file_split(ctx._h, len(parts), arr, C.byref(opt), n_threads, os.fsencode(reads_path), os.fsencode(out_path), mini_batch_bases, st.ctypes.data))
    return dict(zip(("reads", "bases", "batches", "t_read", "t_map", "t_write"), (float(x) for x in st)))


def map_file_split_fasta(ctx, fasta, kmer_file, k, w, batch_bases, opt, n_threads, reads_path, out_path, on_device=False, build_threads=8, mini_batch_bases=0):
    """wm_map_file_split_fasta: like `winnowmap -I <batch_bases> --split-prefix`, one index part in memory at a time (built when its turn comes)"""
    L = lib()
    L.wm_map_file_split_fasta.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(MapOpt), C.c_int,
                                          C.c_char_p, C.c_char_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int)]
    st = np.zeros(6, np.float64)
    n = C.c_int()
    _chk(L.wm_map_file_split_fasta(ctx._h, os.fsencode(fasta), os.fsencode(kmer_file) if kmer_file else None, k, w, build_threads, batch_bases, 1 if on_device else 0,
                                   C.byref(opt), n_threads, os.fsencode(reads_path), os.fsencode(out_path), mini_batch_bases, st.ctypes.data, C.byref(n)))
    d = dict(zip(("reads", "bases", "batches", "t_read", "t_map", "t_write"), (float(x) for x in st)))
    d["parts"] = n.value
    return d


class SplitRun:
    """wm_split_begin / wm_split_add_part / wm_split_finish: a reference indexed in parts, one part at a time (src/main.c:398-429)"""

    def __init__(self, ctx, opt, k, w, n_threads, reads_path, mini_batch_bases=0):
        L = lib()
        L.wm_split_begin.argtypes = [C.c_void_p, C.POINTER(MapOpt), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.wm_split_add_part.argtypes = [C.c_void_p, C.c_void_p]
        L.wm_split_finish.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        L.wm_split_abort.argtypes = [C.c_void_p]
        L.wm_split_abort.restype = None
        self._h = C.c_void_p()
        _chk(L.wm_split_begin(ctx._h, C.byref(opt), k, w, n_threads, os.fsencode(reads_path), mini_batch_bases, C.byref(self._h)))

    def add_part(self, idx):
        _chk(lib().wm_split_add_part(self._h, idx._h))

    def finish(self, out_path):
        st = np.zeros(6, np.float64)
        h, self._h = self._h, None
        _chk(lib().wm_split_finish(h, os.fsencode(out_path), st.ctypes.data))
        return dict(zip(("reads", "bases", "batches", "t_read", "t_map", "t_write"), (float(x) for x in st)))

    def abort(self):
        if self._h:
            lib().wm_split_abort(self._h)
            self._h = None


class Index:
    """Reference index (host build, mm_idx_gen semantics); `upload(ctx)` copies the flat arrays to HBM."""

    def __init__(self, fasta=None, kmer_file=None, k=15, w=50, n_threads=8, _handle=None, hpc=False):
        L = lib()
        _bind_map(L)
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
            return
        L.wm_index_build_flag.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        _chk(L.wm_index_build_flag(os.fsencode(fasta), os.fsencode(kmer_file) if kmer_file else None, k, w, 1 if hpc else 0, n_threads, C.byref(self._h)))      # hpc: MM_I_HPC (-H)

    @staticmethod
    def build_on_device(ctx, fasta, kmer_file=None, k=15, w=50, n_threads=8, hpc=False):
        """wm_index_build_gpu[_flag]: the reference is sketched on the device (one wavefront per contig, per chunk of a long one). Returns (Index, stats dict)."""
        L = lib()
        _bind_map(L)
        L.wm_index_build_gpu_flag.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
        h = C.c_void_p()
        st = np.zeros(4, np.float64)
        _chk(L.wm_index_build_gpu_flag(ctx._h, os.fsencode(fasta), os.fsencode(kmer_file) if kmer_file else None, k, w, 1 if hpc else 0, n_threads, C.byref(h), st.ctypes.data))
        L.wm_last_aux_ms.restype = C.c_float
        L.wm_last_aux_ms.argtypes = [C.c_void_p]
        return Index(_handle=h), {"read_pack_s": float(st[0]), "device_sketch_s": float(st[1]), "table_s": float(st[2]), "minimizers": int(st[3]),
                                  "table_on_device_s": float(L.wm_last_aux_ms(ctx._h)) * 1e-3}       # (< 0: the table was built by the host)

    def read_junc_bed(self, path):
        """--junc-bed: annotated introns for splice mode's junction bonus (wm_index_read_junc_bed = mm_idx_bed_read, src/index.c:756)"""
        L = lib()
        L.wm_index_read_junc_bed.argtypes = [C.c_void_p, C.c_char_p]
        _chk(L.wm_index_read_junc_bed(self._h, os.fsencode(path)))

    def export_arrays(self):
        """(sizes9, [S, hkey, hval, P, bloom, seq_meta, names]) as numpy arrays — the payload of the RCCL broadcast."""
        L = lib()
        sizes = np.zeros(9, np.uint64)
        _chk(L.wm_index_export(self._h, sizes.ctypes.data, None, None, None, None, None, None, None))
        n = [int(sizes[0]), int(sizes[1]), int(sizes[1]), int(sizes[2]), int(sizes[3]), 2 * int(sizes[4]), int(sizes[5])]
        arrs = [np.zeros(max(m, 1), dt) for m, dt in zip(n, _EXPORT_DTYPES)]
        _chk(L.wm_index_export(self._h, sizes.ctypes.data, *[a.ctypes.data for a in arrs]))
        return sizes, arrs

    @staticmethod
    def from_arrays(sizes, arrs):
        L = lib()
        _bind_map(L)
        h = C.c_void_p()
        arrs = [np.ascontiguousarray(a, dt) for a, dt in zip(arrs, _EXPORT_DTYPES)]
        sizes = np.ascontiguousarray(sizes, np.uint64)
        _chk(L.wm_index_import(sizes.ctypes.data, *[a.ctypes.data for a in arrs], C.byref(h)))
        return Index(_handle=h)

    def save(self, path):
        """write the reference's MMI index file format"""
        L = lib()
        L.wm_index_save.argtypes = [C.c_void_p, C.c_char_p]
        _chk(L.wm_index_save(self._h, path.encode()))

    @staticmethod
    def load(path, kmer_file=None):
        L = lib()
        _bind_map(L)
        L.wm_index_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        _chk(L.wm_index_load(path.encode(), kmer_file.encode() if kmer_file else None, C.byref(h)))
        return Index(_handle=h)

    def upload(self, ctx):
        _chk(lib().wm_index_upload(ctx._h, self._h))

    def upload_dev(self, ctx, d_ptrs, src_device):
        """wm_index_upload_dev: the flat arrays S, hkey, hval, P, bloom from DEVICE pointers (e.g. the receive buffers of the RCCL broadcast) on src_device"""
        L = lib()
        L.wm_index_upload_dev.argtypes = [C.c_void_p, C.c_void_p] + [C.c_void_p] * 5 + [C.c_int]
        _chk(L.wm_index_upload_dev(ctx._h, self._h, *[C.c_void_p(int(p)) for p in d_ptrs], int(src_device)))

    def upload_peer(self, dst_ctx, src_ctx):
        """wm_index_upload_peer: the copy context `src_ctx` holds goes to `dst_ctx` (any GPU of the node), device to device"""
        L = lib()
        L.wm_index_upload_peer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(L.wm_index_upload_peer(dst_ctx._h, self._h, src_ctx._h))

    @property
    def n_minimizers(self):
        if not self._h:
            raise RuntimeError("the index has been closed")
        return int(lib().wm_index_n_minimizers(self._h))

    def names(self):
        L = lib()
        return [L.wm_index_seq_name(self._h, i).decode() for i in range(L.wm_index_n_seq(self._h))]

    def query_key(self, name):
        """(lo, eq) of a query name for THIS index: lo = distinct contig names that are strcmp-smaller, eq = the name is a contig's. What the device compares
        instead of skip_seed's strcmp(qname, contig name) (src/map.c:132-154) in self / all-vs-all mapping; wm_index_query_key."""
        return tuple(int(x) for x in self.query_keys([name])[0])

    def query_keys(self, names):
        L = lib()
        L.wm_index_query_key.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        out = np.zeros((len(names), 2), np.uint32)
        for i, nm in enumerate(names):
            _chk(L.wm_index_query_key(self._h, nm if isinstance(nm, bytes) else nm.encode(), out[i:].ctypes.data))
        return out

    def close(self):
        if self._h:
            lib().wm_index_destroy(self._h)
            self._h = C.c_void_p()


MM_F_CIGAR, MM_F_OUT_SAM, MM_F_OUT_CG = 0x4, 0x8, 0x20
# self / all-vs-all mapping (src/minimap.h:9-31, skip_seed src/map.c:132-154): -D, --dual=no, -P, --no-long-join; -X is all four (src/main.c)
MM_F_NO_DIAG, MM_F_NO_DUAL, MM_F_NO_LJOIN, MM_F_ALL_CHAINS = 0x1, 0x2, 0x400, 0x800000
MM_F_AVA = MM_F_ALL_CHAINS | MM_F_NO_DIAG | MM_F_NO_DUAL | MM_F_NO_LJOIN
# --heap-sort=yes (src/main.c:261-262): the seeds of a query merged through a binary heap (collect_seed_hits_heap, src/map.c:156-220) instead of collected and
# radix-sorted; the two orders differ where two anchors share x. Served by the seeding and window operations and by the mapper
MM_F_HEAP_SORT = 0x400000
MM_F_OUT_CS = 0x040           # --cs: the cs:Z tag (write_cs_core, src/format.c:141-187); with MM_F_OUT_CS_LONG (--cs=long) identical stretches are spelled out
MM_F_OUT_CS_LONG = 0x800
MM_F_OUT_MD = 0x1000000       # --MD: the MD:Z tag (write_MD_core, src/format.c:189-218); it wins over --cs when both are set
MM_F_EQX = 0x4000000          # --eqx: M ops come out as runs of = / X (mm_update_cigar_eqx, src/align.c:169-238)
STAT_NAMES = ("super_steps", "ksw_jobs", "chain_jobs", "seed_jobs", "sketch_jobs", "dp_cells", "ksw_kernel_us", "aux_kernel_us", "read_bases")


class Mapper:
    """The batched replacement of kt_for(worker_for) (src/map.c:1164): maps a list of reads in one call."""

    def __init__(self, ctx, index, preset="map-ont", flag=MM_F_CIGAR | MM_F_OUT_CG):
        L = lib()
        _bind_map(L)
        self.ctx, self.index = ctx, index
        self._h = C.c_void_p()
        _chk(L.wm_mapper_create(ctx._h, index._h, preset.encode() if preset else None, flag, C.byref(self._h)))

    def set_threads(self, n_threads, arena_bytes_per_thread=0):
        _chk(lib().wm_mapper_set_threads(self._h, n_threads, arena_bytes_per_thread))

    @staticmethod
    def marshal(names, seqs):
        """the C arrays wm_map_reads takes (name pointers, sequence pointers, lengths): building them from Python lists costs tens of
        milliseconds per 10^5 reads, which a caller timing the mapper does once, outside its clock"""
        n = len(seqs)
        nm = (C.c_char_p * n)(*[x if isinstance(x, bytes) else x.encode() for x in names])
        sq = (C.c_char_p * n)(*seqs)
        lens = np.array([len(s) for s in seqs], np.int32)
        return n, nm, sq, lens, (names, seqs)      # (the lists keep the pointed-to bytes alive)

    def map(self, names, seqs=None, copy_text=True, slot=0):
        """names: list of str/bytes; seqs: list of bytes (ASCII) — or names = the tuple Mapper.marshal() returned. Returns
        (text, hits[n_hits,16], cigars, first[n+1]).
        copy_text=False returns the text LENGTH instead of a Python copy of the records (they stay in the library's buffer).
        slot (0 .. WM_MAX_SLOTS - 1 = 3): calls on different slots may run concurrently from different threads (wm_map_reads_slot; ctypes releases the GIL)."""
        L = lib()
        n, nm, sq, lens, _keep = names if seqs is None else Mapper.marshal(names, seqs)
        text, tlen = C.c_char_p(), C.c_size_t()
        hits, cig, first = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(L.wm_map_reads_slot(self._h, slot, n, nm, sq, lens.ctypes.data, C.byref(text), C.byref(tlen), C.byref(hits), C.byref(cig), C.byref(first)))
        fa = np.ctypeslib.as_array(C.cast(first, C.POINTER(C.c_int64)), shape=(n + 1,)).copy()
        nh = int(fa[n])
        ha = np.ctypeslib.as_array(C.cast(hits, C.POINTER(C.c_int32)), shape=(nh, 16)).copy() if nh else np.zeros((0, 16), np.int32)
        if not copy_text:
            return tlen.value, ha, None, fa
        nc = int(ha[:, 7].sum()) if nh else 0
        ca = np.ctypeslib.as_array(C.cast(cig, C.POINTER(C.c_uint32)), shape=(nc,)).copy() if nc else np.zeros(0, np.uint32)
        return C.string_at(text, tlen.value), ha, ca, fa

    def rep_len_defined(self, slot=0):
        """uint8 per read of the slot's last map() call: 1 where rep_len (hence MAPQ and rl:i) is defined by the reference itself (wm_map_reads_rep_len_defined)"""
        L = lib()
        L.wm_map_reads_rep_len_defined.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        p, n = C.c_void_p(), C.c_size_t()
        _chk(L.wm_map_reads_rep_len_defined(self._h, slot, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint8)

    def stats(self):
        a = np.zeros(9, np.uint64)
        lib().wm_mapper_stats(self._h, a.ctypes.data)
        return dict(zip(STAT_NAMES, (int(x) for x in a)))

    def map_file(self, reads_path, out_path, mini_batch_bases=0):
        """FASTA/FASTQ(.gz) -> PAF/SAM file, mini-batch pipeline (wm_map_file). Returns the stats dict."""
        L = lib()
        L.wm_map_file.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_void_p]
        st = np.zeros(6, np.float64)
        _chk(L.wm_map_file(self._h, reads_path.encode(), out_path.encode(), mini_batch_bases, st.ctypes.data))
        return dict(zip(("reads", "bases", "batches", "t_read", "t_map", "t_write"), (float(x) for x in st)))

    def kernel_stats(self):
        """per ksw kernel class: dict class -> (ms, cells, launches)"""
        out = np.zeros(3 * 64, np.float64)
        n = C.c_int()
        lib().wm_mapper_kernel_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        _chk(lib().wm_mapper_kernel_stats(self._h, out.ctypes.data, len(out), C.byref(n)))
        return {k: (float(out[3 * k]), float(out[3 * k + 1]), int(out[3 * k + 2])) for k in range(n.value)}

    def kernel_union(self, since_ms=0.0):
        """(dict class -> ms with at least one launch of the class running since `since_ms`, device clock now in ms)"""
        ncl = int(lib().wm_ksw_n_classes())
        out = np.zeros(max(64, ncl), np.float64)
        now = C.c_double()
        lib().wm_mapper_kernel_union.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        _chk(lib().wm_mapper_kernel_union(self._h, float(since_ms), out.ctypes.data, len(out), C.byref(now)))
        return {k: float(out[k]) for k in range(ncl)}, now.value

    def host_stats(self):
        """host time accounting since the mapper was created (wm_mapper_host_stats), seconds summed over the worker threads"""
        a = np.zeros(24, np.float64)
        lib().wm_mapper_host_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _chk(lib().wm_mapper_host_stats(self._h, a.ctypes.data, len(a)))
        ops = ("window", "seed", "chain", "ksw")     # (the mapper issues fused window calls and ksw calls; the per-stage slots stay 0)
        return {"cpu_glue_s": float(a[0]), "idle_wall_s": float(a[1]), "cpu_batched_s": {o: float(a[2 + i]) for i, o in enumerate(ops)},
                "wall_batched_s": {o: float(a[6 + i]) for i, o in enumerate(ops)}, "batched_calls": {o: int(a[10 + i]) for i, o in enumerate(ops)},
                "map_wall_s": float(a[14]), "format_wall_s": float(a[15]), "threads": int(a[16]), "cpu_help_s": float(a[17]),
                "glue_wall_s": float(a[18]), "lock_wait_wall_s": float(a[19]), "workers_wall_s": float(a[20])}

    def close(self):
        if self._h:
            lib().wm_mapper_destroy(self._h)
            self._h = C.c_void_p()
