// chain_fill.h — the kernels of mm_chain_dp's score fill (src/chain.c:45-90; seedchain_kernel.h: chain_wave / chain_block / chain_block_wide) and the ONE plan that
// launches them, for the stand-alone call (wm_index.hip: wm_chain_batch) and the window call (wm_window.hip: window_launch). Not seen by the emulator.
// A block serves jobs[list[blockIdx.x]] and leaves when `count` is non-null and blockIdx.x >= *count: wm_chain_batch passes a class's stretch of its host-sorted order
// with an exact grid and no count, the window call the lists and counts its sort kernels wrote on the device with a grid of n.
// Every kernel raises its wave priority (wm_rt.h). Before this header only the window call's copies did: for the stand-alone call that is the one difference, and a
// priority cannot change a result. The raise comes AFTER the job record is read: uniform loads behind s_setprio are compiled as per-lane loads (the builtin seems to
// count as a possible store) — the job's fields in ~19 vector registers instead of scalar ones (profiles/seedfill_share_resources.txt).
#pragma once
#include "wm_rt.h"
#include "simt.h"
#include "seedchain_kernel.h"

// the LDS window of W anchors (28 B each: x, y, f, p, t), the workgroup fills' publish area behind it, and the job's slab in fpvt: f | p | v (extraction) | t
struct ChainFillMem {
	uint64_t *sx, *sy; int *sf, *sp, *st, *pub, *gf, *gp, *gt;
	__device__ __forceinline__ ChainFillMem(unsigned char *smem, int W, int *fpvt, const wm_chain_job_t &jb)
		: sx((uint64_t*)smem), sy(sx + W), sf((int*)(sy + W)), sp(sf + W), st(sp + W), pub(st + W), gf(fpvt + jb.a_off * 4), gp(gf + jb.n), gt(gp + 2 * (size_t)jb.n) {}
};
// dynamic LDS of a fill: the window, and for a workgroup fill the publish area of `tiles` tiles (69 ints each; chain_block: one per wavefront, chain_block_wide: wavefronts x KT)
inline size_t chain_fill_lds(int W, int tiles) { return (size_t)W * 28 + (tiles ? (size_t)tiles * 69 * 4 + 64 : 0); }
// one wavefront per anchor set (chain_wave)
static __global__ __launch_bounds__(64) void chain_fill_kernel(const wm_chain_job_t *jobs, const int *list, const int *count, const wm128_t *anchors, int *fpvt, int W)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	if (count && (int)blockIdx.x >= *count) return;
	const wm_chain_job_t jb = jobs[list[blockIdx.x]];
	WM_SETPRIO(2);
	const ChainFillMem m(smem, W, fpvt, jb);
	wmk::chain_wave(jb, anchors, W, m.sx, m.sy, m.sf, m.sp, m.st, m.gf, m.gp, m.gt);
}
// large anchor sets: NWV wavefronts cooperate on one job (chain_block)
template <int NWV> __global__ __launch_bounds__(64 * NWV) void chain_fill_kernel_block(const wm_chain_job_t *jobs, const int *list, const int *count, const wm128_t *anchors, int *fpvt, int W)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	if (count && (int)blockIdx.x >= *count) return;
	const wm_chain_job_t jb = jobs[list[blockIdx.x]];
	WM_SETPRIO(2);
	const ChainFillMem m(smem, W, fpvt, jb);
	wmk::chain_block(jb, anchors, NWV, W, m.sx, m.sy, m.sf, m.sp, m.st, m.pub, m.gf, m.gp, m.gt);
}
// ... with the whole predecessor window of an anchor per step (chain_block_wide): blockDim / 64 wavefronts x KT tiles
template <int KT> __global__ __launch_bounds__(1024) void chain_fill_kernel_wide(const wm_chain_job_t *jobs, const int *list, const int *count, const wm128_t *anchors, int *fpvt, int W, int kt_first)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	if (count && (int)blockIdx.x >= *count) return;
	const wm_chain_job_t jb = jobs[list[blockIdx.x]];
	WM_SETPRIO(2);
	const ChainFillMem m(smem, W, fpvt, jb);
	wmk::chain_block_wide<KT>(jb, anchors, (int)(blockDim.x >> 6), kt_first, W, m.sx, m.sy, m.sf, m.sp, m.st, m.pub, m.gf, m.gp, m.gt);
}

// The dense fill (class 0) of a call. wide: chain_block_wide, waves x tiles tiles per step, kt_first of them per wavefront in an anchor's first step (seedchain_kernel.h);
// otherwise (WM_CHAIN_WIDE=0) chain_block with 8 wavefronts, the round-5 fill. chain_dense_env: the three switches as the environment has them now — WHEN they are read is
// the caller's business. WM_CHAIN_WIDE_GEOM=<wavefronts>x<tiles> (16x5 | 8x10 | 16x3 | 8x5 | 4x10; tools/chain_fill_probe.py), 16x5 on anything not instantiated.
struct ChainDense { bool wide; int waves, tiles, kt_first; };
inline ChainDense chain_dense_env(bool with_geom)
{
	ChainDense d = { !(getenv("WM_CHAIN_WIDE") && atoi(getenv("WM_CHAIN_WIDE")) == 0), 16, 5, 5 };
	if (with_geom) if (const char *g = getenv("WM_CHAIN_WIDE_GEOM")) sscanf(g, "%dx%d", &d.waves, &d.tiles);
	if ((d.tiles != 10 && d.tiles != 3 && d.tiles != 5) || d.waves < 1 || d.waves > 16 || d.waves * d.tiles > 128) { d.waves = 16; d.tiles = 5; }      // (the instantiated tile counts; chain_block_wide: NT <= 128)
	d.kt_first = getenv("WM_CHAIN_WIDE_FIRST") ? std::min(d.tiles, std::max(1, atoi(getenv("WM_CHAIN_WIDE_FIRST")))) : d.tiles;
	return d;
}
// one class of a call: `grid` blocks over `list` (0 = the class is not launched), `count` as the kernels take it
struct ChainFillList { const int *list, *count; int grid; };
// queues the fills of the four classes on `s`: 0 dense (a workgroup, W 4096) | 1 large sparse (1 wavefront, W 1024) | 2 n <= 1024 (W 1024) | 3 n <= 256 (W 256)
inline int chain_fill_launch(hipStream_t s, const wm_chain_job_t *jobs, const wm128_t *anchors, int *fpvt, const ChainFillList (&cls)[4], const ChainDense &d)
{
	constexpr int NWV = 8, LDS_MAX = 160 * 1024;
	const ChainFillList &l = cls[0];
	auto wide = [&](auto kt) -> int {
		constexpr int KT = decltype(kt)::value;
		HIPCHK(hipFuncSetAttribute((const void*)chain_fill_kernel_wide<KT>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
		hipLaunchKernelGGL(chain_fill_kernel_wide<KT>, dim3(l.grid), dim3(64 * d.waves), chain_fill_lds(4096, d.waves * KT), s, jobs, l.list, l.count, anchors, fpvt, 4096, d.kt_first);
		return WM_OK;
	};
	if (l.grid && d.wide) {
		if (const int rc = d.tiles == 10 ? wide(std::integral_constant<int, 10>()) : d.tiles == 3 ? wide(std::integral_constant<int, 3>()) : wide(std::integral_constant<int, 5>())) return rc;
	} else if (l.grid) {
		HIPCHK(hipFuncSetAttribute((const void*)chain_fill_kernel_block<NWV>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
		hipLaunchKernelGGL(chain_fill_kernel_block<NWV>, dim3(l.grid), dim3(64 * NWV), chain_fill_lds(4096, NWV), s, jobs, l.list, l.count, anchors, fpvt, 4096);
	}
	HIPCHK(hipFuncSetAttribute((const void*)chain_fill_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
	for (int k = 1; k < 4; ++k)
		if (cls[k].grid) hipLaunchKernelGGL(chain_fill_kernel, dim3(cls[k].grid), dim3(64), chain_fill_lds(k == 3 ? 256 : 1024, 0), s, jobs, cls[k].list, cls[k].count, anchors, fpvt, k == 3 ? 256 : 1024);
	return WM_OK;
}
