// tests/simt_emu/emu_selfmap.cpp — TEST INFRASTRUCTURE ONLY.
// The two seeding kernels with the name tables of self / all-vs-all mapping (skip_seed, src/map.c:132-154) on the host wavefront emulator, and the
// host's name ranking (winnowmap_amd/csrc/host/wm_names.h), through a C ABI for ctypes. Beside emu_driver.cpp, which knows nothing of names.
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "seedchain_kernel.h"        // winnowmap_amd/csrc
#include "window_kernel.h"
#include "host/wm_names.h"
#include <vector>

extern "C" {

// rank of every contig name; returns the number of distinct names
int emu_names_rank(int n, const char **names, uint32_t *rank)
{
	const wm::NameTable t = wm::rank_names((size_t)n, [&](uint32_t i) { return names[i]; });
	for (int i = 0; i < n; ++i) rank[i] = t.rank[i];
	return (int)t.sorted.size();
}

// key of a query name: lo_eq[0] = lo, lo_eq[1] = eq
int emu_names_key(int n, const char **names, const char *qname, uint32_t *lo_eq)
{
	const wm::NameTable t = wm::rank_names((size_t)n, [&](uint32_t i) { return names[i]; });
	const wm::NameKey k = wm::name_key(t, [&](uint32_t i) { return names[i]; }, qname);
	lo_eq[0] = k.lo; lo_eq[1] = k.eq;
	return 0;
}

// seed_wave with a name key; res_out = n_anchors, rep_len
int emu_self_seed(const uint64_t *hkey, const uint64_t *hval, const uint64_t *P, int hbits, const uint32_t *name_rank, const uint32_t *seq_len,
                  const uint64_t *mx, const uint64_t *my, int n_mini, int qlen, int max_occ, int flag, uint32_t q_lo, int q_eq,
                  uint64_t *ax, uint64_t *ay, int cap, int32_t *res_out)
{
	wm_index_view_t ix = { hkey, hval, P, hbits, 0, name_rank, seq_len };
	std::vector<wm128_t> mini(n_mini + 1), anc(cap + 1);
	for (int i = 0; i < n_mini; ++i) mini[i].x = mx[i], mini[i].y = my[i];
	wm_seed_job_t jb;
	memset(&jb, 0, sizeof(jb));
	jb.n_mini = n_mini; jb.qlen = qlen; jb.max_occ = max_occ; jb.cap = cap; jb.flag = flag; jb.q_lo = q_lo; jb.q_eq = q_eq;
	std::vector<int> occ(n_mini + 1);
	wm_seed_res_t res = { 0, 0 };
	simt::exec_mask() = ~0ull;
	wmk::seed_wave(ix, jb, mini.data(), anc.data(), occ.data(), &res);
	for (int i = 0; i < res.n_anchors && i < cap; ++i) ax[i] = anc[i].x, ay[i] = anc[i].y;
	res_out[0] = res.n_anchors; res_out[1] = res.rep_len;
	return 0;
}

// win_seed_wave with a name key: n_pre handed-in anchors first, then the seeded ones (unsorted); res_out = n_a, rep_len, err
int emu_self_win_seed(const uint64_t *hkey, const uint64_t *hval, const uint64_t *P, int hbits, const uint32_t *name_rank, const uint32_t *seq_len,
                      const uint64_t *mx, const uint64_t *my, int n_mini, int qlen, int max_occ, int flag, uint32_t q_lo, int q_eq,
                      int n_pre, const uint64_t *px, const uint64_t *py, uint64_t *ax, uint64_t *ay, int cap, int32_t *res_out)
{
	wm_index_view_t ix = { hkey, hval, P, hbits, 0, name_rank, seq_len };
	std::vector<wm128_t> mini(n_mini + 1), pre(n_pre + 1), pool(cap + 64);
	for (int i = 0; i < n_mini; ++i) mini[i].x = mx[i], mini[i].y = my[i];
	for (int i = 0; i < n_pre; ++i) pre[i].x = px[i], pre[i].y = py[i];
	wm_win_job_t jb;
	memset(&jb, 0, sizeof(jb));
	jb.seq_off = 0; jb.len = qlen; jb.n_pre = n_pre; jb.max_occ = max_occ; jb.seed_flag = flag; jb.q_lo = q_lo; jb.q_eq = q_eq;
	std::vector<int> occ(n_mini + 1), emit(n_mini + 1);
	std::vector<uint32_t> first(n_mini + 1);
	uint64_t used = 5;                          // (the pool is shared by the jobs of a call: this job does not start at 0)
	wm_win_res_t res;
	memset(&res, 0, sizeof(res));
	simt::exec_mask() = ~0ull;
	wmk::win_seed_wave(ix, jb, mini.data(), n_mini, pre.data(), occ.data(), first.data(), emit.data(), pool.data(), &used, (uint64_t)cap, &res);
	for (int i = 0; i < res.n_a; ++i) ax[i] = pool[res.a_off + i].x, ay[i] = pool[res.a_off + i].y;
	res_out[0] = res.n_a; res_out[1] = res.rep_len; res_out[2] = res.err;
	return 0;
}

} // extern "C"
