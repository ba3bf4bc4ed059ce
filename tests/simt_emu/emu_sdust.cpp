// tests/simt_emu/emu_sdust.cpp — TEST INFRASTRUCTURE ONLY.
// The two kernels of the -T filter (winnowmap_amd/csrc/sdust_kernel.h: sdust_wave, dust_filter_wave) on the host wavefront emulator, and the host
// restatement (winnowmap_amd/csrc/host/wm_sdust.h), through a C ABI for ctypes. WM_SDUST_CAP is a build define: tests/test_sdust_emu.py builds a
// second library with 64 entries so that the list of perfect intervals overflows and the job is finished by the host restatement.
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "sdust_kernel.h"            // winnowmap_amd/csrc
#include "host/wm_sdust.h"
#include <vector>

extern "C" {

int emu_sdust_cap(void) { return WM_SDUST_CAP; }

// sdust_wave over codes[0 .. len) — staged bytes, or (packed != 0) the same bases inside a packed read buffer at a base offset that is no multiple of
// 64. iv_out: 2 * iv_cap ints. Returns the number of intervals, -1 on overflow; *high = the largest list of perfect intervals held.
int emu_sdust(const uint8_t *codes, int len, int T, int packed, int32_t *iv_out, int iv_cap, int32_t *high)
{
	std::vector<int> lds((size_t)wmk::SDUST_LDS_INTS);
	std::vector<uint8_t> buf;
	std::vector<uint64_t> pk(1), nm(1);
	long long soff = 0;
	const uint8_t *seqs = codes;
	if (packed) {
		const int lead = 37;
		buf.assign((size_t)lead + (size_t)len + 5, 2);
		for (int i = 0; i < len; ++i) buf[(size_t)lead + i] = codes[i];
		pk.assign(wm_pk_words(buf.size()), 0); nm.assign(wm_nm_words(buf.size()), 0);
		wm_pack_codes(buf.data(), buf.size(), pk.data(), nm.data());
		soff = (long long)(WM_RD_PACKED_BIT | (uint64_t)lead);
		seqs = 0;
	}
	int hi = 0;
	simt::exec_mask() = ~0ull;
	const int n = wmk::sdust_wave(seqs, pk.data(), nm.data(), soff, len, T, lds.data(), WM_SDUST_CAP, (int*)iv_out, iv_cap, &hi);
	*high = hi;
	return n;
}

// dust_filter_wave in place on the minimizers (x, y); returns the new size
int emu_dust_filter(uint64_t *mx, uint64_t *my, int n, const int32_t *iv, int n_iv)
{
	std::vector<wm128_t> a((size_t)n + 1);
	for (int i = 0; i < n; ++i) a[i].x = mx[i], a[i].y = my[i];
	simt::exec_mask() = ~0ull;
	const int k = wmk::dust_filter_wave(a.data(), n, (const int*)iv, n_iv);
	for (int i = 0; i < k; ++i) mx[i] = a[i].x, my[i] = a[i].y;
	return k;
}

// the host restatement: intervals (returns how many there are; the first iv_cap are written) and the squeeze
int host_sdust(const uint8_t *codes, int len, int T, int32_t *iv_out, int iv_cap, int32_t *high)
{
	std::vector<wm::DustIv> iv;
	*high = wm::sdust_intervals(codes, len, T, iv);
	for (size_t i = 0; i < iv.size() && (int)i < iv_cap; ++i) iv_out[2 * i] = iv[i].st, iv_out[2 * i + 1] = iv[i].en;
	return (int)iv.size();
}

int host_dust_filter(uint64_t *mx, uint64_t *my, int n, const int32_t *iv, int n_iv)
{
	std::vector<wm::m128> a((size_t)n + 1);
	for (int i = 0; i < n; ++i) a[i].x = mx[i], a[i].y = my[i];
	const int k = wm::dust_filter(a.data(), n, (const wm::DustIv*)iv, n_iv);
	for (int i = 0; i < k; ++i) mx[i] = a[i].x, my[i] = a[i].y;
	return k;
}

// one job as the device serves it: the wavefront's intervals, or — when its list overflowed — the host's, then the squeeze by the wavefront.
// *fell_back = 1 when the host finished the intervals.
int emu_dust_job(const uint8_t *codes, int len, int T, uint64_t *mx, uint64_t *my, int n, int32_t *fell_back)
{
	std::vector<int32_t> iv(2 * ((size_t)len + 2));
	int32_t high = 0;
	int n_iv = emu_sdust(codes, len, T, 0, iv.data(), len + 1, &high);
	*fell_back = n_iv < 0;
	if (n_iv < 0) {
		std::vector<wm::DustIv> h;
		wm::sdust_intervals(codes, len, T, h);
		iv.resize(2 * h.size() + 2);
		for (size_t i = 0; i < h.size(); ++i) iv[2 * i] = h[i].st, iv[2 * i + 1] = h[i].en;
		n_iv = (int)h.size();
	}
	return emu_dust_filter(mx, my, n, iv.data(), n_iv);
}

} // extern "C"
