/*
 * TEST HARNESS ONLY (never part of libdaccord_hip.so): the wavefront primitives of daccord_amd/csrc/wave.hpp, each called
 * in isolation so that its result can be compared with a plain numpy restatement (tests/waveprobe_lib.py, tests/waveprobe_cases.py).
 * The bodies are written once and wrapped twice: probe.hip runs them as gfx950 kernels (one wavefront per workgroup, the DEVICE branch of
 * wave.hpp: DPP scans, ballot + mbcnt, readlane, __shfl), probe_host.cpp runs them under wave_run() of the 64-lane host wavefront
 * (wave_emul64.hpp's restatements).  All 64 lanes call every collective, and every lane writes its own result: a "uniform" result
 * is checked on all 64 lanes.
 */
#ifndef DACC_WAVEPROBE_BODY_HPP
#define DACC_WAVEPROBE_BODY_HPP
#include "../../daccord_amd/csrc/wave.hpp"

namespace dacc {

// ---- 32 bit scans, reductions and votes: out[field*64 + lane] ----
enum { WP32_SCAN_PRE = 0, WP32_SCAN_TOT, WP32_SUM, WP32_MAX, WP32_OR, WP32_FLAG_PRE, WP32_FLAG_TOT, WP32_BALLOT, WP32_ANY, WP32_LANEMASK_LT, WP32_FIELDS };
DEV void wp_body_u32(uint32_t const * vals, uint32_t const * flags, uint64_t * out)
{
	int const lane = wv_lane();
	uint32_t const v = vals[lane]; bool const p = flags[lane] != 0;
	uint32_t tot = 0, ftot = 0;
	uint32_t const pre = wv_scan_excl(v,tot);
	out[WP32_SCAN_PRE*64+lane] = pre; out[WP32_SCAN_TOT*64+lane] = tot;
	out[WP32_SUM*64+lane] = wv_sum(v);
	out[WP32_MAX*64+lane] = wv_max(v);
	out[WP32_OR*64+lane] = wv_or(v);
	uint32_t const fpre = wv_scan_flag(p,ftot);
	out[WP32_FLAG_PRE*64+lane] = fpre; out[WP32_FLAG_TOT*64+lane] = ftot;
	out[WP32_BALLOT*64+lane] = wv_ballot(p ? 1 : 0);
	out[WP32_ANY*64+lane] = wv_any(p ? 1 : 0) ? 1u : 0u;
	out[WP32_LANEMASK_LT*64+lane] = wv_lanemask_lt();
}

// ---- 64 bit reductions ----
enum { WP64_SUM = 0, WP64_MAX, WP64_MIN, WP64_OR, WP64_UNI, WP64_FIELDS };
DEV void wp_body_u64(uint64_t const * vals, uint64_t * out)
{
	int const lane = wv_lane();
	uint64_t const v = vals[lane];
	out[WP64_SUM*64+lane] = wv_sum64(v);
	out[WP64_MAX*64+lane] = wv_max64(v);
	out[WP64_MIN*64+lane] = wv_min64(v);
	out[WP64_OR*64+lane] = wv_or64(v);
	out[WP64_UNI*64+lane] = wv_uni64(v);
}

// ---- broadcasts (wave-uniform source lane bsrc) and shuffles (per-lane source lane src[lane]) ----
enum { WPX_BCAST = 0, WPX_BCAST64, WPX_UNI, WPX_SHFL, WPX_SHFL64, WPX_FIELDS };
DEV void wp_body_xlane(uint32_t const * v32, uint64_t const * v64, int32_t const * src, int32_t const bsrc, uint64_t * out)
{
	int const lane = wv_lane();
	uint32_t const a = v32[lane]; uint64_t const b = v64[lane]; int const s = src[lane];
	out[WPX_BCAST*64+lane] = wv_bcast(a,bsrc);
	out[WPX_BCAST64*64+lane] = wv_bcast64(b,bsrc);
	out[WPX_UNI*64+lane] = wv_uni(a);
	out[WPX_SHFL*64+lane] = wv_shfl(a,s);
	out[WPX_SHFL64*64+lane] = wv_shfl64(b,s);
}

// ---- sorts of 64 bit keys in memory (PT: an LDS or a global pointer on the device) ----
// The (CAP, R32) pairs of wv_sort_keys the product instantiates (fast_window.hpp: FastLds<CT>::keycap, CT::precap, fcpow2(CT::scap) over
// the FastTier table, and the 32-registers-per-lane case of tier 4); tests/test_waveprobe.py reads the tier table and holds this list against it.
#define WP_SORT_PAIRS(X) \
	X(0,32,false) X(1,64,false) X(2,128,false) X(3,256,false) X(4,512,false) X(5,576,false) X(6,704,false) X(7,1024,false) \
	X(8,2048,false) X(9,2560,false) X(10,3072,false) X(11,4096,false) X(12,8192,false) X(13,16384,false) X(14,2048,true)
enum { WP_SORT_NPAIRS = 15, WP_SORT_BITONIC = 15, WP_SORT_BITONIC_N = 16, WP_SORT_MODES = 17, WP_SORT_MAXN = 16384 };
template<typename PT>
DEV void wp_body_sort(uint32_t const mode, PT A, uint32_t const n)
{
	switch ( mode )
	{
#define WP_SORT_CASE(ID,CAP,R32) case ID: wv_sort_keys<CAP,R32>(A,n); break;
		WP_SORT_PAIRS(WP_SORT_CASE)
#undef WP_SORT_CASE
		case WP_SORT_BITONIC: wv_bitonic_sort(A,n); break;          // n a power of two
		case WP_SORT_BITONIC_N: wv_bitonic_sort_n(A,n); break;
		default: break;
	}
}
// copy between the job's slice of the key buffer and the array the sort runs on (the LDS variant of the device; all lanes call)
template<typename PD, typename PS>
DEV void wp_copy64(PD dst, PS src, uint32_t const n)
{
	for ( uint32_t i = wv_lane(); i < n; i += WSZ ) dst[i] = src[i];
	wv_sync();
}

// ---- atomics: every lane adds lane+1 to one word and keeps the old value ----
template<typename PT>
DEV uint32_t wp_body_atomic(PT word)
{
	return wv_atomic_add(word,static_cast<uint32_t>(wv_lane()+1));
}

}
#endif
