/*
 * TEST HARNESS ONLY (libwaveprobe_host.so): the probe bodies of probe_body.hpp under wave_run() of the 64-lane host wavefront
 * (g++ -DDACC_EMUL -DDACC_EMUL_LANES=64 -DDACC_EMUL_IMPL).  Where there is no GPU this validates the bodies and the expected values
 * of tests/waveprobe_cases.py, and it holds wave_emul64.hpp's restatements of the primitives to the same table the device is held to.
 * Same entry points as probe.hip; LDS and global memory are the same thing here, both variants of a sort run the same code.
 */
#include <vector>
#include <cstring>
#include "probe_body.hpp"
#include "probe_api.h"

using namespace dacc;

extern "C" const char * wp_error_string(int rc) { return rc ? "argument out of range (host probe)" : "ok"; }
extern "C" int wp_is_device(void) { return 0; }
extern "C" int wp_sort_pairs(uint32_t * cap, int32_t * r32, uint32_t room)
{
#define WP_PAIR(ID,CAP,R32) if ( ID < room ) { cap[ID] = CAP; r32[ID] = R32 ? 1 : 0; }
	WP_SORT_PAIRS(WP_PAIR)
#undef WP_PAIR
	return WP_SORT_NPAIRS;
}

extern "C" int wp_u32(uint32_t const * vals, uint32_t const * flags, uint64_t * out, uint32_t ncases)
{
	std::memset(out,0xEE,static_cast<size_t>(ncases)*WP32_FIELDS*64*8);
	for ( uint64_t c = 0; c < ncases; ++c ) wave_run([&]() { wp_body_u32(vals + 64*c,flags + 64*c,out + WP32_FIELDS*64*c); });
	return 0;
}
extern "C" int wp_u64(uint64_t const * vals, uint64_t * out, uint32_t ncases)
{
	std::memset(out,0xEE,static_cast<size_t>(ncases)*WP64_FIELDS*64*8);
	for ( uint64_t c = 0; c < ncases; ++c ) wave_run([&]() { wp_body_u64(vals + 64*c,out + WP64_FIELDS*64*c); });
	return 0;
}
extern "C" int wp_xlane(uint32_t const * v32, uint64_t const * v64, int32_t const * src, int32_t const * bsrc, uint64_t * out, uint32_t ncases)
{
	for ( size_t i = 0; i < static_cast<size_t>(ncases)*64; ++i ) if ( src[i] < 0 || src[i] > 63 ) return 1;
	for ( uint32_t i = 0; i < ncases; ++i ) if ( bsrc[i] < 0 || bsrc[i] > 63 ) return 1;
	std::memset(out,0xEE,static_cast<size_t>(ncases)*WPX_FIELDS*64*8);
	for ( uint64_t c = 0; c < ncases; ++c ) wave_run([&]() { wp_body_xlane(v32 + 64*c,v64 + 64*c,src + 64*c,bsrc[c],out + WPX_FIELDS*64*c); });
	return 0;
}
extern "C" int wp_sort(int space, wp_job const * jobs, uint32_t njobs, uint64_t * keys, uint64_t nkeys)
{
	uint32_t maxn = 0;
	if ( (space != WP_SPACE_LDS && space != WP_SPACE_GLOBAL) || !wp_sort_jobs_ok(jobs,njobs,nkeys,maxn) ) return 1;
	std::vector<uint64_t> lds(maxn ? maxn : 1);
	for ( uint32_t i = 0; i < njobs; ++i )
	{
		wp_job const j = jobs[i];
		if ( space == WP_SPACE_GLOBAL ) wave_run([&]() { wp_body_sort(j.mode,keys + j.off,j.n); });
		else wave_run([&]() { uint64_t * A = lds.data(); wp_copy64(A,keys + j.off,j.n); wp_body_sort(j.mode,A,j.n); wv_sync(); wp_copy64(keys + j.off,A,j.n); });
	}
	return 0;
}
extern "C" int wp_sort_idx(int space, wp_idxjob const * jobs, uint32_t njobs, uint64_t const * kbuf, uint64_t nk, uint32_t * idx, uint64_t nidx)
{
	uint32_t bytes = 0;
	if ( (space != WP_SPACE_LDS && space != WP_SPACE_GLOBAL) || !wp_idx_jobs_ok(jobs,njobs,nk,idx,nidx,bytes) ) return 1;
	for ( uint32_t i = 0; i < njobs; ++i )
	{
		wp_idxjob const j = jobs[i];
		wave_run([&]() { wv_bitonic_sort_idx(idx + j.ioff,kbuf + j.koff,j.p2); });
	}
	return 0;
}
extern "C" int wp_atomic(uint32_t init, uint32_t * out)
{
	uint32_t words[3] = { init, init, init };
	std::memset(out,0xEE,3*65*4);
	wave_run([&]() {
		int const lane = wv_lane();
		out[lane] = wp_body_atomic(&words[0]);
		out[65+lane] = wv_atomic_add_global(&words[1],static_cast<uint32_t>(lane+1));
		out[130+lane] = wp_body_atomic(&words[2]);
	});
	out[64] = words[0]; out[129] = words[1]; out[194] = words[2];
	return 0;
}
