/* TEST HARNESS ONLY: the entry points libwaveprobe_dev.so (probe.hip, gfx950) and libwaveprobe_host.so (probe_host.cpp, 64-lane host
 * wavefront) share; tests/waveprobe_lib.py calls either through ctypes.  Every entry point returns 0 or an error code (the device
 * library: a hipError_t, text from wp_error_string; the host library: 1 for arguments out of range), and none throws. */
#ifndef DACC_WAVEPROBE_API_H
#define DACC_WAVEPROBE_API_H
#include <stdint.h>

/* one sort: `n` keys at keys[off .. off+n), sorted in place by sort mode `mode` (probe_body.hpp: WP_SORT_PAIRS, WP_SORT_BITONIC, WP_SORT_BITONIC_N) */
typedef struct wp_job { uint32_t mode, n, off, pad; } wp_job;
/* one index sort: idx[ioff .. ioff+p2) (indices into kbuf[koff .. koff+nk), 0xFFFFFFFF pads) by (key, index) */
typedef struct wp_idxjob { uint32_t p2, nk, koff, ioff; } wp_idxjob;

enum { WP_SPACE_LDS = 0, WP_SPACE_GLOBAL = 1 };

#ifdef __cplusplus
extern "C" {
#endif
const char * wp_error_string(int rc);
int wp_is_device(void);
/* (cap, r32) of sort modes 0 .. wp_sort_pairs()-1 */
int wp_sort_pairs(uint32_t * cap, int32_t * r32, uint32_t room);
int wp_u32(uint32_t const * vals, uint32_t const * flags, uint64_t * out, uint32_t ncases);                          /* out[ncases][WP32_FIELDS][64] */
int wp_u64(uint64_t const * vals, uint64_t * out, uint32_t ncases);                                                   /* out[ncases][WP64_FIELDS][64] */
int wp_xlane(uint32_t const * v32, uint64_t const * v64, int32_t const * src, int32_t const * bsrc, uint64_t * out, uint32_t ncases);   /* out[ncases][WPX_FIELDS][64] */
int wp_sort(int space, wp_job const * jobs, uint32_t njobs, uint64_t * keys, uint64_t nkeys);
int wp_sort_idx(int space, wp_idxjob const * jobs, uint32_t njobs, uint64_t const * kbuf, uint64_t nk, uint32_t * idx, uint64_t nidx);
/* out[3][65]: old value per lane + final value of (LDS word, wv_atomic_add) / (global word, wv_atomic_add_global) / (global word, wv_atomic_add) */
int wp_atomic(uint32_t init, uint32_t * out);
#ifdef __cplusplus
}
#endif

#if defined(__cplusplus) && defined(DACC_WAVEPROBE_BODY_HPP)
/* argument checks shared by both libraries: nothing is launched on jobs that would read or write outside their buffers */
static inline bool wp_sort_jobs_ok(wp_job const * jobs, uint32_t njobs, uint64_t nkeys, uint32_t & maxn)
{
	static uint32_t const caps[] = {
#define WP_CAP(ID,CAP,R32) CAP,
		WP_SORT_PAIRS(WP_CAP)
#undef WP_CAP
	};
	maxn = 0;
	for ( uint32_t i = 0; i < njobs; ++i )
	{
		wp_job const & j = jobs[i];
		if ( j.mode >= dacc::WP_SORT_MODES || j.n > dacc::WP_SORT_MAXN || static_cast<uint64_t>(j.off) + j.n > nkeys ) return false;
		if ( j.mode < dacc::WP_SORT_NPAIRS && j.n > caps[j.mode] ) return false;
		if ( j.mode == dacc::WP_SORT_BITONIC && (j.n & (j.n-1)) ) return false;
		if ( j.n > maxn ) maxn = j.n;
	}
	return true;
}
static inline bool wp_idx_jobs_ok(wp_idxjob const * jobs, uint32_t njobs, uint64_t nk, uint32_t const * idx, uint64_t nidx, uint32_t & maxbytes)
{
	maxbytes = 0;
	for ( uint32_t i = 0; i < njobs; ++i )
	{
		wp_idxjob const & j = jobs[i];
		if ( j.p2 > 4096 || (j.p2 & (j.p2-1)) || j.nk > 4096 || static_cast<uint64_t>(j.koff) + j.nk > nk || static_cast<uint64_t>(j.ioff) + j.p2 > nidx ) return false;
		for ( uint32_t q = 0; q < j.p2; ++q ) if ( idx[j.ioff+q] != 0xFFFFFFFFu && idx[j.ioff+q] >= j.nk ) return false;
		uint32_t const b = j.nk*8u + j.p2*4u;
		if ( b > maxbytes ) maxbytes = b;
	}
	return true;
}
#endif
#endif
