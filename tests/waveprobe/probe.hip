/*
 * TEST HARNESS ONLY (libwaveprobe_dev.so, never part of libdaccord_hip.so): the probe bodies of probe_body.hpp as gfx950 kernels, one
 * wavefront per workgroup (what wv_sync() assumes), compiled with the product's flags.  The sorts run twice: on an LDS array (address
 * space 3, as in the LDS tiers) and on a global one (address space 1, as in k_window_fast<13|14>).  Every entry point allocates, copies
 * in, launches, synchronises, copies out and frees, and returns the first HIP error it met.
 */
#include <hip/hip_runtime.h>
#include "probe_body.hpp"
#include "probe_api.h"

using namespace dacc;

// address spaces by name: this unit needs both kinds of pointer at once (wave.hpp's LDSQ is one or the other per unit)
#if defined(__HIP_DEVICE_COMPILE__)
#define WP_LDS __attribute__((address_space(3)))
#define WP_GLB __attribute__((address_space(1)))
#else
#define WP_LDS
#define WP_GLB
#endif

__global__ void __launch_bounds__(64) k_wp_u32(uint32_t const * vals, uint32_t const * flags, uint64_t * out)
{
	uint64_t const c = blockIdx.x;
	wp_body_u32(vals + 64*c,flags + 64*c,out + WP32_FIELDS*64*c);
}
__global__ void __launch_bounds__(64) k_wp_u64(uint64_t const * vals, uint64_t * out)
{
	uint64_t const c = blockIdx.x;
	wp_body_u64(vals + 64*c,out + WP64_FIELDS*64*c);
}
__global__ void __launch_bounds__(64) k_wp_xlane(uint32_t const * v32, uint64_t const * v64, int32_t const * src, int32_t const * bsrc, uint64_t * out)
{
	uint64_t const c = blockIdx.x;
	wp_body_xlane(v32 + 64*c,v64 + 64*c,src + 64*c,bsrc[c],out + WPX_FIELDS*64*c);
}
__global__ void __launch_bounds__(64) k_wp_sort_glb(wp_job const * jobs, uint64_t * keys)
{
	wp_job const j = jobs[blockIdx.x];
	uint32_t const mode = __builtin_amdgcn_readfirstlane(j.mode), n = __builtin_amdgcn_readfirstlane(j.n);
	WP_GLB uint64_t * A = (WP_GLB uint64_t *)(keys + j.off);
	wp_body_sort(mode,A,n);
}
__global__ void __launch_bounds__(64) k_wp_sort_lds(wp_job const * jobs, uint64_t * keys)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t wp_lds[];
	wp_job const j = jobs[blockIdx.x];
	uint32_t const mode = __builtin_amdgcn_readfirstlane(j.mode), n = __builtin_amdgcn_readfirstlane(j.n);
	WP_LDS uint64_t * A = (WP_LDS uint64_t *)wp_lds;
	wp_copy64(A,keys + j.off,n);
	wp_body_sort(mode,A,n);
	wv_sync();
	wp_copy64(keys + j.off,A,n);
}
__global__ void __launch_bounds__(64) k_wp_idx_glb(wp_idxjob const * jobs, uint64_t const * kbuf, uint32_t * idx)
{
	wp_idxjob const j = jobs[blockIdx.x];
	wv_bitonic_sort_idx(idx + j.ioff,kbuf + j.koff,__builtin_amdgcn_readfirstlane(j.p2));
}
__global__ void __launch_bounds__(64) k_wp_idx_lds(wp_idxjob const * jobs, uint64_t const * kbuf, uint32_t * idx)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t wp_lds[];
	wp_idxjob const j = jobs[blockIdx.x];
	uint32_t const p2 = __builtin_amdgcn_readfirstlane(j.p2), nk = __builtin_amdgcn_readfirstlane(j.nk);
	uint64_t * K = reinterpret_cast<uint64_t *>(wp_lds); uint32_t * I = reinterpret_cast<uint32_t *>(wp_lds + 8u*nk);
	for ( uint32_t i = wv_lane(); i < nk; i += WSZ ) K[i] = kbuf[j.koff+i];
	for ( uint32_t i = wv_lane(); i < p2; i += WSZ ) I[i] = idx[j.ioff+i];
	wv_sync();
	wv_bitonic_sort_idx(I,K,p2);
	wv_sync();
	for ( uint32_t i = wv_lane(); i < p2; i += WSZ ) idx[j.ioff+i] = I[i];
}
// gwords[0]: wv_atomic_add_global, gwords[1]: wv_atomic_add through a global pointer; both hold `init` at the launch (the host reads their final values)
__global__ void __launch_bounds__(64) k_wp_atomic(uint32_t const init, uint32_t * gwords, uint32_t * out)
{
	__shared__ uint32_t word;
	int const lane = wv_lane();
	if ( lane == 0 ) word = init;
	wv_sync();
	out[lane] = wp_body_atomic((WP_LDS uint32_t *)&word);
	wv_sync();
	if ( lane == 0 ) out[64] = word;
	out[65+lane] = wv_atomic_add_global(gwords,static_cast<uint32_t>(lane+1));
	out[130+lane] = wp_body_atomic((WP_GLB uint32_t *)(gwords+1));
}

namespace {
// a device buffer that frees itself; nothing here throws
struct Buf
{
	void * p; Buf() : p(0) {}
	~Buf() { if ( p ) (void)hipFree(p); }
	hipError_t alloc(size_t const bytes) { return hipMalloc(&p,bytes ? bytes : 16); }
	hipError_t up(void const * src, size_t const bytes) { return bytes ? hipMemcpy(p,src,bytes,hipMemcpyHostToDevice) : hipSuccess; }
	hipError_t down(void * dst, size_t const bytes) const { return bytes ? hipMemcpy(dst,p,bytes,hipMemcpyDeviceToHost) : hipSuccess; }
	template<typename T> T * as() const { return static_cast<T *>(p); }
};
}
#define WPCHK(x) do { hipError_t const e_ = (x); if ( e_ != hipSuccess ) return static_cast<int>(e_); } while ( 0 )
#define WPSYNC() do { WPCHK(hipGetLastError()); WPCHK(hipDeviceSynchronize()); } while ( 0 )

extern "C" const char * wp_error_string(int rc) { return hipGetErrorString(static_cast<hipError_t>(rc)); }
extern "C" int wp_is_device(void) { return 1; }
extern "C" int wp_sort_pairs(uint32_t * cap, int32_t * r32, uint32_t room)
{
#define WP_PAIR(ID,CAP,R32) if ( ID < room ) { cap[ID] = CAP; r32[ID] = R32 ? 1 : 0; }
	WP_SORT_PAIRS(WP_PAIR)
#undef WP_PAIR
	return WP_SORT_NPAIRS;
}

extern "C" int wp_u32(uint32_t const * vals, uint32_t const * flags, uint64_t * out, uint32_t ncases)
{
	if ( !ncases ) return 0;
	size_t const nin = static_cast<size_t>(ncases)*64*4, nout = static_cast<size_t>(ncases)*WP32_FIELDS*64*8;
	Buf dv, df, dout;
	WPCHK(dv.alloc(nin)); WPCHK(df.alloc(nin)); WPCHK(dout.alloc(nout));
	WPCHK(dv.up(vals,nin)); WPCHK(df.up(flags,nin)); WPCHK(hipMemset(dout.p,0xEE,nout));
	hipLaunchKernelGGL(k_wp_u32,dim3(ncases),dim3(64),0,0,dv.as<uint32_t const>(),df.as<uint32_t const>(),dout.as<uint64_t>());
	WPSYNC();
	WPCHK(dout.down(out,nout));
	return 0;
}
extern "C" int wp_u64(uint64_t const * vals, uint64_t * out, uint32_t ncases)
{
	if ( !ncases ) return 0;
	size_t const nin = static_cast<size_t>(ncases)*64*8, nout = static_cast<size_t>(ncases)*WP64_FIELDS*64*8;
	Buf dv, dout;
	WPCHK(dv.alloc(nin)); WPCHK(dout.alloc(nout));
	WPCHK(dv.up(vals,nin)); WPCHK(hipMemset(dout.p,0xEE,nout));
	hipLaunchKernelGGL(k_wp_u64,dim3(ncases),dim3(64),0,0,dv.as<uint64_t const>(),dout.as<uint64_t>());
	WPSYNC();
	WPCHK(dout.down(out,nout));
	return 0;
}
extern "C" int wp_xlane(uint32_t const * v32, uint64_t const * v64, int32_t const * src, int32_t const * bsrc, uint64_t * out, uint32_t ncases)
{
	if ( !ncases ) return 0;
	for ( size_t i = 0; i < static_cast<size_t>(ncases)*64; ++i ) if ( src[i] < 0 || src[i] > 63 ) return static_cast<int>(hipErrorInvalidValue);
	for ( uint32_t i = 0; i < ncases; ++i ) if ( bsrc[i] < 0 || bsrc[i] > 63 ) return static_cast<int>(hipErrorInvalidValue);
	size_t const n32 = static_cast<size_t>(ncases)*64*4, n64 = 2*n32, nout = static_cast<size_t>(ncases)*WPX_FIELDS*64*8;
	Buf d32, d64, dsrc, db, dout;
	WPCHK(d32.alloc(n32)); WPCHK(d64.alloc(n64)); WPCHK(dsrc.alloc(n32)); WPCHK(db.alloc(ncases*4)); WPCHK(dout.alloc(nout));
	WPCHK(d32.up(v32,n32)); WPCHK(d64.up(v64,n64)); WPCHK(dsrc.up(src,n32)); WPCHK(db.up(bsrc,ncases*4)); WPCHK(hipMemset(dout.p,0xEE,nout));
	hipLaunchKernelGGL(k_wp_xlane,dim3(ncases),dim3(64),0,0,d32.as<uint32_t const>(),d64.as<uint64_t const>(),dsrc.as<int32_t const>(),db.as<int32_t const>(),dout.as<uint64_t>());
	WPSYNC();
	WPCHK(dout.down(out,nout));
	return 0;
}
extern "C" int wp_sort(int space, wp_job const * jobs, uint32_t njobs, uint64_t * keys, uint64_t nkeys)
{
	if ( !njobs ) return 0;
	uint32_t maxn = 0;
	if ( (space != WP_SPACE_LDS && space != WP_SPACE_GLOBAL) || !wp_sort_jobs_ok(jobs,njobs,nkeys,maxn) ) return static_cast<int>(hipErrorInvalidValue);
	Buf dj, dk;
	WPCHK(dj.alloc(njobs*sizeof(wp_job))); WPCHK(dk.alloc(nkeys*8));
	WPCHK(dj.up(jobs,njobs*sizeof(wp_job))); WPCHK(dk.up(keys,nkeys*8));
	if ( space == WP_SPACE_GLOBAL )
		hipLaunchKernelGGL(k_wp_sort_glb,dim3(njobs),dim3(64),0,0,dj.as<wp_job const>(),dk.as<uint64_t>());
	else
	{
		uint32_t const lds = maxn*8u < 1024u ? 1024u : maxn*8u;      // at most 128 KiB of the CU's 160
		if ( lds > 64*1024 ) WPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_wp_sort_lds),hipFuncAttributeMaxDynamicSharedMemorySize,lds));
		hipLaunchKernelGGL(k_wp_sort_lds,dim3(njobs),dim3(64),lds,0,dj.as<wp_job const>(),dk.as<uint64_t>());
	}
	WPSYNC();
	WPCHK(dk.down(keys,nkeys*8));
	return 0;
}
extern "C" int wp_sort_idx(int space, wp_idxjob const * jobs, uint32_t njobs, uint64_t const * kbuf, uint64_t nk, uint32_t * idx, uint64_t nidx)
{
	if ( !njobs ) return 0;
	uint32_t lds = 0;
	if ( (space != WP_SPACE_LDS && space != WP_SPACE_GLOBAL) || !wp_idx_jobs_ok(jobs,njobs,nk,idx,nidx,lds) ) return static_cast<int>(hipErrorInvalidValue);
	Buf dj, dk, di;
	WPCHK(dj.alloc(njobs*sizeof(wp_idxjob))); WPCHK(dk.alloc(nk*8)); WPCHK(di.alloc(nidx*4));
	WPCHK(dj.up(jobs,njobs*sizeof(wp_idxjob))); WPCHK(dk.up(kbuf,nk*8)); WPCHK(di.up(idx,nidx*4));
	if ( space == WP_SPACE_GLOBAL )
		hipLaunchKernelGGL(k_wp_idx_glb,dim3(njobs),dim3(64),0,0,dj.as<wp_idxjob const>(),dk.as<uint64_t const>(),di.as<uint32_t>());
	else
		hipLaunchKernelGGL(k_wp_idx_lds,dim3(njobs),dim3(64),lds < 1024u ? 1024u : lds,0,dj.as<wp_idxjob const>(),dk.as<uint64_t const>(),di.as<uint32_t>());      // (at most 48 KiB: wp_idx_jobs_ok)
	WPSYNC();
	WPCHK(di.down(idx,nidx*4));
	return 0;
}
extern "C" int wp_atomic(uint32_t init, uint32_t * out)
{
	Buf dg, dout;
	uint32_t const g[2] = { init, init };
	WPCHK(dg.alloc(8)); WPCHK(dout.alloc(3*65*4));
	WPCHK(dg.up(g,8)); WPCHK(hipMemset(dout.p,0xEE,3*65*4));
	hipLaunchKernelGGL(k_wp_atomic,dim3(1),dim3(64),0,0,init,dg.as<uint32_t>(),dout.as<uint32_t>());
	WPSYNC();
	WPCHK(dout.down(out,3*65*4));
	uint32_t fin[2] = { 0, 0 };
	WPCHK(dg.down(fin,8));
	out[65+64] = fin[0]; out[130+64] = fin[1];
	return 0;
}
