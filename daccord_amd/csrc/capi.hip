/*
 * libdaccord_hip.so: C ABI (include/daccord_hip.h) + gfx950 kernels.
 * Host side: the context and what it owns on the device (context.hpp), batch planning, the batch setup (dacc_submit_piles_body; its arithmetic: launch_geometry.hpp)
 * and the device pass (runDevice), each a sequence of phases, HIP-event timing.
 * There is no CPU fallback anywhere in this file: no device => DACC_ENODEV.
 */
#include <hip/hip_runtime.h>
#include <vector>
#include <string>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <new>
#include "../../include/daccord_hip.h"
#include "batch_plan.hpp"
#include "host_tables.hpp"
#include "window_kernels.hpp"
#include "trace_kernel.hpp"
#include "launch_geometry.hpp"
#include "vote_kernel.hpp"
#include "emit_record.hpp"
#include "context.hpp"

using namespace dacc;

// ---------------------------------------------------------------- kernels

struct PrepBatch
{
	DevOvl const * ovl; uint64_t novl; uint8_t const * trace; uint32_t trace_bytes;
	uint32_t * blk_ovl; uint32_t * blk_b0;
};

// per overlap: block task table (overlap id, B start of every tspace block = prefix sum of the trace B lengths)
__global__ void k_prep(PrepBatch B)
{
	uint64_t const o = static_cast<uint64_t>(blockIdx.x)*blockDim.x + threadIdx.x;
	if ( o >= B.novl ) return;
	DevOvl const ov = B.ovl[o];
	uint32_t b = ov.bbpos;
	for ( int32_t i = 0; i < ov.nblk; ++i )
	{
		B.blk_ovl[ov.blk0+i] = o; B.blk_b0[ov.blk0+i] = b;
		b += B.trace_bytes == 2 ? reinterpret_cast<uint16_t const *>(B.trace)[ov.trace_off+2*i+1] : B.trace[ov.trace_off+2*i+1];
	}
}

// one lane per tspace block, one wavefront per workgroup; the column checkpoints of every lane go to the workgroup's global
// slab, the segment the traceback is in lives in the workgroup's dynamic LDS (TRACE2_LDS = 8 KB)
__global__ void __launch_bounds__(64) k_trace(TraceBatch B)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lds_trace[];
	TraceStoreGL st;
	st.g = B.slab + static_cast<size_t>(blockIdx.x)*traceSlabWords(B.maxcols);
	st.w = (LDSQ uint32_t *)lds_trace; st.lane = threadIdx.x;
	if ( B.work )
	{
		// (round 6) rounds of 64 consecutive blocks drawn from a counter: with a fixed stride the workgroups whose blocks have long B spans
		// were still running when the others had left (11.8 of 18 wavefronts per CU resident on average, profiles/r06t_pmc_summary.json)
		while ( true )
		{
			uint32_t b = 0;
			if ( threadIdx.x == 0 ) b = atomicAdd(B.work,64u);
			b = __builtin_amdgcn_readfirstlane(b);
			if ( b >= B.nblocks ) break;
			uint64_t const task = static_cast<uint64_t>(b) + threadIdx.x;
			if ( task < B.nblocks ) traceBlock(B,task,st);
		}
		return;
	}
	for ( uint64_t task = static_cast<uint64_t>(blockIdx.x)*64 + threadIdx.x; task < B.nblocks; task += static_cast<uint64_t>(gridDim.x)*64 )
		traceBlock(B,task,st);
}

// tspace in (128, 64*NW]: NW words per column vector; the first nl lanes of the wavefront take blocks (nl = 64, 32, 16 or 8:
// as many as have room for their column checkpoints in LDS)
template<int NW>
__global__ void __launch_bounds__(64) k_trace_wide(TraceBatch B, uint32_t const nl)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lds_trace[];
	uint32_t const slots = traceSlots(B.maxcols);
	TraceStoreW<NW> st;
	st.w = (LDSQ uint64_t *)lds_trace; st.sc = (LDSQ uint16_t *)(lds_trace + static_cast<size_t>(slots)*(2*NW)*nl*8); st.lane = threadIdx.x; st.nl = nl;
	if ( threadIdx.x < nl )
		for ( uint64_t task = static_cast<uint64_t>(blockIdx.x)*nl + threadIdx.x; task < B.nblocks; task += static_cast<uint64_t>(gridDim.x)*nl )
			traceBlockWide<NW>(B,task,st);
}

// Before the LDS tiers: one wavefront per overlap scans its rows of the window tables for B strings that the first slot's tiers (strings of
// up to 64 bases) cannot hold.  Two bit maps: pregen = a string of more than 64 bases (the first slot's tiers and the size-class pre-pass skip
// the window), pregen2 = one of more than 128 (every LDS tier skips it).  k_prescan_lists then sorts the flagged windows into two lists.
// (Round 6: tiers 6 and 3 hold strings of up to 128 bases -- two words per pattern mask -- so a window with a string of 65 ... 128 bases joins
// the list the second slot reads, next to the first slot's hand-overs; rounds 3-5 ran all of them in tier 5 on the second stream, the LDS of a
// whole CU per wavefront: at -w 56 / 60 / 63 that is 21 / 65 / 88 % of the windows of PacBio-like reads, profiles/r06l.)
__global__ void __launch_bounds__(256) k_prescan(DevOvl const * ovl, uint64_t novl, uint32_t const * ovl_pile, DevPile const * piles, uint32_t const * wt_b, uint32_t const * wt_e,
	uint32_t * pregen, uint32_t * pregen2, uint32_t const thr1)
{
	// one wavefront per overlap, lanes over its rows: coalesced reads of the two tables
	uint64_t const o = static_cast<uint64_t>(blockIdx.x)*4 + (threadIdx.x>>6);
	if ( o >= novl ) return;
	DevOvl const ov = ovl[o];
	uint64_t const winbase = piles[ovl_pile[o]].winbase;
	for ( uint32_t r = threadIdx.x & 63; r < ov.ny; r += 64 )
	{
		uint32_t const len = wt_e[ov.wtoff+r] - wt_b[ov.wtoff+r];
		if ( len > thr1 )      // 64; a wide batch (tier 8: strings of up to 128 bases): 128
		{
			uint64_t const w = winbase + ov.y0 + r;
			uint32_t const bit = 1u << (w&31);
			atomicOr(pregen + (w>>5),bit);
			if ( len > 128u ) atomicOr(pregen2 + (w>>5),bit);
		}
	}
}
// one thread per word of the bit maps: a flagged window goes to the second stream's list (a string of more than 128 bases: tier 5 / the generic
// engine) or to the list the second slot's tier reads; its result record forgets what an earlier batch left (the tiers resume from it)
__global__ void __launch_bounds__(256) k_prescan_lists(uint32_t const * pregen, uint32_t const * pregen2, uint64_t nwindows, uint32_t * list128, uint32_t * slot1list, WindowOut * wout)
{
	uint64_t const wi = static_cast<uint64_t>(blockIdx.x)*256 + threadIdx.x;
	if ( wi*32 >= nwindows ) return;
	uint32_t m = pregen[wi]; uint32_t const m2 = pregen2[wi];
	while ( m )
	{
		uint32_t const b = static_cast<uint32_t>(__builtin_ctz(m)); m &= m-1;
		uint64_t const w = wi*32 + b;
		if ( w >= nwindows ) break;
		wout[w].status = WS_INSUFFICIENT;
		uint32_t * const dst = ((m2 >> b) & 1u) || !slot1list ? list128 : slot1list;
		uint32_t const q = atomicAdd(dst,1u); dst[1+q] = static_cast<uint32_t>(w);
	}
}

// after all engines: a window still marked as handed on is an internal error (errflag); a window the generic engine
// could not hold even with grown scratch drops its pile (pilebad), the batch goes on
__global__ void k_check_done(WindowOut const * wout, uint64_t n, uint32_t * errflag, DevPile const * piles, uint32_t npiles, uint8_t * pilebad)
{
	uint64_t const i = static_cast<uint64_t>(blockIdx.x)*blockDim.x + threadIdx.x;
	if ( i >= n ) return;
	uint32_t const st = wout[i].status;
	if ( st == WS_RETRY ) atomicOr(errflag,1u);
	if ( st == WS_OVERFLOW )
	{
		uint32_t lo = 0, hi = npiles;
		while ( hi-lo > 1 ) { uint32_t const mid = (lo+hi)>>1; if ( piles[mid].winbase <= i ) lo = mid; else hi = mid; }
		pilebad[lo] = 1;
	}
}

// behind all engines and in front of the vote: one lane per window turns the pending record a tier left (narrow windows, dev_types.hpp:
// WREC_PENDING) into the final one (emit_record.hpp: the consensus -> A alignment); final and empty records -- the generic engine's, the
// windows without a consensus -- stay as they are, so a second run over the same records changes nothing.  A wide batch has none pending.
__global__ void __launch_bounds__(256) k_emit(uint8_t * wrec, uint64_t n, uint32_t w)
{
	uint64_t const i = static_cast<uint64_t>(blockIdx.x)*256 + threadIdx.x;
	if ( i >= n || w == 0 || DACC_WIDE_W(w) ) return;
	emitPendingRecord(wrec + i*WREC,w);
}

// dacc_timing's counters of the deep-window tier: the windows with more than `mins` strings on the list the tier read (out[0]) and on the
// list it handed on (out[1]); the tier passes every other window of its list on untouched.  Reads the final window records.
__global__ void k_count_deeper(uint32_t const * in, uint32_t const * handon, WindowOut const * wout, uint32_t const mins, uint32_t * out)
{
	uint32_t const nin = in[0], nout = handon[0];
	uint32_t a = 0, b = 0;
	for ( uint32_t i = blockIdx.x*blockDim.x + threadIdx.x; i < nin; i += gridDim.x*blockDim.x ) a += static_cast<uint32_t>(wout[in[1+i]].mao) > mins;
	for ( uint32_t i = blockIdx.x*blockDim.x + threadIdx.x; i < nout; i += gridDim.x*blockDim.x ) b += static_cast<uint32_t>(wout[handon[1+i]].mao) > mins;
	if ( a ) atomicAdd(out,a);
	if ( b ) atomicAdd(out+1,b);
}
// windows the generic engine left as WS_OVERFLOW -> list (count in list[0])
__global__ void k_collect_overflow(WindowOut const * wout, uint64_t n, uint32_t * list)
{
	uint64_t const i = static_cast<uint64_t>(blockIdx.x)*blockDim.x + threadIdx.x;
	if ( i < n && wout[i].status == WS_OVERFLOW ) { uint32_t const q = atomicAdd(list,1u); list[1+q] = static_cast<uint32_t>(i); }
}

// exclusive scan of one value per thread over the 256 threads of the workgroup (4 wavefronts): DPP scan inside a
// wavefront, the four wavefront totals through LDS; MAXOP: running maximum instead of a sum
template<bool MAXOP>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t const v, uint32_t * part4, uint32_t & total)
{
	uint32_t const wave = threadIdx.x >> 6;
	uint32_t x = v;
	if ( MAXOP ) { DACC_DPP_SCAN(x,DACC_OP_MAX,0u) } else { DACC_DPP_SCAN(x,DACC_OP_ADD,0u) }
	// x = inclusive value of this lane; the exclusive one is the inclusive value of the lane before
	uint32_t excl = __shfl_up(x,1,64); if ( (threadIdx.x & 63) == 0 ) excl = 0;
	__syncthreads();
	if ( (threadIdx.x & 63) == 63 ) part4[wave] = x;
	__syncthreads();
	uint32_t base = 0, tot = 0;
	#pragma unroll
	for ( uint32_t i = 0; i < 4; ++i )
	{
		uint32_t const t = part4[i];
		if ( i < wave ) base = MAXOP ? (t > base ? t : base) : (base + t);
		tot = MAXOP ? (t > tot ? t : tot) : (tot + t);
	}
	total = tot;
	return MAXOP ? (excl > base ? excl : base) : (base + excl);
}

// Size classes (shallow batches): one thread per window decides from the window tables whether the window starts in tier 0 (small list),
// in tier 7 (middle list = the list tier 0 appends its hand-overs to; round 6) or in tier 1 (big list = the list tier 7 appends its
// hand-overs to); windows the pre-scan set aside are in none.  Blocks reserve their range of a list with one atomic each, so a list keeps
// the window order inside a block.  t7inst == 0: no middle class.
__global__ void __launch_bounds__(256) k_classify(WindowBatch B, uint32_t * small, uint32_t * mid, uint32_t * big, uint32_t const t0inst, uint32_t const t7inst)
{
	__shared__ uint32_t part4[4]; __shared__ uint32_t base3[3];
	uint64_t const w = static_cast<uint64_t>(blockIdx.x)*256 + threadIdx.x;
	uint32_t cls = 3;
	if ( w < B.nwindows && !(B.pregen && ((B.pregen[w>>5] >> (w&31)) & 1)) )
	{
		cls = classifyWindow(B,w,t0inst,t7inst);
		B.wout[w].status = WS_INSUFFICIENT;      // never WS_RETRY from an earlier batch: the tiers resume from a hand-over record
	}
	uint32_t tot0, tot1, tot2;
	uint32_t const p0 = block_scan_excl<false>(cls == 0 ? 1u : 0u,part4,tot0);
	__syncthreads();
	uint32_t const p1 = block_scan_excl<false>(cls == 1 ? 1u : 0u,part4,tot1);
	__syncthreads();
	uint32_t const p2 = block_scan_excl<false>(cls == 2 ? 1u : 0u,part4,tot2);
	if ( threadIdx.x == 0 ) { base3[0] = tot0 ? atomicAdd(small,tot0) : 0u; base3[1] = tot1 ? atomicAdd(big,tot1) : 0u; base3[2] = tot2 ? atomicAdd(mid,tot2) : 0u; }
	__syncthreads();
	if ( cls == 0 ) small[1+base3[0]+p0] = static_cast<uint32_t>(w);
	if ( cls == 1 ) big[1+base3[1]+p1] = static_cast<uint32_t>(w);
	if ( cls == 2 ) mid[1+base3[2]+p2] = static_cast<uint32_t>(w);
}


// one workgroup per pile.  The pile is walked in tiles of 256 positions (thread = position); the records of the windows
// that cover a tile (256/a + w/a + 2 of them, 256 B each) are staged in LDS once per pass, coalesced, so that the
// byte-wise reads of the vote hit LDS and every record leaves HBM once per pass.
enum { VOTE_STAGE = 48 };
__device__ __forceinline__ VoteTile vote_stage(VoteBatch const & B, DevPile const & pile, uint32_t const p0, uint32_t const np, uint8_t * lds)
{
	VoteTile VT; VT.stage = (LDSQ uint8_t const *)lds; VT.y0 = 0; VT.n = 0;
	uint32_t const a = B.P.a, w = B.P.w, nwin = pile.nwin;
	if ( ! nwin ) return VT;
	uint32_t const plast = (p0+255 < np) ? (p0+255) : (np-1);
	uint32_t const ylo = (p0 > w) ? ((p0-w + a-1)/a) : 0;
	uint32_t yhi = plast / a; if ( yhi > nwin-1 ) yhi = nwin-1;
	__syncthreads();      // the previous tile's readers are done
	if ( ylo <= yhi && yhi-ylo+1 <= VOTE_STAGE && !DACC_WIDE_W(w) )      // (wide records, w > 64, are read where they lie)
	{
		VT.y0 = ylo; VT.n = yhi-ylo+1;
		uint4 const * src = reinterpret_cast<uint4 const *>(B.wrec + (pile.winbase+ylo)*WREC);
		uint4 * dst = reinterpret_cast<uint4 *>(lds);
		for ( uint32_t i = threadIdx.x; i < VT.n*(WREC/16); i += 256 ) dst[i] = src[i];
	}
	__syncthreads();
	return VT;
}
__global__ void __launch_bounds__(256) k_vote(VoteBatch B)
{
	__shared__ uint32_t part4[4];
	__shared__ __attribute__((aligned(16))) uint8_t stage[VOTE_STAGE*WREC];
	uint32_t const pi = blockIdx.x;
	DevPile const pile = B.piles[pi];
	uint32_t const np = pileNpos(pile);
	uint32_t const tid = threadIdx.x;
	if ( B.pilebad && B.pilebad[pi] ) { if ( tid == 0 ) B.nfrag[pi] = 0; return; }     // dropped pile: no fragments
	for ( uint32_t t0 = 0; t0 < np; t0 += 256 )
	{
		VoteTile const VT = vote_stage(B,pile,t0,np,stage);
		if ( t0+tid < np ) votePass1(B,pile,t0+tid,VT);
	}
	__syncthreads();
	uint32_t run0 = 0;
	for ( uint32_t t0 = 0; t0 < np; t0 += 256 )
	{
		VoteTile const VT = vote_stage(B,pile,t0,np,stage);
		uint32_t const p = t0+tid;
		uint32_t const n = p < np ? votePass2(B,pile,p,0,VT) : 0u;
		uint32_t tot; uint32_t const ex = block_scan_excl<false>(n,part4,tot);
		if ( p < np ) { B.oc[pile.posbase+p] = n; B.ocs[pile.posbase+p] = run0 + ex; }
		run0 += tot;
	}
	uint32_t const total = run0;
	bool const fits = total <= 2*np+64;
	if ( !fits && tid == 0 ) atomicOr(B.errflag,2u);
	uint64_t const symbase = 2*pile.posbase + 64ull*pi;
	if ( fits )
		for ( uint32_t t0 = 0; t0 < np; t0 += 256 )
		{
			VoteTile const VT = vote_stage(B,pile,t0,np,stage);
			uint32_t const p = t0+tid;
			if ( p < np ) votePass2(B,pile,p,B.outsym+symbase+B.ocs[pile.posbase+p],VT);
		}
	__syncthreads();
	uint32_t const chunk = (np + 255)/256;
	uint32_t const p0 = tid*chunk < np ? tid*chunk : np, p1 = (p0+chunk < np) ? (p0+chunk) : np;
	// runs of consecutive positions with elements, kept if last-first >= 100 (HandleContext.hpp:2590-2612): every thread
	// walks its chunk; the start of the run that is open at the chunk's first position comes from a running maximum
	// over the chunks before it (start position + 1, 0 = none)
	uint8_t const * has = B.has + pile.posbase;
	uint32_t laststart = 0; bool open = false;
	for ( uint32_t p = p0; p < p1; ++p )
		if ( has[p] && (p == 0 || !has[p-1]) ) laststart = p+1;
	uint32_t dummy;
	uint32_t const instart = block_scan_excl<true>(laststart,part4,dummy);
	(void)open;
	uint32_t cur = instart;       // start+1 of the run a position of this chunk belongs to
	uint32_t nfr = 0;
	for ( int pass = 0; pass < 2; ++pass )
	{
		uint32_t fbase = 0, ftot = 0;
		if ( pass == 1 ) { fbase = block_scan_excl<false>(nfr,part4,ftot); if ( tid == 0 ) B.nfrag[pi] = fits ? ftot : 0; if ( !fits ) break; }
		cur = instart; uint32_t k = 0;
		VoteFragment * F = B.frags + B.fragbase[pi];
		for ( uint32_t p = p0; p < p1; ++p )
		{
			if ( ! has[p] ) continue;
			if ( p == 0 || !has[p-1] ) cur = p+1;
			if ( p+1 == np || !has[p+1] )
			{
				uint32_t const first = cur-1, q = p;
				if ( q-first >= 100 )
				{
					uint32_t const so = B.ocs[pile.posbase+first];
					uint32_t const eo = B.ocs[pile.posbase+q] + B.oc[pile.posbase+q];
					uint32_t const len = eo-so;
					if ( B.P.producefull || len >= B.P.minlen )
					{
						if ( pass == 1 ) { VoteFragment & f = F[fbase+k]; f.first = first; f.last = q; f.len = len; f.pad = 0; f.off = symbase + so; }
						++k;
					}
				}
			}
		}
		nfr = k;
	}
}

// ---------------------------------------------------------------- host

#define HIPCHK(call) do { hipError_t const e_ = (call); if ( e_ != hipSuccess ) { c->err = std::string(#call) + ": " + hipGetErrorString(e_); if ( e_ == hipErrorOutOfMemory ) c->oom = true; return DACC_EHIP; } } while (0)

template<typename T>
static int upload(dacc_ctx * c, DevBuf<T> & b, T const * src, size_t n)
{
	HIPCHK(b.ensure(n ? n : 1));
	if ( n ) HIPCHK(hipMemcpyAsync(b.p,src,n*sizeof(T),hipMemcpyHostToDevice,c->stream));
	return DACC_OK;
}

// The host side of these entry points allocates (plans, tables, staging vectors; the planner also runs threads): nothing leaves through
// the C ABI but a return code.  Their bodies are the *_body functions below.
template<typename F> static int guarded(dacc_ctx * c, F const & f)
{
	try { return f(); }
	catch ( std::bad_alloc const & ) { if ( c ) { try { c->err = "out of host memory"; } catch ( ... ) {} } return DACC_ENOMEM; }
	//  anything that is not an allocation failure -- std::system_error of a planner thread, length_error -- is an internal error,
	// not "out of memory", and the message names it instead of leaving the previous call's text in place
	catch ( std::exception const & ex ) { if ( c ) { try { c->err = std::string("host side failed: ") + ex.what(); } catch ( ... ) {} } return DACC_EINTERNAL; }
	catch ( ... ) { if ( c ) { try { c->err = "host side failed: unknown exception"; } catch ( ... ) {} } return DACC_EINTERNAL; }
}

extern "C" {

// number of HIP devices this process sees (0 if there is none or the runtime fails): lets a caller that spreads workers over
// devices tell "no such device" from any other dacc_create failure
int dacc_device_count(void)
{
	int ndev = 0;
	if ( hipGetDeviceCount(&ndev) != hipSuccess || ndev < 0 ) return 0;
	return ndev;
}

int dacc_create(dacc_ctx ** out, dacc_params const * p)
{
	if ( !out || !p ) return DACC_EINVAL;
	*out = 0;
	if ( p->klow < 3 || p->khigh > 16 || p->klow > p->khigh || !p->w || !p->a || p->w > DACC_WMAX || p->minfilterfreq < 0 ||
	     p->maxfilterfreq < p->minfilterfreq || p->tspace <= 0 || p->tspace > 512 )      // (tspace: 1..512, what the planner and the trace kernels hold)
		return DACC_EINVAL;
	// the DACC_*_AS_SLOT2=1 switches of the trailing stages each name the third slot's main tier: more than one is refused before anything is set up
	if ( readTierSwitches().conflict() ) return DACC_EINVAL;
	int ndev = 0;
	if ( hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p->device < 0 || p->device >= ndev )
		return DACC_ENODEV;
	if ( hipSetDevice(p->device) != hipSuccess ) return DACC_ENODEV;
	dacc_ctx * c = new (std::nothrow) dacc_ctx;
	if ( !c ) return DACC_ENOMEM;
	c->par = *p; c->device = p->device;
	c->sw = readTierSwitches();      // DACC_NOFAST, DACC_TIERS, DACC_WIDE_TIER, DACC_DENSE_TIER, DACC_DEEP_TIER, the trailing stages' DACC_*_TIER and DACC_*_AS_SLOT2, DACC_LONGSTR_TIER, DACC_LONG128, DACC_HAND, DACC_T0INST, DACC_T7INST, DACC_LDS_T1, DACC_LDS_T0
	c->env_sched = static_cast<int>(envNum("DACC_SCHED",1));      // bit 0: LDS tiers pull work from a counter, bit 1: generic engine too
	c->env_trdyn = !envOff("DACC_TRACE_DYN");      // 0: k_trace walks its blocks with a fixed stride
	c->env_t7adapt = !envOff("DACC_T7_ADAPT");      // 0: tier 7 stays on whatever it hands on
	c->env_dbgretry = envOn("DACC_DEBUG_RETRY");
	c->env_feasneed = envOff("DACC_FEAS_NEED") ? 0u : 1u; c->env_tiefast = envOff("DACC_TIE_FAST") ? 0u : 1u;
	// (a failure from here on: `delete c` destroys what has been created)
	if ( hipStreamCreate(&c->stream.h) != hipSuccess ) { delete c; return DACC_EHIP; }
	{ int lo = 0, hi = 0; hipDeviceGetStreamPriorityRange(&lo,&hi); if ( hipStreamCreateWithPriority(&c->stream2.h,hipStreamNonBlocking,hi) != hipSuccess ) { delete c; return DACC_EHIP; } }
	hipEventCreateWithFlags(&c->evFirstTier.h,hipEventDisableTiming); hipEventCreateWithFlags(&c->evEarlyGeneric.h,hipEventDisableTiming); hipEventCreateWithFlags(&c->evPrescan.h,hipEventDisableTiming);
	for ( Event & e : c->ev ) hipEventCreate(&e.h);
	for ( Event & e : c->evEmit ) hipEventCreate(&e.h);
	for ( Event & e : c->evLong ) hipEventCreate(&e.h);
	for ( Event & e : c->evslot ) hipEventCreate(&e.h);
	for ( dacc_ctx::Stage & S : c->st ) hipEventCreate(&S.done.h);
	hipEventCreate(&c->h2dend.h);
	*out = c;
	return DACC_OK;
}

void dacc_destroy(dacc_ctx * c)
{
	if ( !c ) return;
	hipSetDevice(c->device);
	hipStreamSynchronize(c->stream); hipStreamSynchronize(c->stream2);
	delete c;
}

char const * dacc_last_error(dacc_ctx * c) { return c ? c->err.c_str() : "null context"; }

static int dacc_set_error_profile_body(dacc_ctx * c, double p_i, double p_d, double est_cor)
{
	if ( !c ) return DACC_EINVAL;
	if ( !(p_i >= 0 && p_i < 1 && p_d >= 0 && p_d < 1 && est_cor >= 0 && est_cor <= 1) ) { c->err = "error profile out of range"; return DACC_EINVAL; }
	hipSetDevice(c->device);
	buildHostTables(c->H,c->par.w,p_i,p_d,est_cor,c->par.klow,c->par.khigh,4200);
	c->est_cor = est_cor;
	int rc;
	if ( (rc = upload(c,c->d_dpnorm,c->H.dpnorm.data(),c->H.dpnorm.size())) ) return rc;
	if ( (rc = upload(c,c->d_dpsq,c->H.dpsq.data(),c->H.dpsq.size())) ) return rc;
	if ( (rc = upload(c,c->d_vs,c->H.dpsq_vs.data(),c->H.dpsq_vs.size())) ) return rc;
	if ( (rc = upload(c,c->d_vst,c->H.dpsq_vst.data(),c->H.dpsq_vst.size())) ) return rc;
	if ( (rc = upload(c,c->d_tab32,c->H.tab32.data(),c->H.tab32.size())) ) return rc;
	if ( (rc = upload(c,c->d_first,c->H.dpsq_first.data(),c->H.dpsq_first.size())) ) return rc;
	if ( (rc = upload(c,c->d_size,c->H.dpsq_size.data(),c->H.dpsq_size.size())) ) return rc;
	if ( (rc = upload(c,c->d_suplo,c->H.suplo.data(),c->H.suplo.size())) ) return rc;
	if ( (rc = upload(c,c->d_suphi,c->H.suphi.data(),c->H.suphi.size())) ) return rc;
	if ( (rc = upload(c,c->d_klim,c->H.klim.data(),c->H.klim.size())) ) return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	DevTables & T = c->T;
	T.nrows = c->H.nrows; T.nsup = c->H.nsup; T.kln = c->H.kln; T.pad = 0;
	T.dpnorm = c->d_dpnorm.p; T.dpsq = c->d_dpsq.p; T.dpsq_vs = c->d_vs.p; T.dpsq_first = c->d_first.p; T.dpsq_size = c->d_size.p;
	T.suplo = c->d_suplo.p; T.suphi = c->d_suphi.p; T.klim = c->d_klim.p;
	dacc_params const & p = c->par;
	DevParams & P = c->P;
	P.w = p.w; P.a = p.a; P.klow = p.klow; P.khigh = p.khigh; P.minff = p.minfilterfreq; P.maxff = p.maxfilterfreq;
	P.minwindowcov = p.minwindowcov; P.checklim = (est_cor != 0.0); P.maxalign = p.maxalign; P.eminrate = p.eminrate;
	P.tspace = p.tspace; P.producefull = p.producefull; P.minlen = p.minlen;
	c->haveprofile = true;
	return DACC_OK;
}

int dacc_debug_tables(dacc_ctx * c, uint64_t * out, uint64_t cap, uint64_t * n, uint64_t klimit_n)
{
	if ( !c || !n ) return DACC_EINVAL;
	if ( !c->haveprofile ) return DACC_ESTATE;
	std::vector<uint64_t> B; serialiseHostTables(c->H,B,klimit_n);
	*n = B.size();
	if ( out ) std::memcpy(out,B.data(),8*std::min<uint64_t>(cap,B.size()));
	return DACC_OK;
}

static int dacc_load_db_body(dacc_ctx * c, uint8_t const * bps, uint64_t bps_bytes, uint64_t const * boff, uint32_t const * rlen, uint64_t nreads)
{
	if ( !c || !bps || !boff || !rlen || !nreads ) return DACC_EINVAL;
	hipSetDevice(c->device);
	for ( uint64_t i = 0; i < nreads; ++i )
		if ( boff[i] + (rlen[i]+3)/4 > bps_bytes ) { c->err = "read store offsets exceed the buffer"; return DACC_EINVAL; }
	int rc;
	HIPCHK(c->d_bps.ensure(bps_bytes+16));
	HIPCHK(hipMemsetAsync(c->d_bps.p,0,bps_bytes+16,c->stream));
	HIPCHK(hipMemcpyAsync(c->d_bps.p,bps,bps_bytes,hipMemcpyHostToDevice,c->stream));
	if ( (rc = upload(c,c->d_boff,boff,nreads)) ) return rc;
	if ( (rc = upload(c,c->d_rlen,rlen,nreads)) ) return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	c->h_rlen.assign(rlen,rlen+nreads);
	c->havedb = true;
	return DACC_OK;
}

// dacc_timing's counters of the stages that pass on untouched what is not theirs, in chain order.  `deeper`: the stage's own share are the windows of more than
// `mins` strings on the list it read (windows + out) and on the list it handed on (out), counted by k_count_deeper into two words of d_work from the final
// window records (behind the scratch retries of the generic engine); else everything on its list is its own: the difference of the two list lengths -- what the
// last stage handed on is what k_window ran, or what the very deep stage read.  The deepest stage and the full-depth stage count with the very deep stage's threshold:
// what the deepest stage read with more than VDEEP_MINS strings is vdeep_out where that stage ran, what the full-depth stage read is xdeep_out where the deepest ran.  The wide deep stage (wide batches, where none of those three runs) reads what the last stage handed on.  `ms`: a trailing stage's kernel time (the deep-window tier's has a start event of its own)
struct StageCounters { TierId id; float dacc_timing::* ms; uint32_t dacc_timing::* windows, dacc_timing::* out; bool deeper; uint32_t mins, countwords; };
static StageCounters const STAGE_COUNTERS[] = {
	{ ID_DEEP, nullptr, &dacc_timing::deep_windows, &dacc_timing::deep_out, true, FastTier<12>::mins, WORK_DEEP_COUNT },
	{ ID_LAST, &dacc_timing::last_ms, &dacc_timing::last_windows, &dacc_timing::last_out, false, 0, 0 },
	{ ID_VDEEP, &dacc_timing::vdeep_ms, &dacc_timing::vdeep_windows, &dacc_timing::vdeep_out, true, VDEEP_MINS, WORK_VDEEP_COUNT },
	{ ID_XDEEP, &dacc_timing::xdeep_ms, &dacc_timing::xdeep_windows, &dacc_timing::xdeep_out, true, VDEEP_MINS, WORK_XDEEP_COUNT },
	{ ID_FDEEP, &dacc_timing::fdeep_ms, &dacc_timing::fdeep_windows, &dacc_timing::fdeep_out, true, VDEEP_MINS, WORK_FDEEP_COUNT },
	{ ID_WDEEP, &dacc_timing::wdeep_ms, &dacc_timing::wdeep_windows, &dacc_timing::wdeep_out, true, VDEEP_MINS, WORK_WDEEP_COUNT },
	// (the stage of a w = 128 batch reads every window of the batch -- no list -- and its time runs from the end of the trace kernels: fetchStageCounters)
	{ ID_W128, &dacc_timing::w128_ms, &dacc_timing::w128_windows, &dacc_timing::w128_out, false, 0, 0 } };

// ---- the device pass (runDevice): one function per phase, in the order they run; they share the context and the state of the pass
// DACC_DEBUG_SYNC=1: wait for every kernel of the generic-only path and say so on stderr (a device fault then names its kernel)
static bool dbgSync() { static bool const on = getenv("DACC_DEBUG_SYNC") && getenv("DACC_DEBUG_SYNC")[0] == '1'; return on; }
static void mark(dacc_ctx * c, char const * what) { if ( dbgSync() ) { hipError_t const e = hipStreamSynchronize(c->stream); std::fprintf(stderr,"[dacc] %s: %s\n",what,hipGetErrorString(e)); std::fflush(stderr); } }
// a stage's work counter (DACC_SCHED bit 0: the tiers pull their windows from a counter)
static uint32_t * workCounter(dacc_ctx * c, uint32_t const off) { return (c->sched&1) ? c->d_work.p+off : static_cast<uint32_t *>(0); }
static dacc_ctx::Stage * ranOf(dacc_ctx * c, TierId const id) { return c->st[id].ran ? &c->st[id] : static_cast<dacc_ctx::Stage *>(0); }
// a batch of w = 128 in which no slot runs: the generic engine's launch geometry and events, as before the stage of w = 128 existed (its model table is one the
// wide tiers' pipeline admits since then -- TP.usefast --, but no slot, no pre-scan and no second stream run), and that stage (ID_W128) in front of k_window where it is resolved
static bool aloneBatch(dacc_ctx const * c) { return c->TP.usefast && !c->TP.anytier() && c->par.w == W128; }

struct Pass
{
	WindowBatch WB;                  // the batch's record; pregen: the pre-scan's first map once the chain starts
	uint32_t const * list = 0;       // what the last slot or trailing stage that ran handed on (0: all windows)
	int lastslot = -1;               // the last slot that ran
	bool early = false;              // the first slot that runs has run: the early generic list is closed, the second stream may read it
	uint32_t herr[4] = {0,0,0,0};    // d_err behind the last vote: generic engine out of scratch, vote, trace, a window handed on and never run
	size_t symbytes = 0;             // the symbol stream of the batch
};

// the batch's record for the window kernels (the main pass's: with its profile counters), no pregen map
static WindowBatch windowBatch(dacc_ctx * c)
{
	BatchPlan & BP = c->BP; WindowBatch WB;
	WB.P = c->P; WB.T = c->T; WB.C = BP.caps; WB.bps = c->d_bps.p; WB.boff = c->d_boff.p; WB.rlen = c->d_rlen.p;
	WB.piles = c->d_piles.p; WB.npiles = BP.piles.size(); WB.ovl = c->d_ovl.p; WB.wt_b = c->d_wt_b.p; WB.wt_e = c->d_wt_e.p;
	WB.nwindows = BP.nwindows; WB.wrec = c->d_wrec.p; WB.wout = c->d_wout.p; WB.arena = c->d_arena.p; WB.prof = c->d_prof.p;
	return WB;
}
// the base record of stage `id`: the batch's record, the stage's capacities, the model tables, the switches and, for a stage of the main stream's chain, the hand-over
// slots and the ledger mask.  What differs from launch to launch (hand-on list, early list, slab and stride, pregen map, arena) is stated where the launch is
static FastBatch stageBatch(dacc_ctx * c, WindowBatch const & WB, uint32_t const id, bool const chain = true)
{
	FastBatch FB; FB.W = WB; FB.F = c->BP.stageCaps(id); FB.dpsq_vst = c->d_vst.p; FB.tab32 = c->d_tab32.p; FB.feasneed = c->env_feasneed; FB.tiefast = c->env_tiefast;
	if ( !chain ) return FB;
	// (a wide batch has handcap == 0, dacc_submit_piles: its hand-overs go to the generic engine, which sorts for itself)
	FB.hand = c->handcap ? c->d_hand.p : static_cast<uint64_t *>(0); FB.handctr = c->d_handctr.p; FB.handcap = c->handcap; FB.handwords = c->TP.handwords;
#if defined(DACC_LEDGER)
	{ char const * lm = getenv("DACC_LEDGER_MASK"); FB.ledger = lm ? static_cast<uint32_t>(strtoul(lm,0,0)) : 0u; }      // (scripts/ledger.py)
#endif
	return FB;
}
// where the record's stage hands on, and its slab (one stride of the stage's gbytes per workgroup)
static void handsOn(FastBatch & FB, uint32_t * const handon, uint8_t * const slab) { FB.retry = handon; FB.gslab = slab; FB.gstride = FB.F.gbytes; }
// The launch of stage `id` on the main stream: its tier's kernel over `in` (0: all windows) with the record FB, no LDS for a layout in device memory.  A trailing stage and
// the stage of w = 128 own their hand-on list and clear it here; a front tier's holds the pre-pass's windows by now and a main tier's the pre-scan's (enqueueSlot,
// enqueuePrescan).  A main tier is done at its slot's event (runDevice), every other stage at its own.  what: the launch's name for DACC_DEBUG_SYNC
static int launchStage(dacc_ctx * c, uint32_t const id, FastBatch const & FB, uint32_t const * const in, char const * const what = 0)
{
	dacc_ctx::Stage & S = c->st[id]; TierStage const & R = TIER_CHAIN[id]; hipStream_t const s = c->stream;
	if ( R.role == ROLE_LAST || R.role == ROLE_ALONE ) HIPCHK(hipMemsetAsync(S.handon.p,0,sizeof(uint32_t),s));
	hipLaunchKernelGGL(fastKernel(c->TP.tier[id]),dim3(S.grid),dim3(64),FB.F.gmem ? 0u : FB.F.ldsbytes,s,FB,in,workCounter(c,R.work));
	if ( what ) mark(c,what);
	if ( R.role != ROLE_MAIN ) { HIPCHK(hipEventRecord(S.done,s)); S.ran = true; S.in = in; }      // (a main tier keeps no run state: its slot's event and list say it)
	return DACC_OK;
}
// The stages whose slab an allocation failure gives back (dacc_drop_hand) and that the retried call and the rest of the context run without (`noslab`): a row with a slab
// budget of its own, and the stage of w = 128 whatever its budget (a build with DACC_W128_SLAB_MB=0 gives it the common one, and `.slab` alone would then miss it)
static bool ownSlab(uint32_t const id) { return TIER_CHAIN[id].slab || TIER_CHAIN[id].role == ROLE_ALONE; }
// The hand-on list (what the next stage or the generic engine reads) and the slab, grid x gbytes, of an optional device-memory stage: a trailing stage, the stage of
// w = 128, the long string stage.  Optional like the hand-over buffer: a device that cannot spare them runs the batch without the stage, on the route it had before
static int reserveStage(dacc_ctx * c, uint32_t const id, DevBuf<uint32_t> & handon, DevBuf<uint8_t> & slab, uint32_t const grid)
{
	if ( ownSlab(id) && c->noslab ) { slab.release(); c->TP.ok[id] = false; return DACC_OK; }
	hipError_t e = handon.ensure(c->BP.nwindows+2);
	if ( e == hipSuccess ) e = slab.ensure(static_cast<size_t>(grid)*c->BP.stageCaps(id).gbytes + 256);
	if ( e == hipErrorOutOfMemory ) { (void)hipGetLastError(); slab.release(); c->TP.ok[id] = false; return DACC_OK; }
	HIPCHK(e);
	return DACC_OK;
}

// 1. second use of this context: now the hand-over buffer pays (dacc_submit_piles); an optimisation only -- if the device cannot spare it, halve it, and in the end do without
static void growHandOver(dacc_ctx * c)
{
	if ( !(c->nruns && c->handwant > c->handcap && !c->nohand) ) return;
	uint64_t cap = c->handwant;
	// never more than half of what the device has free right now: the buffer is an optimisation and must not be what makes a later, larger
	// batch of this context (or of another worker on the same device) fail its mandatory buffers
	{ size_t fr = 0, tot = 0; if ( hipMemGetInfo(&fr,&tot) == hipSuccess ) { uint64_t const lim = (static_cast<uint64_t>(fr)/2) / (static_cast<uint64_t>(c->TP.handwords)*8ull); if ( cap > lim ) cap = lim; } else (void)hipGetLastError(); }
	while ( cap && c->d_hand.ensure(static_cast<size_t>(cap)*c->TP.handwords) != hipSuccess ) { (void)hipGetLastError(); cap = cap > 65536 ? cap/2 : 0; }
	c->handcap = static_cast<uint32_t>(cap); c->handwant = cap;
}

// 2. block task table, then the trace points of every block -> the window tables
static int enqueuePrepAndTrace(dacc_ctx * c)
{
	BatchPlan & BP = c->BP; hipStream_t const s = c->stream;
	HIPCHK(hipMemsetAsync(c->d_err.p,0,4*sizeof(uint32_t),s));
	HIPCHK(hipEventRecord(c->ev[0],s));
	if ( BP.ovl.size() )
	{
		PrepBatch PB; PB.ovl = c->d_ovl.p; PB.novl = BP.ovl.size(); PB.trace = c->d_trace.p; PB.trace_bytes = c->trace_bytes; PB.blk_ovl = c->d_blk_ovl.p; PB.blk_b0 = c->d_blk_b0.p;
		hipLaunchKernelGGL(k_prep,dim3((BP.ovl.size()+255)/256),dim3(256),0,s,PB);
	}
	if ( BP.nblocks )
	{
		TraceBatch TB;
		TB.P = c->P; TB.bps = c->d_bps.p; TB.boff = c->d_boff.p; TB.rlen = c->d_rlen.p;
		TB.piles = c->d_piles.p; TB.ovl = c->d_ovl.p; TB.ovl_pile = c->d_ovl_pile.p; TB.trace = c->d_trace.p;
		TB.blk_ovl = c->d_blk_ovl.p; TB.blk_b0 = c->d_blk_b0.p; TB.nblocks = BP.nblocks; TB.wt_b = c->d_wt_b.p; TB.wt_e = c->d_wt_e.p;
		TB.maxcols = BP.maxcols; TB.trace_bytes = c->trace_bytes; TB.errflag = c->d_err.p + 2; TB.slab = c->d_trslab.p;
		TB.work = (c->env_trdyn && traceCounterHolds(BP.nblocks)) ? c->d_work.p + WORK_TRACE : static_cast<uint32_t *>(0);
		if ( TB.work ) HIPCHK(hipMemsetAsync(TB.work,0,sizeof(uint32_t),s));
		if ( c->tr_words == 2 ) hipLaunchKernelGGL(k_trace,dim3(c->tr_grid),dim3(64),c->tr_lds,s,TB);
		else if ( c->tr_words == 4 ) hipLaunchKernelGGL(k_trace_wide<4>,dim3(c->tr_grid),dim3(64),c->tr_lds,s,TB,c->tr_lanes);
		else hipLaunchKernelGGL(k_trace_wide<8>,dim3(c->tr_grid),dim3(64),c->tr_lds,s,TB,c->tr_lanes);
	}
	mark(c,"prep + trace");
	HIPCHK(hipEventRecord(c->ev[1],s));
	return DACC_OK;
}

// 3. windows only the generic engine can run (a string longer than 64 bases): found by a scan of the window tables, for the second stream to start
// concurrently with all LDS tiers; then the lists and counters of the chain are cleared
static int enqueuePrescan(dacc_ctx * c, Pass & P)
{
	BatchPlan & BP = c->BP; TierPipeline & TP = c->TP; hipStream_t const s = c->stream;
	HIPCHK(hipMemsetAsync(c->d_pregen.p,0,((BP.nwindows+31)/32+1)*sizeof(uint32_t),s));
	HIPCHK(hipMemsetAsync(c->d_pregen2.p,0,((BP.nwindows+31)/32+1)*sizeof(uint32_t),s));
	HIPCHK(hipMemsetAsync(c->d_pregenlist.p,0,sizeof(uint32_t),s));
	for ( int i = 0; i < TIER_NSLOTS; ++i ) HIPCHK(hipMemsetAsync(c->d_retry[i].p,0,sizeof(uint32_t),s));
	if ( BP.ovl.size() )
	{
		hipLaunchKernelGGL(k_prescan,dim3((BP.ovl.size()+3)/4),dim3(256),0,s,c->d_ovl.p,static_cast<uint64_t>(BP.ovl.size()),c->d_ovl_pile.p,c->d_piles.p,c->d_wt_b.p,c->d_wt_e.p,c->d_pregen.p,c->d_pregen2.p,TP.widetier ? 128u : 64u);
		// windows with a string of 65 ... 128 bases join the first slot's hand-overs when the second slot's tier holds such strings (tiers 6 / 3;
		// a deep batch's tier 2 does not: it hands them on to tier 3 at its length check) and the first slot runs at all
		hipLaunchKernelGGL(k_prescan_lists,dim3(((BP.nwindows+31)/32+255)/256),dim3(256),0,s,c->d_pregen.p,c->d_pregen2.p,static_cast<uint64_t>(BP.nwindows),c->d_pregenlist.p,
			TP.slot1_long ? c->d_retry[0].p : static_cast<uint32_t *>(0),c->d_wout.p);
	}
	HIPCHK(hipEventRecord(c->evPrescan,s));
	c->nlong[0] = c->nlong[1] = 0; c->longran[0] = c->longran[1] = false;
	P.WB.pregen = c->d_pregen.p;
	HIPCHK(hipMemsetAsync(c->d_gearly.p,0,sizeof(uint32_t),s));
	HIPCHK(hipMemsetAsync(c->d_handctr.p,0,sizeof(uint32_t),s));
	HIPCHK(hipMemsetAsync(c->d_work.p,0,WORK_LONGSTR*sizeof(uint32_t),s));      // (the long string stage's counters are the second stream's: cleared there, in front of its launch)
	return DACC_OK;
}

// 4. one slot of the chain (tier_pipeline.hpp): the pre-pass and the front tiers of the slot that run in this pass, each handing on to the next stage of the
// slot, then its main tier; it takes the windows the slot in front handed over (P.list = 0: all windows)
static int enqueueSlot(dacc_ctx * c, Pass & P, uint32_t const slot)
{
	BatchPlan & BP = c->BP; TierPipeline & TP = c->TP; hipStream_t const s = c->stream; int rc;
	if ( !TP.slotok(slot) ) return DACC_OK;
	int const m = TIER_MAIN[slot];
	FastBatch FB = stageBatch(c,P.WB,m); handsOn(FB,c->d_retry[slot].p,c->d_gslab.p);
	// the first slot's tiers skip every window with a string of more than 64 bases; the later ones only those the second stream has (without the 128-base route: all of them)
	if ( (slot > 0 && TP.late_long) || TP.widetier ) FB.W.pregen = c->d_pregen2.p;
	// only the first tier feeds the early generic list (its kernel reads the list once, right after that tier): a window that reaches a later tier first
	// (mao beyond the earlier tier) and turns out to be generic-only takes the ordinary hand-over chain to the generic kernel at the end
	FB.gearly = P.early ? static_cast<uint32_t *>(0) : c->d_gearly.p;
	// (tier 7 switches itself off for the rest of a context's batches when it hands on more than a fifth of what it runs: on the
	// ONT mix at k = 10 / 12 a third / a quarter of its windows overflow it late, on their stretches and pools, and the class costs
	// 2.6 / 1.4 % instead of gaining the 3 % it gains at k = 14 and 16 and on config 2, profiles/r06j; results do not depend on it)
	int fr[TIER_NSTAGES]; uint32_t nfr = 0;
	for ( int i = 0; i < m; ++i ) if ( TIER_CHAIN[i].slot == slot && TP.ok[i] && !((TIER_CHAIN[i].flags & STAGE_ADAPTIVE) && c->tier7_adapt_off) ) fr[nfr++] = i;
	bool const classed = nfr && (TIER_CHAIN[fr[0]].flags & STAGE_PREPASS);
	if ( classed ) HIPCHK(hipMemsetAsync(c->d_small.p,0,sizeof(uint32_t),s));
	for ( uint32_t k = 0; k < nfr; ++k ) HIPCHK(hipMemsetAsync(c->st[fr[k]].handon.p,0,sizeof(uint32_t),s));
	uint32_t const * in = P.list;
	if ( classed )
	{
		// size classes: the small windows run in tier 0 (8 wavefronts per CU), the middle class and tier 0's hand-overs in tier 7
		// (7 per CU), tier 7's hand-overs and all other windows in tier 1 (6 per CU); without tier 7 the middle class counts as big
		uint32_t * const mid = c->st[fr[0]].handon.p, * const big = c->st[fr[nfr-1]].handon.p;
		hipLaunchKernelGGL(k_classify,dim3((BP.nwindows+255)/256),dim3(256),0,s,P.WB,c->d_small.p,mid,big,c->sw.t0inst,nfr > 1 ? c->sw.t7inst : 0u);
		// (what the pre-pass itself put on the middle and the big list, before the tiers' hand-overs join them: for the counters of dacc_timing)
		if ( nfr > 1 ) { HIPCHK(hipMemcpyAsync(c->d_work.p+WORK_PRE_MID,mid,sizeof(uint32_t),hipMemcpyDeviceToDevice,s)); HIPCHK(hipMemcpyAsync(c->d_work.p+WORK_PRE_BIG,big,sizeof(uint32_t),hipMemcpyDeviceToDevice,s)); }
		in = c->d_small.p;
	}
	for ( uint32_t k = 0; k < nfr; ++k )
	{
		FastBatch FF = FB; FF.F = BP.stageCaps(fr[k]); handsOn(FF,c->st[fr[k]].handon.p,FB.gslab);
		if ( (rc = launchStage(c,fr[k],FF,in)) ) return rc;
		in = c->st[fr[k]].handon.p;
	}
	if ( (rc = launchStage(c,m,FB,in)) ) return rc;      // (a device-memory tier in a slot, DACC_LAST_AS_SLOT2=1: no LDS)
	P.list = c->d_retry[slot].p; P.lastslot = static_cast<int>(slot);
	if ( !P.early )
	{
		// the first tier has seen every window: what only the generic engine can run starts now, on its own (high priority) stream and arena, while the remaining tiers run
		P.early = true;
		HIPCHK(hipEventRecord(c->evFirstTier,s));
	}
	return DACC_OK;
}

// 5. the trailing stages (tier_pipeline.hpp: layout in device memory), in chain order: each takes the list the stage or slot in front of it that ran
// handed on and hands on to the next, the last to the generic engine; one that does not run (switched off, no window deep enough in the batch)
// leaves the list as it is.  They skip the windows the second stream has, like every slot behind the first, and feed no early list (the early
// kernel has read its list)
static int enqueueTrailingStages(dacc_ctx * c, Pass & P)
{
	TierPipeline & TP = c->TP; int rc;
	for ( uint32_t i = 0; i < TIER_NROWS; ++i )
		if ( TIER_CHAIN[i].role == ROLE_LAST && TP.ok[i] && P.list && P.lastslot >= 0 )
		{
			dacc_ctx::Stage & S = c->st[i];
			FastBatch FZ = stageBatch(c,P.WB,i); handsOn(FZ,S.handon.p,S.slab.p);
			FZ.W.pregen = (TP.late_long || TP.widetier) ? c->d_pregen2.p : c->d_pregen.p;
			if ( (rc = launchStage(c,i,FZ,P.list)) ) return rc;
			P.list = S.handon.p;
		}
	return DACC_OK;
}

// 6. DACC_DEBUG_RETRY: which windows did the last LDS tier hand on, and why (flags of its FFAIL)
static int dumpRetryFlags(dacc_ctx * c, uint32_t const * const list)
{
	HIPCHK(hipStreamSynchronize(c->stream));
	uint32_t n = 0; HIPCHK(hipMemcpy(&n,list,sizeof(uint32_t),hipMemcpyDeviceToHost));
	std::vector<uint32_t> idx(n); if ( n ) HIPCHK(hipMemcpy(idx.data(),list+1,n*sizeof(uint32_t),hipMemcpyDeviceToHost));
	c->retry_flags.clear();
	for ( uint32_t i = 0; i < n; ++i ) { WindowOut o; HIPCHK(hipMemcpy(&o,c->d_wout.p+idx[i],sizeof(WindowOut),hipMemcpyDeviceToHost)); c->retry_flags.push_back(idx[i]); c->retry_flags.push_back(o.flags); c->retry_flags.push_back(o.mao); c->retry_flags.push_back(static_cast<uint32_t>(o.filterfreq)); }
	return DACC_OK;
}

// 7b. one list of the second stream.  The length of the list is fetched before its launch and the grid follows it: an empty list -- the rule at the
// default window -- is not launched at all, a list of three windows asks for three CUs' worth of LDS instead of 256.
// The 4 byte copy and the wait run on the SECOND stream, behind the event of the kernel that fills the list, and only after every tier and the
// generic kernel have been queued on the main stream: a wait in the middle of the chain keeps the host -- and a second context's batches on the
// same device -- out of the queue until the first tier has retired.
static int launchLong(dacc_ctx * c, FastBatch & FL, uint32_t const * const lst, hipEvent_t const filled, uint32_t const which)
{
	BatchPlan & BP = c->BP; TierPipeline & TP = c->TP;
	uint32_t & nlist = c->nlong[which]; nlist = 0;
	HIPCHK(hipStreamWaitEvent(c->stream2,filled,0));
	HIPCHK(hipMemcpyAsync(&nlist,lst,sizeof(uint32_t),hipMemcpyDeviceToHost,c->stream2));
	HIPCHK(hipStreamSynchronize(c->stream2));
	if ( !nlist ) return DACC_OK;
	uint32_t const * glist = lst;      // what the generic engine of this stream reads
	if ( TP.ok[ID_LONG] && TP.tier[ID_LONG] != 5 )
	{
		// the long string stage of a wide batch (tier 17: strings of up to 255 bases, layout in device memory): a kernel of its own over the list, no
		// LDS, a slab of grid x gbytes and a hand-on list, both reserved here, where the list is known not to be empty (the second stream is idle: the
		// copy above has been waited for)
		FastCaps const & F = BP.stageCaps(ID_LONG);
		uint32_t const grid = tierGridGmem(F.gbytes,nlist);
		int const rc = reserveStage(c,ID_LONG,c->d_longhand[which],c->d_longslab,grid); if ( rc ) return rc;
		if ( TP.ok[ID_LONG] )
		{
			// (not launchStage: the second stream, a grid that follows the list, a counter per list and events on both sides of the launch)
			FastBatch FS = FL; FS.F = F; handsOn(FS,c->d_longhand[which].p,c->d_longslab.p);
			uint32_t * const wk = (c->sched&1) ? c->d_work.p + TIER_CHAIN[ID_LONG].work + 8u*which : static_cast<uint32_t *>(0);
			HIPCHK(hipMemsetAsync(FS.retry,0,sizeof(uint32_t),c->stream2));
			if ( wk ) HIPCHK(hipMemsetAsync(wk,0,8*sizeof(uint32_t),c->stream2));
			HIPCHK(hipEventRecord(c->evLong[2*which],c->stream2));
			hipLaunchKernelGGL(fastKernel(TP.tier[ID_LONG]),dim3(grid),dim3(64),0,c->stream2,FS,lst,wk);
			HIPCHK(hipEventRecord(c->evLong[2*which+1],c->stream2));
			c->longran[which] = true;
			glist = FS.retry;      // (its length is read on the device: workgroups beyond it leave at once)
		}
	}
	uint32_t const grid = nlist < c->early_grid ? nlist : c->early_grid;
	(void)hipGetLastError();
	hipLaunchKernelGGL(k_window_long,dim3(grid),dim3(64),FL.F.ldsbytes,c->stream2,FL,c->d_err.p,glist);
	// a launch the device refuses (the LDS of a whole CU) falls back to the generic engine alone, for good
	if ( FL.F.ldsbytes && hipGetLastError() != hipSuccess )
	{
		TP.ok[ID_LONG] = false; FL.F.ldsbytes = 0;
		hipLaunchKernelGGL(k_window_long,dim3(grid),dim3(64),0,c->stream2,FL,c->d_err.p,glist);
	}
	return DACC_OK;
}

// 7. what is left (rare shapes) goes through the generic engine.  Then, the main stream's queue being full, the second stream: the pre-scan's list (a
// string of more than 64 bases) as soon as the pre-scan is done, the first tier's generic-only windows behind the first tier
static int enqueueGenericAndSecondStream(dacc_ctx * c, Pass & P)
{
	TierPipeline & TP = c->TP; hipStream_t const s = c->stream; int rc;
	hipLaunchKernelGGL(k_window,dim3(c->retry_grid),dim3(64),0,s,P.WB,c->d_err.p,P.list,(c->sched&2) ? c->d_work.p+WORK_GENERIC : static_cast<uint32_t *>(0));
	// the second stream's record: its own arena, no profile counters, every window of its list, no hand-over slots
	FastBatch FL = stageBatch(c,P.WB,ID_LONG,false); FL.W.arena = c->d_arena2.p; FL.W.prof = 0; FL.W.pregen = 0;
	// (k_window_long runs tier 5 in its own LDS; a wide batch's ID_LONG is tier 17, a kernel of its own in front of it -- k_window_long then is the generic
	// engine alone and never sees that tier's capacities)
	bool const long5 = TP.ok[ID_LONG] && TP.tier[ID_LONG] == 5;
	if ( TP.tier[ID_LONG] != 5 ) FL.F = tierCaps(5,c->H.nrows,c->H.nsup);
	if ( !long5 ) FL.F.ldsbytes = 0;
	if ( (rc = launchLong(c,FL,c->d_pregenlist.p,c->evPrescan,0)) ) return rc;
	if ( P.early && (rc = launchLong(c,FL,c->d_gearly.p,c->evFirstTier,1)) ) return rc;
	// everything the second stream ran (pre-scan list, first tier's generic-only windows) must be done before the vote
	HIPCHK(hipEventRecord(c->evEarlyGeneric,c->stream2));
	HIPCHK(hipStreamWaitEvent(s,c->evEarlyGeneric,0));
	return DACC_OK;
}

// 8. pending records -> final ones, the check that every window was run, the vote; then the error flags, fragments and symbols come back
static int voteAndFetch(dacc_ctx * c, Pass & P)
{
	BatchPlan & BP = c->BP; hipStream_t const s = c->stream;
	HIPCHK(hipMemsetAsync(c->d_pilebad.p,0,BP.piles.size()+1,s));
	// the tiers' pending records become final ones (every engine is done: the main stream has waited for the second one); on the
	// path where all windows went through k_window it finds nothing pending
	HIPCHK(hipEventRecord(c->evEmit[0],s));
	if ( BP.nwindows ) { hipLaunchKernelGGL(k_emit,dim3((BP.nwindows+255)/256),dim3(256),0,s,c->d_wrec.p,static_cast<uint64_t>(BP.nwindows),c->par.w); mark(c,"k_emit"); }
	HIPCHK(hipEventRecord(c->evEmit[1],s));
	if ( BP.nwindows ) hipLaunchKernelGGL(k_check_done,dim3((BP.nwindows+255)/256),dim3(256),0,s,c->d_wout.p,BP.nwindows,c->d_err.p+3,c->d_piles.p,static_cast<uint32_t>(BP.piles.size()),c->d_pilebad.p);
	if ( BP.piles.size() )
	{
		VoteBatch VB;
		VB.P = c->P; VB.bps = c->d_bps.p; VB.boff = c->d_boff.p; VB.rlen = c->d_rlen.p; VB.piles = c->d_piles.p; VB.npiles = BP.piles.size();
		VB.wrec = c->d_wrec.p; VB.has = c->d_has.p; VB.ld0 = c->d_ld0.p; VB.oc = c->d_oc.p; VB.ocs = c->d_ocs.p; VB.outsym = c->d_outsym.p;
		VB.frags = c->d_frags.p; VB.fragbase = c->d_fragbase.p; VB.nfrag = c->d_nfrag.p; VB.errflag = c->d_err.p + 1; VB.pilebad = c->d_pilebad.p;
		mark(c,"k_check_done");
		hipLaunchKernelGGL(k_vote,dim3(BP.piles.size()),dim3(256),0,s,VB);
		mark(c,"k_vote");
	}
	HIPCHK(hipEventRecord(c->ev[3],s));
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(P.herr,c->d_err.p,sizeof(P.herr),hipMemcpyDeviceToHost,s));
	if ( BP.piles.size() )
	{
		HIPCHK(hipMemcpyAsync(c->h_nfrag.data(),c->d_nfrag.p,BP.piles.size()*sizeof(uint32_t),hipMemcpyDeviceToHost,s));
		HIPCHK(hipMemcpyAsync(c->h_frags.data(),c->d_frags.p,BP.nfragslots*sizeof(VoteFragment),hipMemcpyDeviceToHost,s));
		HIPCHK(hipMemcpyAsync(c->h_outsym.p,c->d_outsym.p,P.symbytes,hipMemcpyDeviceToHost,s));
	}
	HIPCHK(hipEventRecord(c->ev[4],s));
	HIPCHK(hipStreamSynchronize(s));
	return DACC_OK;
}

// 9. dacc_timing's counters of the slots and of the front tiers: tier 0 and tier 7 are the first slot's (size classes), tier 10 the last slot's (dense
// graphs; tier 11 in deep batches); and tier 7's adaptive switch
static int fetchTierCounters(dacc_ctx * c)
{
	BatchPlan & BP = c->BP; TierPipeline & TP = c->TP;
	dacc_ctx::Stage * const f0 = ranOf(c,ID_T0), * const f7 = ranOf(c,ID_T7), * const fD = ranOf(c,ID_DENSE);
	for ( int i = 0; i < 3; ++i ) c->timing.tier_out[i] = 0;
	if ( TP.usefast && BP.nwindows ) for ( int i = 0; i < 3; ++i ) if ( TP.slotok(i) ) HIPCHK(hipMemcpy(&c->timing.tier_out[i],c->d_retry[i].p,sizeof(uint32_t),hipMemcpyDeviceToHost));
	c->timing.tier10_out = 0;
	if ( fD ) HIPCHK(hipMemcpy(&c->timing.tier10_out,fD->handon.p,sizeof(uint32_t),hipMemcpyDeviceToHost));
	c->timing.tier0_in = 0; c->timing.tier0_out = 0; c->timing.tier7_in = 0; c->timing.tier7_out = 0;
	c->timing.long_windows = 0; c->timing.long_first_tier = 0;      // (a pass that does not get to the second stream ran nothing there)
	if ( !(TP.usefast && BP.nwindows && TP.anytier()) ) return DACC_OK;
	// length of the two lists of the second stream (pre-scan, first tier's generic-only windows), fetched before their launches
	uint32_t const n1 = c->nlong[0], n2 = c->nlong[1];
	c->timing.long_windows = n1 + n2; c->timing.long_first_tier = n2;
	if ( !f0 ) return DACC_OK;
	// size classes: the pre-pass sent nsmall windows to tier 0, nmid0 to the middle list and nwindows - nsmall - nmid0 - n1 to the big
	// list; tier 0's hand-overs have joined the middle list since (the big list without tier 7), tier 7's the big list
	uint32_t nsmall = 0, nbig = 0, nmid = 0;
	HIPCHK(hipMemcpy(&nsmall,c->d_small.p,sizeof(uint32_t),hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(&nbig,(f7 ? f7 : f0)->handon.p,sizeof(uint32_t),hipMemcpyDeviceToHost));
	if ( f7 ) HIPCHK(hipMemcpy(&nmid,f0->handon.p,sizeof(uint32_t),hipMemcpyDeviceToHost));
	c->timing.tier0_in = nsmall;
	if ( !f7 )
	{
		uint64_t const big0 = BP.nwindows - std::min<uint64_t>(BP.nwindows,static_cast<uint64_t>(nsmall) + n1);
		c->timing.tier0_out = nbig > big0 ? static_cast<uint32_t>(nbig - big0) : 0u;
	}
	else
	{
		// nmid = what the pre-pass put on the middle list + tier 0's hand-overs, nbig = the pre-pass's big windows + tier 7's hand-overs
		uint32_t pre[2] = {0,0};
		HIPCHK(hipMemcpy(pre,c->d_work.p+WORK_PRE_MID,2*sizeof(uint32_t),hipMemcpyDeviceToHost));
		uint32_t const t7out = nbig > pre[1] ? nbig - pre[1] : 0u;
		c->timing.tier0_out = nmid > pre[0] ? nmid - pre[0] : 0u;
		c->timing.tier7_in = nmid; c->timing.tier7_out = t7out;
		if ( c->env_t7adapt && nmid >= 4096 && static_cast<uint64_t>(t7out)*5 > nmid ) c->tier7_adapt_off = true;
	}
	return DACC_OK;
}

// 10. a window the generic engine could not hold (dense graph at small k): grow its scratch capacities and run those
// windows again, then the vote (rare; the capacities stay grown for the rest of the batch geometry)
static int scratchRetry(dacc_ctx * c, Pass & P)
{
	BatchPlan & BP = c->BP; hipStream_t const s = c->stream;
	for ( int attempt = 0; P.herr[0] && !P.herr[1] && !P.herr[2] && attempt < 3; ++attempt )
	{
		growArenaCaps(BP.caps,c->par.w);
		Arena Atmp; BP.caps.bytes = arena_carve(Atmp,0,BP.caps,c->par.w);
		uint32_t const g = boundByArena(c->retry_grid < 64 ? c->retry_grid : 64,BP.caps.bytes,4);
		c->retry_grid = g; c->win_grid = g; if ( c->early_grid > g ) c->early_grid = g;     // later launches of this batch use the grown arenas
		HIPCHK(c->d_arena.ensure(static_cast<size_t>(g)*BP.caps.bytes));
		if ( c->TP.usefast && !aloneBatch(c) ) HIPCHK(c->d_arena2.ensure(static_cast<size_t>(c->early_grid)*BP.caps.bytes));
		HIPCHK(c->d_gearly.ensure(BP.nwindows+2)); HIPCHK(c->d_pregenlist.ensure(BP.nwindows+2)); HIPCHK(c->d_pregen.ensure((BP.nwindows+31)/32+2)); HIPCHK(c->d_pregen2.ensure((BP.nwindows+31)/32+2));
		HIPCHK(hipMemsetAsync(c->d_err.p,0,4*sizeof(uint32_t),s));
		HIPCHK(hipMemsetAsync(c->d_gearly.p,0,sizeof(uint32_t),s));
		hipLaunchKernelGGL(k_collect_overflow,dim3((BP.nwindows+255)/256),dim3(256),0,s,c->d_wout.p,BP.nwindows,c->d_gearly.p);
		mark(c,"k_collect_overflow");
		if ( dbgSync() ) std::fprintf(stderr,"[dacc] scratch retry %d: grid %u, arena %llu bytes per wavefront\n",attempt,g,static_cast<unsigned long long>(BP.caps.bytes));
		WindowBatch WB = windowBatch(c); WB.prof = 0;      // (the grown capacities and arena)
		hipLaunchKernelGGL(k_window,dim3(g),dim3(64),0,s,WB,c->d_err.p,static_cast<uint32_t const *>(c->d_gearly.p),static_cast<uint32_t *>(0));
		mark(c,"k_window (scratch retry)");
		int const rc = voteAndFetch(c,P); if ( rc ) return rc;
	}
	return DACC_OK;
}

// 11. the counters of the deep-window tier and of the trailing stages (STAGE_COUNTERS), zero for a stage that did not run.  A trailing stage's time runs from
// the nearest trailing stage in front of it that ran, else from the last slot.  Then the long string stage's
static int fetchStageCounters(dacc_ctx * c)
{
	BatchPlan & BP = c->BP; TierPipeline & TP = c->TP; hipStream_t const s = c->stream;
	hipEvent_t from = c->evslot[TIER_NSLOTS-1];
	for ( StageCounters const & K : STAGE_COUNTERS )
	{
		dacc_ctx::Stage const & S = c->st[K.id];
		c->timing.*K.windows = 0; c->timing.*K.out = 0; if ( K.ms ) c->timing.*K.ms = 0;
		bool const alone = TIER_CHAIN[K.id].role == ROLE_ALONE;      // the stage of a w = 128 batch: all windows, no stage in front of it
		if ( !S.ran || (!S.in && !alone) ) continue;
		uint32_t cnt[2] = {0,0};      // what it read, what it handed on
		if ( K.deeper )
		{
			HIPCHK(hipMemsetAsync(c->d_work.p+K.countwords,0,2*sizeof(uint32_t),s));
			hipLaunchKernelGGL(k_count_deeper,dim3(64),dim3(256),0,s,S.in,static_cast<uint32_t const *>(S.handon.p),c->d_wout.p,K.mins,c->d_work.p+K.countwords);
			HIPCHK(hipMemcpyAsync(cnt,c->d_work.p+K.countwords,sizeof(cnt),hipMemcpyDeviceToHost,s));
			HIPCHK(hipStreamSynchronize(s));
		}
		else
		{
			if ( S.in ) HIPCHK(hipMemcpy(&cnt[0],S.in,sizeof(uint32_t),hipMemcpyDeviceToHost)); else cnt[0] = static_cast<uint32_t>(BP.nwindows);
			HIPCHK(hipMemcpy(&cnt[1],S.handon.p,sizeof(uint32_t),hipMemcpyDeviceToHost));
		}
		c->timing.*K.out = cnt[1]; c->timing.*K.windows = cnt[0] > cnt[1] ? cnt[0] - cnt[1] : 0u;
		if ( K.ms && alone ) { float sms = 0; hipEventElapsedTime(&sms,c->ev[1],S.done); c->timing.*K.ms = sms; }
		else if ( K.ms ) { float sms = 0; hipEventElapsedTime(&sms,from,S.done); c->timing.*K.ms = sms; from = S.done; }
	}
	// the long string stage (wide batches, second stream): what it read is what the second stream read (long_windows), what it handed on is what k_window_long ran
	c->timing.longstr_ms = 0; c->timing.longstr_windows = 0; c->timing.longstr_out = 0; c->timing.pad2_ = 0; c->timing.pad3_ = 0; c->timing.pad4_ = 0; c->timing.pad5_ = 0;
	if ( !(TP.usefast && BP.nwindows && TP.anytier()) ) c->longran[0] = c->longran[1] = false;
	for ( int i = 0; i < 2; ++i )
		if ( c->longran[i] )
		{
			uint32_t nout = 0; float lms = 0;
			HIPCHK(hipMemcpy(&nout,c->d_longhand[i].p,sizeof(uint32_t),hipMemcpyDeviceToHost));
			hipEventElapsedTime(&lms,c->evLong[2*i],c->evLong[2*i+1]);
			c->timing.longstr_ms += lms; c->timing.longstr_out += nout; c->timing.longstr_windows += c->nlong[i] > nout ? c->nlong[i] - nout : 0u;
		}
	return DACC_OK;
}

// 12. what the caller collects: the status of every pile and the text of what went wrong, then the fragments
static int assembleResults(dacc_ctx * c, Pass const & P)
{
	BatchPlan & BP = c->BP;
	c->pile_status = BP.pile_status; c->pile_errors = BP.pile_errors;
	if ( P.herr[0] && BP.piles.size() )
	{
		// windows the generic engine could not hold even with grown scratch: their piles were dropped by the vote
		std::vector<uint8_t> bad(BP.piles.size());
		HIPCHK(hipMemcpy(bad.data(),c->d_pilebad.p,bad.size(),hipMemcpyDeviceToHost));
		for ( size_t pi = 0; pi < bad.size(); ++pi )
			if ( bad[pi] )
			{
				c->pile_status[pi] = DACC_ENOTSUP;
				if ( c->pile_errors.size() < 64 ) c->pile_errors.push_back("read " + std::to_string(BP.piles[pi].aread) + ": window kernel scratch capacity exceeded (depth / graph size), read skipped");
			}
	}
	if ( P.herr[3] ) { c->err = "internal error: a window was handed on between engines and never processed"; return DACC_EHIP; }
	if ( P.herr[1] ) { c->err = "vote kernel capacity exceeded"; return DACC_ENOTSUP; }
	if ( P.herr[2] ) { c->err = "trace kernel capacity exceeded (a tspace block longer than the column vectors or a B span beyond the column store)"; return DACC_ENOTSUP; }
	// 13. the fragments of every pile and their bases, in pile order
	c->frags.clear(); c->bases.clear();
	uint64_t nbases = 0;
	for ( uint64_t pi = 0; pi < BP.piles.size(); ++pi )
		for ( uint32_t f = 0; f < c->h_nfrag[pi]; ++f ) nbases += c->h_frags[BP.fragbase[pi]+f].len;
	c->bases.reserve(nbases);
	for ( uint64_t pi = 0; pi < BP.piles.size(); ++pi )
		for ( uint32_t f = 0; f < c->h_nfrag[pi]; ++f )
		{
			VoteFragment const & F = c->h_frags[BP.fragbase[pi]+f];
			dacc_fragment g; g.aread = BP.piles[pi].aread; g.first = F.first; g.last = F.last; g.len = F.len; g.seq_off = c->bases.size();
			c->bases.append(reinterpret_cast<char const *>(c->h_outsym.p)+F.off,F.len);
			c->frags.push_back(g);
		}
	return DACC_OK;
}

// 14. dacc_timing's times, from the events of the pass
static void eventTimes(dacc_ctx * c)
{
	BatchPlan & BP = c->BP; TierPipeline & TP = c->TP;
	dacc_ctx::Stage * const f0 = ranOf(c,ID_T0), * const f7 = ranOf(c,ID_T7), * const fD = ranOf(c,ID_DENSE), * const fX = ranOf(c,ID_DEEP);
	float ms = 0;
	hipEventElapsedTime(&ms,c->ev[0],c->ev[1]); c->timing.trace_ms = ms;
	hipEventElapsedTime(&ms,c->ev[1],c->ev[2]); c->timing.window_ms = ms;
	for ( int i = 0; i < 3; ++i ) c->timing.tier_ms[i] = 0;
	if ( TP.usefast && !aloneBatch(c) && BP.nwindows ) for ( int i = 0; i < 3; ++i ) { hipEventElapsedTime(&ms,i ? c->evslot[i-1] : c->ev[1],c->evslot[i]); c->timing.tier_ms[i] = ms; }
	c->timing.tier0_ms = 0; c->timing.tier7_ms = 0; c->timing.pad_ = 0; c->timing.tier10_ms = 0; c->timing.tier10_ran = fD ? 1u : 0u;
	if ( f0 ) { hipEventElapsedTime(&ms,c->ev[1],f0->done); c->timing.tier0_ms = ms; }
	if ( f7 ) { hipEventElapsedTime(&ms,f0->done,f7->done); c->timing.tier7_ms = ms; }
	if ( fD ) { hipEventElapsedTime(&ms,c->evslot[1],fD->done); c->timing.tier10_ms = ms; }
	c->timing.deep_ms = 0;
	if ( fX ) { hipEventElapsedTime(&ms,fD ? fD->done : c->evslot[1],fX->done); c->timing.deep_ms = ms; }
	hipEventElapsedTime(&ms,c->ev[2],c->ev[3]); c->timing.vote_ms = ms;
	hipEventElapsedTime(&ms,c->evEmit[0],c->evEmit[1]); c->timing.emit_ms = ms;      // (of the last vote of the batch; a part of vote_ms)
	hipEventElapsedTime(&ms,c->ev[3],c->ev[4]); c->timing.d2h_ms = ms;
	hipEventElapsedTime(&ms,c->ev[0],c->ev[3]); c->timing.total_ms = ms;
	c->timing.first_tier = (TP.usefast && BP.deep) ? 4u : 1u;
	c->timing.nwindows = BP.nwindows; c->timing.nblocks = BP.nblocks; c->timing.algo_bytes = BP.algo_bytes + c->bases.size();
}

static int runDevice(dacc_ctx * c)
{
	BatchPlan & BP = c->BP; TierPipeline & TP = c->TP; hipStream_t const s = c->stream;
	Pass P; int rc;
	growHandOver(c);
	++c->nruns;
	if ( (rc = enqueuePrepAndTrace(c)) ) return rc;
	// the run state of the stages and of the second stream is this pass's alone: a pass without windows launches none of them, and the counter and time
	// fetches behind it must not see what the pass before it ran (nor read the lists it kept)
	for ( dacc_ctx::Stage & S : c->st ) { S.ran = false; S.in = 0; }
	c->nlong[0] = c->nlong[1] = 0; c->longran[0] = c->longran[1] = false;
	if ( BP.nwindows )
	{
		P.WB = windowBatch(c);
		// no LDS tier usable (DACC_TIERS=0 or a model table no tier's overlay holds): everything runs in the generic engine on
		// the main stream; the pre-scan / second stream would hand the same windows to two kernels
		if ( TP.usefast && TP.anytier() )
		{
			if ( (rc = enqueuePrescan(c,P)) ) return rc;
			for ( uint32_t slot = 0; slot < TIER_NSLOTS; ++slot ) { if ( (rc = enqueueSlot(c,P,slot)) ) return rc; hipEventRecord(c->evslot[slot],s); }
			uint32_t const * const slotlist = P.list;      // what the last enabled slot handed on (dacc_debug_retry, tier_out)
			if ( (rc = enqueueTrailingStages(c,P)) ) return rc;
			if ( c->env_dbgretry && slotlist && (rc = dumpRetryFlags(c,slotlist)) ) return rc;
			if ( (rc = enqueueGenericAndSecondStream(c,P)) ) return rc;
		}
		else
		{
			HIPCHK(hipMemsetAsync(c->d_work.p,0,WORK_WORDS*sizeof(uint32_t),s));
			uint32_t const * glist = 0;      // what the generic engine reads (0: all windows)
			if ( TP.ok[ID_W128] )
			{
				// a batch of w = 128: every window runs in the stage's tier first (layout in its own slab, no LDS, no pre-scan map and no early list: a string
				// of more than 255 bases is handed on like a table that overflowed), the generic engine runs what it hands on
				dacc_ctx::Stage & S = c->st[ID_W128];
				FastBatch FZ = stageBatch(c,P.WB,ID_W128,false); handsOn(FZ,S.handon.p,S.slab.p);
				if ( (rc = launchStage(c,ID_W128,FZ,0,"k_window_fast (w = 128 stage)")) ) return rc;
				glist = S.handon.p;
			}
			hipLaunchKernelGGL(k_window,dim3(c->win_grid),dim3(64),0,s,P.WB,c->d_err.p,glist,(c->sched&2) ? c->d_work.p+WORK_GENERIC : static_cast<uint32_t *>(0));
			mark(c,glist ? "k_window (what the w = 128 stage handed on)" : "k_window (all windows)");
		}
	}
	HIPCHK(hipEventRecord(c->ev[2],s));
	P.symbytes = 2*BP.npos + 64*BP.piles.size() + 64;
	c->h_nfrag.resize(BP.piles.size()); c->h_frags.resize(BP.nfragslots+1); HIPCHK(c->h_outsym.ensure(P.symbytes));
	if ( (rc = voteAndFetch(c,P)) ) return rc;
	if ( (rc = fetchTierCounters(c)) ) return rc;
	if ( (rc = scratchRetry(c,P)) ) return rc;
	if ( (rc = fetchStageCounters(c)) ) return rc;
	if ( (rc = assembleResults(c,P)) ) return rc;
	eventTimes(c);
	return DACC_OK;
}

// ---- the batch setup (dacc_submit_piles_body): one function per phase, in the order they run.  The device allocations and the hipFuncSetAttribute calls keep their
// order from phase to phase and inside each: it decides which allocation meets an out-of-memory first, and so which optional buffer is given up (dacc_drop_hand)

// 1. the error flags and profile counters, then the planned batch and its trace points go up; the tables the trace kernels fill
static int uploadBatch(dacc_ctx * c, void const * trace, uint64_t const ntrace, int const trace_bytes)
{
	BatchPlan & BP = c->BP; hipStream_t const s = c->stream; int rc;
	HIPCHK(c->d_err.ensure(4));
	HIPCHK(c->d_prof.ensure(DACC_PROFW*4096)); HIPCHK(hipMemsetAsync(c->d_prof.p,0,DACC_PROFW*4096*sizeof(uint64_t),s));   // one row of counters per workgroup (no contention)
	HIPCHK(hipEventRecord(c->ev[5],s));
	if ( (rc = upload(c,c->d_piles,BP.piles.data(),BP.piles.size())) ) return rc;
	if ( (rc = upload(c,c->d_ovl,BP.ovl.data(),BP.ovl.size())) ) return rc;
	if ( (rc = upload(c,c->d_ovl_pile,BP.ovl_pile.data(),BP.ovl_pile.size())) ) return rc;
	if ( (rc = upload(c,c->d_trace,static_cast<uint8_t const *>(trace),ntrace*trace_bytes)) ) return rc;
	if ( (rc = upload(c,c->d_fragbase,BP.fragbase.data(),BP.fragbase.size())) ) return rc;
	HIPCHK(c->d_blk_ovl.ensure(BP.nblocks+1)); HIPCHK(c->d_blk_b0.ensure(BP.nblocks+1));
	HIPCHK(c->d_wt_b.ensure(BP.nwt+1)); HIPCHK(c->d_wt_e.ensure(BP.nwt+1));
	c->trace_bytes = trace_bytes;
	return DACC_OK;
}

static void const * traceKernel(uint32_t const words)
{
	return words == 2 ? reinterpret_cast<void const *>(k_trace) : words == 4 ? reinterpret_cast<void const *>(k_trace_wide<4>) : reinterpret_cast<void const *>(k_trace_wide<8>);
}
// 2. the trace kernels' launch (launch_geometry.hpp: traceGeometry), the LDS attribute of a wide kernel and the two word kernel's checkpoint slabs
static int setupTrace(dacc_ctx * c)
{
	BatchPlan & BP = c->BP;
	TraceGeometry G = traceGeometry(c->par.tspace,BP.maxcols,BP.nblocks,0);
	c->tr_words = G.words; c->tr_lanes = G.lanes; c->tr_lds = G.lds;
	if ( !G.fits ) { c->err = "a trace block spans too many B bases for the trace kernel's LDS column store"; return DACC_ENOTSUP; }
	if ( G.lds > 64*1024 ) HIPCHK(hipFuncSetAttribute(traceKernel(G.words),hipFuncAttributeMaxDynamicSharedMemorySize,G.lds));
	if ( char const * e = getenv("DACC_TR_PERCU") ) G = traceGeometry(c->par.tspace,BP.maxcols,BP.nblocks,strtoull(e,0,10));      // (moves the workgroups per CU and the grid alone)
	c->tr_grid = G.grid;
	if ( G.words == 2 ) HIPCHK(c->d_trslab.ensure(static_cast<size_t>(G.grid)*traceSlabWords(BP.maxcols)));
	return DACC_OK;
}

// 3. which LDS tiers this batch runs (tier_pipeline.hpp); none: the generic engine alone
static void resolveBatchTiers(dacc_ctx * c)
{
	BatchPlan & BP = c->BP;
	c->sched = c->env_sched;
	bool fits32 = true;
	for ( size_t i = 0; i < c->H.dpsq_vst.size(); ++i ) if ( c->H.dpsq_vst[i] >> 32 ) fits32 = false; // table must fit 32 bits
	c->TP = resolveTiers(c->sw,!c->sw.nofast && fits32,BP.deep,BP.wide,c->H.nrows,c->H.nsup,c->par.w,[&](uint32_t const id) -> FastCaps & { return BP.stageCaps(id); },BP.maxstrings(c->par),TIER_NROWS);
}

// 4. the stages: launch geometry, the slots' hand-on lists and those of the front tiers (and the pre-pass's list of small windows), the global slab of the gw tiers
// (weights, spill: one per workgroup, the tiers run one after the other and share the buffer), and list and slab of every optional device-memory stage (reserveStage).
// chain: slots run, every row is visited; else the row of the stage of w = 128 alone -- a batch of w = 128 in which no slot runs (aloneBatch), behind the
// generic engine's arenas
static int reserveStages(dacc_ctx * c, bool const chain)
{
	BatchPlan & BP = c->BP; TierPipeline const & TP = c->TP; int rc;
	if ( chain ) for ( int t = 0; t < TIER_NSLOTS; ++t ) HIPCHK(c->d_retry[t].ensure(BP.nwindows+2));
	for ( uint32_t i = 0; i < TIER_NROWS; ++i )
	{
		TierStage const & R = TIER_CHAIN[i]; dacc_ctx::Stage & S = c->st[i]; FastCaps const & F = BP.stageCaps(i);
		if ( !chain && !(R.role == ROLE_ALONE && TP.ok[i]) ) continue;      // without a chain: the stage of w = 128 alone, and only where it is resolved (with one it never is)
		S.grid = F.gmem ? tierGridGmem(F.gbytes,BP.nwindows,R.slab) : tierGrid(F.ldsbytes,BP.nwindows);      // (a slab within TIER_GMEM_SLAB, or the row's own budget, TierStage::slab)
		if ( !TP.ok[i] || R.role == ROLE_LONG ) continue;
		if ( R.role == ROLE_LAST || R.role == ROLE_ALONE ) { if ( (rc = reserveStage(c,i,S.handon,S.slab,S.grid)) ) return rc; continue; }
		if ( R.role == ROLE_FRONT ) HIPCHK(S.handon.ensure(BP.nwindows+2));
		if ( R.flags & STAGE_PREPASS ) HIPCHK(c->d_small.ensure(BP.nwindows+2));
		if ( F.gbytes ) HIPCHK(c->d_gslab.ensure(static_cast<size_t>(S.grid)*F.gbytes + 256));
		if ( !F.gmem && F.ldsbytes > 64*1024 ) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(fastKernel(TP.tier[i])),hipFuncAttributeMaxDynamicSharedMemorySize,F.ldsbytes));
	}
	return DACC_OK;
}

// 5. the hand-over buffer's size (launch_geometry.hpp: handOverCapacity); DACC_HAND=0 switches the mechanism off (every hand-over restarts).
// The buffer is an optimisation for contexts that live: the driver clears device memory it hands out (16 GB = half a second on some boxes), which a single pass
// does not earn back, so the FIRST pass of a context runs without it and the buffer is allocated when the context is used again (growHandOver).
static int sizeHandOver(dacc_ctx * c)
{
	TierPipeline const & TP = c->TP;
	uint64_t const cap = handOverCapacity(c->BP.nwindows,TP.handwords,c->par.klow != c->par.khigh,c->nohand,TP.handover);
	c->handwant = cap;
	HIPCHK(c->d_handctr.ensure(4));
	if ( c->d_hand.cap < static_cast<size_t>(cap)*TP.handwords ) c->handcap = static_cast<uint32_t>(c->d_hand.cap / TP.handwords);     // what an earlier batch left
	else c->handcap = static_cast<uint32_t>(cap);
	return DACC_OK;
}

// 6. the generic engine: its grids (launch_geometry.hpp: genericGeometry) and arenas; with a chain in front of it the second stream's kernel, lists and arena as well
static int setupGenericEngine(dacc_ctx * c, bool const chain)
{
	BatchPlan & BP = c->BP; TierPipeline const & TP = c->TP;
	Arena Atmp; BP.caps.bytes = arena_carve(Atmp,0,BP.caps,c->par.w);
	GenericGeometry const G = genericGeometry(BP.nwindows,BP.caps.bytes,chain);
	c->retry_grid = G.retry_grid; c->win_grid = G.win_grid; c->early_grid = G.early_grid;
	if ( chain )
	{
		if ( TP.ok[ID_LONG] && TP.tier[ID_LONG] == 5 && BP.stageCaps(ID_LONG).ldsbytes > 64*1024 ) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_window_long),hipFuncAttributeMaxDynamicSharedMemorySize,BP.stageCaps(ID_LONG).ldsbytes));
		HIPCHK(c->d_gearly.ensure(BP.nwindows+2)); HIPCHK(c->d_pregenlist.ensure(BP.nwindows+2)); HIPCHK(c->d_pregen.ensure((BP.nwindows+31)/32+2)); HIPCHK(c->d_pregen2.ensure((BP.nwindows+31)/32+2));
		HIPCHK(c->d_arena2.ensure(static_cast<size_t>(c->early_grid)*BP.caps.bytes));
	}
	HIPCHK(c->d_work.ensure(WORK_WORDS));
	HIPCHK(c->d_arena.ensure(static_cast<size_t>(c->retry_grid)*BP.caps.bytes));
	return DACC_OK;
}

// 7. window records and results, the vote's buffers, what comes back
static int ensureResultBuffers(dacc_ctx * c)
{
	BatchPlan & BP = c->BP;
	HIPCHK(c->d_wrec.ensure((BP.nwindows+1)*static_cast<size_t>(DACC_WREC_OF(c->par.w)))); HIPCHK(c->d_wout.ensure(BP.nwindows+1));
	HIPCHK(c->d_has.ensure(BP.npos+1)); HIPCHK(c->d_oc.ensure(BP.npos+1)); HIPCHK(c->d_ld0.ensure(BP.npos+1)); HIPCHK(c->d_ocs.ensure(BP.npos+1));
	HIPCHK(c->d_outsym.ensure(2*BP.npos + 64*BP.piles.size() + 64));
	HIPCHK(c->d_nfrag.ensure(BP.piles.size()+1)); HIPCHK(c->d_frags.ensure(BP.nfragslots+1)); HIPCHK(c->d_pilebad.ensure(BP.piles.size()+1));
	return DACC_OK;
}

static int dacc_submit_piles_body(dacc_ctx * c, dacc_pile const * piles, uint64_t npiles, dacc_overlap const * ovl, uint64_t novl,
	void const * trace, uint64_t ntrace, int trace_bytes)
{
	if ( !c ) return DACC_EINVAL;
	if ( !c->haveprofile || !c->havedb ) { c->err = "dacc_set_error_profile and dacc_load_db must precede dacc_submit_piles"; return DACC_ESTATE; }
	if ( (npiles && !piles) || (novl && (!ovl || !trace)) ) return DACC_EINVAL;
	hipSetDevice(c->device);
	c->havebatch = false;
	int rc = c->BP.plan(c->par,piles,npiles,ovl,novl,trace,ntrace,trace_bytes,c->h_rlen.data(),c->h_rlen.size(),c->err,c->H.nrows,c->H.nsup);
	if ( rc ) return rc;
	if ( (rc = uploadBatch(c,trace,ntrace,trace_bytes)) ) return rc;
	if ( (rc = setupTrace(c)) ) return rc;
	resolveBatchTiers(c);
	bool const chain = c->TP.usefast && !aloneBatch(c);      // slots and a second stream run; else the generic engine alone, or behind the stage of w = 128
	if ( chain && (rc = reserveStages(c,true)) ) return rc;
	if ( chain && (rc = sizeHandOver(c)) ) return rc;
	if ( (rc = setupGenericEngine(c,chain)) ) return rc;
	if ( !chain && (rc = reserveStages(c,false)) ) return rc;
	if ( (rc = ensureResultBuffers(c)) ) return rc;
	hipEventRecord(c->h2dend,c->stream);
	rc = runDevice(c);
	float ms = 0; hipEventElapsedTime(&ms,c->ev[5],c->h2dend); c->timing.h2d_ms = ms;
	if ( rc ) return rc;
	c->havebatch = true;
	return DACC_OK;
}

static int dacc_rerun_resident_body(dacc_ctx * c)
{
	if ( !c ) return DACC_EINVAL;
	if ( !c->havebatch ) { c->err = "no resident batch"; return DACC_ESTATE; }
	hipSetDevice(c->device);
	return runDevice(c);
}

int dacc_collect(dacc_ctx * c, dacc_fragment const ** frags, uint64_t * nfrags, char const ** bases, uint64_t * nbases)
{
	if ( !c || !frags || !nfrags || !bases || !nbases ) return DACC_EINVAL;
	if ( !c->havebatch ) return DACC_ESTATE;
	*frags = c->frags.data(); *nfrags = c->frags.size(); *bases = c->bases.data(); *nbases = c->bases.size();
	return DACC_OK;
}

void dacc_release(dacc_ctx * c) { if ( c ) { c->frags.clear(); c->bases.clear(); } }

// dacc_last_timing: the record as it was when the call got its signature (everything in front of deep_ms), so that a caller compiled against
// that header is not overrun; dacc_last_timing2 copies as much of today's record as the caller says it has room for
static_assert(offsetof(dacc_timing,deep_ms) == DACC_TIMING_SIZE_V1,"dacc_last_timing fills the record in front of deep_ms");
static_assert(offsetof(dacc_timing,vdeep_ms) == 160 && offsetof(dacc_timing,longstr_ms) == DACC_TIMING_SIZE_V2 && DACC_TIMING_SIZE_V2 == 176 && offsetof(dacc_timing,fdeep_ms) == DACC_TIMING_SIZE_V3 && DACC_TIMING_SIZE_V3 == 192 && offsetof(dacc_timing,wdeep_ms) == DACC_TIMING_SIZE_V4 && DACC_TIMING_SIZE_V4 == 208 && offsetof(dacc_timing,wdeep_windows) == 212 && offsetof(dacc_timing,wdeep_out) == 216 && offsetof(dacc_timing,w128_ms) == DACC_TIMING_SIZE_V5 && DACC_TIMING_SIZE_V5 == 224 && offsetof(dacc_timing,w128_windows) == 228 && offsetof(dacc_timing,w128_out) == 232 && sizeof(dacc_timing) == 240,"the 16 bytes of the stage of w = 128 are appended behind the wide deep stage's; the very deep stage's fields are appended behind last_*, the long string stage's 16 bytes behind emit_ms, the full-depth stage's 16 bytes behind those, the wide deep stage's 16 bytes behind those");
static_assert(offsetof(dacc_timing,xdeep_ms) == 140 && offsetof(dacc_timing,xdeep_windows) == 156 && offsetof(dacc_timing,xdeep_out) == 124,"the deepest stage's fields take the pad words: the record keeps its size");
static_assert(offsetof(dacc_timing,emit_ms) == 172,"emit_ms is the last word of the first 176 bytes, where the very deep stage's pad word was");
int dacc_last_timing(dacc_ctx * c, dacc_timing * t)
{
	if ( !c || !t ) return DACC_EINVAL;
	std::memcpy(static_cast<void *>(t),&c->timing,DACC_TIMING_SIZE_V1);
	return DACC_OK;
}
int dacc_last_timing2(dacc_ctx * c, dacc_timing * t, size_t size)
{
	if ( !c || !t ) return DACC_EINVAL;
	// each stage's 16 bytes behind the first 176 go only to a caller that has room for all of them (launch_geometry.hpp: TIMING_SIZES)
	std::memcpy(static_cast<void *>(t),&c->timing,timingCopySize(size));
	return DACC_OK;
}

// per-phase cycle counters of the window kernel (all zero unless built with -DDACC_PROFILE): a row of DACC_PROFW counters per
// workgroup; 0...31 the phases (scripts/prof_phases.py), 32...127 the fine sites of round 5 (site s: cycles at 32+s, visits at 80+s)
static int dacc_debug_profile_rows(dacc_ctx * c, uint64_t * out, int const from, int const n)
{
	if ( !c || !out ) return DACC_EINVAL;
	if ( !c->havebatch ) return DACC_ESTATE;
	hipSetDevice(c->device);
	{
		std::vector<uint64_t> H(DACC_PROFW*4096);
		HIPCHK(hipMemcpy(H.data(),c->d_prof.p,DACC_PROFW*4096*sizeof(uint64_t),hipMemcpyDeviceToHost));
		for ( int i = 0; i < n; ++i ) out[i] = 0;
		for ( int b = 0; b < 4096; ++b ) for ( int i = 0; i < n; ++i ) { uint64_t const v = H[DACC_PROFW*b+from+i]; if ( from+i == 29 ) out[i] = std::max(out[i],v); else out[i] += v; }
	}
	return DACC_OK;
}
int dacc_debug_profile(dacc_ctx * c, uint64_t * out32) { return dacc_debug_profile_rows(c,out32,0,32); }
int dacc_debug_profile_fine(dacc_ctx * c, uint64_t * out96) { return dacc_debug_profile_rows(c,out96,32,96); }

// DACC_DEBUG_RETRY=1: (window, flags, mao, filterfreq) of the windows the last LDS tier handed to the generic engine
int dacc_debug_retry(dacc_ctx * c, uint32_t * out, uint64_t cap, uint64_t * n)
{
	if ( !c || !n ) return DACC_EINVAL;
	*n = c->retry_flags.size();
	if ( out ) std::memcpy(out,c->retry_flags.data(),sizeof(uint32_t)*std::min<uint64_t>(cap,c->retry_flags.size()));
	return DACC_OK;
}

// per pile status of the last batch (DACC_OK or why the pile was dropped) and the messages a caller would log
int dacc_pile_status(dacc_ctx * c, int32_t * out, uint64_t cap, uint64_t * n)
{
	if ( !c || !n ) return DACC_EINVAL;
	*n = c->pile_status.size();
	if ( out ) std::memcpy(out,c->pile_status.data(),sizeof(int32_t)*std::min<uint64_t>(cap,c->pile_status.size()));
	return DACC_OK;
}
char const * dacc_pile_errors(dacc_ctx * c)
{
	if ( !c ) return "";
	c->pile_errors_joined.clear();
	for ( size_t i = 0; i < c->pile_errors.size(); ++i ) { c->pile_errors_joined += c->pile_errors[i]; c->pile_errors_joined += '\n'; }
	return c->pile_errors_joined.c_str();
}

int dacc_debug_windows(dacc_ctx * c, dacc_window_result * out, uint64_t cap, uint64_t * nwin)
{
	if ( !c || !nwin ) return DACC_EINVAL;
	if ( !c->havebatch ) return DACC_ESTATE;
	BatchPlan & BP = c->BP;
	*nwin = BP.nwindows;
	if ( !out ) return DACC_OK;
	hipSetDevice(c->device);
	size_t const wrecb = DACC_WREC_OF(c->par.w);
	std::vector<WindowOut> wout(BP.nwindows); std::vector<uint8_t> wrec(BP.nwindows*wrecb);
	if ( BP.nwindows )
	{
		HIPCHK(hipMemcpy(wout.data(),c->d_wout.p,BP.nwindows*sizeof(WindowOut),hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(wrec.data(),c->d_wrec.p,BP.nwindows*wrecb,hipMemcpyDeviceToHost));
	}
	uint64_t i = 0;
	for ( uint64_t pi = 0; pi < BP.piles.size() && i < cap; ++pi )
		for ( uint32_t y = 0; y < BP.piles[pi].nwin && i < cap; ++y, ++i )
		{
			uint64_t const wdx = BP.piles[pi].winbase+y;
			WindowOut const & o = wout[wdx];
			dacc_window_result r; std::memset(&r,0,sizeof(r));
			r.pile = pi; r.y = y; r.status = o.status; r.mao = o.mao; r.elength = o.elength; r.k = o.k;
			r.filterfreq = (o.status == WS_OK) ? o.filterfreq : 0; r.conslen = o.conslen; r.minrate = o.minrate;
			// (a record that is not final -- a run that failed between the tiers and k_emit -- has no symbols to show)
			if ( o.status == WS_OK && wrec[wdx*wrecb] == WREC_FINAL )
			{
				// (the consensus as text, cut at 79 symbols: a debugging view)
				uint8_t const * rec = wrec.data() + wdx*wrecb;
				uint32_t const w = c->P.w; bool const wide = DACC_WIDE_W(w);
				uint8_t const * sym = wide ? rec+2+2*(w+2) : rec+1+(w+2);
				uint32_t const nsym = wide ? (rec[2+2*(w+1)] | (static_cast<uint32_t>(rec[3+2*(w+1)])<<8)) : rec[1+(w+1)];
				uint32_t cl = 0;
				for ( uint32_t q = 0; q < nsym && cl < 79; ++q ) if ( sym[q] < 4 ) r.cons[cl++] = "ACGT"[sym[q]];
			}
			out[i] = r;
		}
	return DACC_OK;
}


// guarded entry points (bodies: the *_body functions above)
int dacc_set_error_profile(dacc_ctx * c, double p_i, double p_d, double est_cor) { return guarded(c,[&]() { return dacc_set_error_profile_body(c,p_i,p_d,est_cor); }); }
int dacc_load_db(dacc_ctx * c, uint8_t const * bps, uint64_t bps_bytes, uint64_t const * boff, uint32_t const * rlen, uint64_t nreads) { return guarded(c,[&]() { return dacc_load_db_body(c,bps,bps_bytes,boff,rlen,nreads); }); }
// Measurement hook, host only (no device, no context): the planner of dacc_submit_piles (BatchPlan::plan: device records, window schedule,
// active ranges, offsets -- everything a batch needs before its first byte is uploaded) on the caller's thread + the planner's own.  With
// it the front end can time the whole host side of a run (loader + selection + plan) on a box without a GPU: `daccord_hip --loaderonly`.
int dacc_plan_only(dacc_params const * par, uint32_t const * rlen, uint64_t nreads, dacc_pile const * piles, uint64_t npiles, dacc_overlap const * ovl, uint64_t novl,
	void const * trace, uint64_t ntrace, int trace_bytes, uint64_t * nwindows, uint64_t * nblocks)
{
	if ( !par || !rlen || (!piles && npiles) ) return DACC_EINVAL;
	try
	{
		BatchPlan BP; std::string err;
		int const rc = BP.plan(*par,piles,npiles,ovl,novl,trace,ntrace,trace_bytes,rlen,nreads,err);
		if ( nwindows ) *nwindows = BP.nwindows;
		if ( nblocks ) *nblocks = BP.nblocks;
		return rc;
	}
	catch ( std::bad_alloc const & ) { return DACC_ENOMEM; }
	catch ( ... ) { return DACC_EINTERNAL; }
}

//  a device ALLOCATION failure while the optional hand-over buffer is held (up to 16 GB) may be an allocation it
// starved: give the buffer back and run the call once more without it -- the context keeps `nohand` set, so neither the planner of the
// retried call nor growHandOver's "second use" allocation brings the buffer back.  Other failures (a device fault, internal error
// flags, host allocation) are not retried: a second pass would only overwrite the first error's text.
// The same holds for the slab of a trailing stage whose row names a budget of its own (TierStage::slab: the wide deep stage's, up to 2.1 GB): it is given back
// with the hand-over buffer, the stage is off for the retried call (`noslab`) and for the rest of the context, and its windows run in k_window as before the stage.
static bool dacc_drop_hand(dacc_ctx * c)
{
	if ( !c || !c->oom ) return false;
	c->oom = false;
	bool slabs = false;
	for ( uint32_t i = 0; i < TIER_NROWS; ++i ) slabs = slabs || (ownSlab(i) && c->st[i].slab.p);
	if ( !c->d_hand.p && !slabs ) return false;
	(void)hipGetLastError(); hipSetDevice(c->device); (void)hipDeviceSynchronize(); (void)hipGetLastError();
	if ( c->d_hand.p ) { c->d_hand.release(); c->handcap = 0; c->handwant = 0; c->nohand = true; }
	if ( slabs )
	{
		for ( uint32_t i = 0; i < TIER_NROWS; ++i ) if ( ownSlab(i) ) { c->st[i].slab.release(); c->TP.ok[i] = false; }
		c->noslab = true;
	}
	return true;
}
int dacc_submit_piles(dacc_ctx * c, dacc_pile const * piles, uint64_t npiles, dacc_overlap const * ovl, uint64_t novl, void const * trace, uint64_t ntrace, int trace_bytes)
{
	if ( c ) c->oom = false;
	int rc = guarded(c,[&]() { return dacc_submit_piles_body(c,piles,npiles,ovl,novl,trace,ntrace,trace_bytes); });
	if ( rc == DACC_EHIP && dacc_drop_hand(c) ) rc = guarded(c,[&]() { return dacc_submit_piles_body(c,piles,npiles,ovl,novl,trace,ntrace,trace_bytes); });
	return rc;
}
int dacc_rerun_resident(dacc_ctx * c)
{
	if ( c ) c->oom = false;
	int rc = guarded(c,[&]() { return dacc_rerun_resident_body(c); });
	if ( rc == DACC_EHIP && dacc_drop_hand(c) ) rc = guarded(c,[&]() { return dacc_rerun_resident_body(c); });
	return rc;
}

}
