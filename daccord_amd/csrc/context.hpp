/*
 * Host side of libdaccord_hip.so: the context (dacc_ctx, include/daccord_hip.h) and what it owns on the device.
 * Every device buffer, pinned host buffer, stream and event is owned by a type that releases it: a member of such a type needs
 * no line in dacc_destroy and cannot leak on a failure path of dacc_create, and none of them can be copied.  Every scalar and
 * flag member has its initial value where it is declared: a member dacc_create does not set is defined.
 */
#ifndef DACC_CONTEXT_HPP
#define DACC_CONTEXT_HPP
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/daccord_hip.h"
#include "batch_plan.hpp"
#include "host_tables.hpp"
#include "window_main.hpp"
#include "vote_kernel.hpp"

namespace dacc {

template<typename T>
struct DevBuf
{
	T * p = 0; size_t cap = 0;
	DevBuf() = default; DevBuf(DevBuf const &) = delete; DevBuf & operator=(DevBuf const &) = delete;
	~DevBuf() { release(); }
	hipError_t ensure(size_t n)
	{
		if ( n <= cap ) return hipSuccess;
		if ( p ) { hipFree(p); p = 0; cap = 0; }
		hipError_t const e = hipMalloc(reinterpret_cast<void **>(&p),n*sizeof(T));
		if ( e == hipSuccess ) cap = n;
		return e;
	}
	void release() { if ( p ) hipFree(p); p = 0; cap = 0; }
};

// pinned host buffer (the symbol stream of a batch comes back at PCIe speed instead of through a pageable staging copy)
template<typename T>
struct HostBuf
{
	T * p = 0; size_t cap = 0; bool pinned = false;
	HostBuf() = default; HostBuf(HostBuf const &) = delete; HostBuf & operator=(HostBuf const &) = delete;
	~HostBuf() { release(); }
	// where the process may not lock that much memory (memlock limit) a pageable buffer does the same job through the runtime's staging copy
	hipError_t ensure(size_t n)
	{
		if ( n <= cap ) return hipSuccess;
		release();
		hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p),n*sizeof(T),hipHostMallocDefault);
		if ( e == hipSuccess ) { cap = n; pinned = true; return e; }
		(void)hipGetLastError();
		p = static_cast<T *>(std::malloc(n*sizeof(T)));
		if ( !p ) return hipErrorOutOfMemory;
		cap = n; pinned = false;
		return hipSuccess;
	}
	void release() { if ( p ) { if ( pinned ) hipHostFree(p); else std::free(p); } p = 0; cap = 0; pinned = false; }
};

// a stream or an event: a null handle until its owner creates it (hipStreamCreate(&x.h), hipEventCreate(&x.h), with whatever flags and
// priority the owner wants), destroyed if it is not null; reads as the plain handle
template<typename H, hipError_t (*DESTROY)(H)>
struct Handle
{
	H h = 0;
	Handle() = default; Handle(Handle const &) = delete; Handle & operator=(Handle const &) = delete;
	~Handle() { if ( h ) DESTROY(h); }
	operator H() const { return h; }
};
typedef Handle<hipStream_t,hipStreamDestroy> Stream;
typedef Handle<hipEvent_t,hipEventDestroy> Event;

struct Context
{
	dacc_params par = {};
	int device = 0;
	Stream stream, stream2;      // stream2: generic engine for the windows no LDS tier can run, concurrent with tiers 2 and 3
	Event evFirstTier, evEarlyGeneric, evPrescan;
	Event ev[6], evEmit[2], evslot[TIER_NSLOTS];      // evslot[t]: slot t of the tier chain is done
	Event h2dend;      // behind the last upload of dacc_submit_piles
	std::string err;
	bool haveprofile = false, havedb = false, havebatch = false;
	double est_cor = 0;
	HostTables H;
	DevTables T = {}; DevParams P = {};
	DevBuf<double> d_dpnorm, d_dpsq; DevBuf<uint64_t> d_vs; DevBuf<uint16_t> d_first, d_size, d_suplo, d_suphi; DevBuf<uint32_t> d_klim;
	DevBuf<uint8_t> d_bps; DevBuf<uint64_t> d_boff; DevBuf<uint32_t> d_rlen;
	std::vector<uint32_t> h_rlen;
	BatchPlan BP;
	DevBuf<DevPile> d_piles; DevBuf<DevOvl> d_ovl; DevBuf<uint32_t> d_ovl_pile; DevBuf<uint8_t> d_trace;
	DevBuf<uint32_t> d_blk_ovl, d_blk_b0, d_wt_b, d_wt_e;
	DevBuf<uint8_t> d_wrec; DevBuf<WindowOut> d_wout; DevBuf<uint8_t> d_arena;
	DevBuf<uint8_t> d_has, d_oc, d_outsym, d_pilebad; DevBuf<uint16_t> d_ld0; DevBuf<uint32_t> d_ocs, d_nfrag, d_err;
	DevBuf<VoteFragment> d_frags; DevBuf<uint64_t> d_fragbase; DevBuf<uint64_t> d_prof;
	DevBuf<uint64_t> d_vst; DevBuf<uint32_t> d_tab32; DevBuf<uint8_t> d_gslab, d_arena2; DevBuf<uint64_t> d_trslab;
	DevBuf<uint32_t> d_retry[TIER_NSLOTS], d_work, d_gearly, d_pregen, d_pregen2, d_pregenlist, d_small;
	DevBuf<uint8_t> d_longslab;         // the long string stage's (wide batches, second stream), allocated by the first pass whose second stream has a window
	DevBuf<uint32_t> d_longhand[2];     // what that stage hands on to k_window_long, one list per list of the second stream
	// the hand-over buffer (dacc_submit_piles): slots it has, slots the batch wants, passes of this context so far; nohand: given up after an allocation failure
	DevBuf<uint64_t> d_hand; DevBuf<uint32_t> d_handctr; uint32_t handcap = 0; uint64_t handwant = 0, nruns = 0; bool nohand = false, oom = false;
	bool noslab = false;      // given up after an allocation failure: the slab of a trailing stage with a budget of its own (TierStage::slab)
	bool tier7_adapt_off = false;
	// the LDS tiers (tier_pipeline.hpp): their switches, the resolved chain of the current batch (capacities: BP.stageCaps), by TierId and the launch state of its stages.
	// A main tier hands on through d_retry[slot] and is done at evslot[slot]; `handon` and `done` are those of the front tiers and of the trailing stages.
	// `slab`: a trailing stage's own slab (layout included; the kernels' grids differ), allocated by the first batch the stage is resolved for.
	TierSwitches sw = {}; TierPipeline TP = {};
	struct Stage { bool ran = false; uint32_t grid = 0; DevBuf<uint32_t> handon; DevBuf<uint8_t> slab; Event done; uint32_t const * in = 0; /* the list it read in the last pass */ } st[TIER_NROWS];
	uint32_t nlong[2] = {0,0};      // windows on the two lists of the second stream in the current pass (pre-scan, first tier's generic-only windows)
	bool longran[2] = {false,false}; Event evLong[4];      // the long string stage (tier 17): did it run over list i in the current pass, and the events around its two launches on the second stream
	// launch geometry: set by every batch (dacc_submit_piles); a generic-only batch (DACC_NOFAST, w >= 64, a model table no tier holds) reads retry_grid in its scratch retry
	uint32_t retry_grid = 0, early_grid = 0; int sched = 0;
	uint32_t tr_grid = 0, tr_lds = 0, tr_words = 0, tr_lanes = 0, trace_bytes = 0, win_grid = 0;
	int env_sched = 1, env_dbgretry = 0, env_t7adapt = 1, env_trdyn = 1;     // debugging knobs, read once in dacc_create
	uint32_t env_feasneed = 1;       // DACC_FEAS_NEED=0: stretch feasibility of every (stretch, direction, position) instead of what the enumerations can read (A/B runs, tests)
	uint32_t env_tiefast = 1;        // DACC_TIE_FAST=0: kept candidates of equal weight always take lane 0's two heaps (A/B runs, tests)
	std::vector<uint32_t> retry_flags;                      // DACC_DEBUG_RETRY: (window, flags) of what the last LDS tier handed on
	std::vector<dacc_fragment> frags; std::string bases;
	std::vector<int32_t> pile_status; std::vector<std::string> pile_errors; std::string pile_errors_joined;
	std::vector<uint32_t> h_nfrag; std::vector<VoteFragment> h_frags; HostBuf<uint8_t> h_outsym;
	dacc_timing timing = {};
};

}

struct dacc_ctx : dacc::Context {};      // the C ABI's opaque handle (include/daccord_hip.h), at global scope
#endif
