/*
 * LDS-resident fast path of the per-window de Bruijn consensus (one wavefront = one window).
 *
 * Same algorithm and exactly the same results as the generic engine (dbg_window.hpp, a close
 * restatement of the reference's control flow); what changes is where the state lives and how
 * the work is organised for CDNA4:
 *
 *  - all per-window working state sits in the workgroup's LDS slice with 8/16-bit fields; the
 *    sort buffer of the build phase is overlaid by the traversal structures;
 *  - node successors need no table: the <= 4 successor k-mers of a node are adjacent in the sorted
 *    node-key array, one lower bound per node is kept;
 *  - weights are exact 64-bit fixed point: every weight the reference forms is an integer multiple of
 *    2^-32 (w = sum of VS entries / 2^32, DotProduct.hpp:54-60) and all its partial sums stay below
 *    2^21, so the reference's FP64 sums/differences are exact and equal our integer sums times 2^-32.
 *    Thresholds become integer compares (>= 1e-3 <=> >= 4294968, > 0.1 / >= 0.1 <=> >= 429496730,
 *    >= 0.5 <=> >= 2^31), heap orders are unchanged;
 *  - k-mer feasibility is never materialised: stretch feasibility is evaluated with lanes = candidate
 *    start positions straight from a 32-bit copy of the fixed-point table held in LDS, results kept as
 *    a 64-bit position mask per stretch plus a compact weight list; stretch links are mask
 *    intersections evaluated on demand;
 *  - the reference recomputes stretches, feasibility and both path enumerations for every
 *    (first k-mer, last k-mer) candidate pair (traverse, DebruijnGraph.hpp:4774-5097; hundreds of
 *    pairs per window at k=14).  Here stretches and feasibility are computed once per activation
 *    state; the split pieces of every candidate first / last k-mer are added to the pool once;
 *    the reverse enumeration is cached per last k-mer and the forward enumeration per first k-mer,
 *    and reused for a pair whenever the other k-mer's split provably cannot touch it (no scan
 *    target of the enumeration equals a node that identifies the split stretch or its pieces);
 *    otherwise the pair is enumerated on its exact stretch set.
 *
 *  - stretches are looked up by first / last node through small index arrays, the weights of a feasible (stretch,
 *    position) entry carry the weights of its end nodes, candidates are kept as stretch sequences and decoded once.
 *
 * The same code is instantiated once per capacity tier.  The tiers -- the rows FastTier<N>, the table of their roles and the meaning of the
 * overflow flags that processWindowFast reports with FW_NEXT / FW_GENERIC -- are in fast_tiers.hpp; the layout FastLds<CT> of a tier's working
 * state, a compile time constant so that every LDS access has an immediate offset, and fastCapsOf are in fast_layout.hpp; the emulation's
 * design aids (FSTAT_*, FEAS_*) are in fast_diag.hpp.  Which tiers a batch runs, in which order and behind which switches, is written down
 * once, in tier_pipeline.hpp.  This file holds the batch record, the engine FastEngine<CT> and its entry points classifyWindow and processWindowFast.
 */
#ifndef DACC_FAST_WINDOW_HPP
#define DACC_FAST_WINDOW_HPP
#include "wave.hpp"
#include "dev_types.hpp"
#include "arena.hpp"
#include "window_main.hpp"
#include "tier_pipeline.hpp"
#include "fast_tiers.hpp"
#include "fast_layout.hpp"
#include "fast_diag.hpp"
#include "emit_record.hpp"

namespace dacc {

enum { WS_RETRY = 4 };
enum { FNOPAR = 0xFF };
enum { FSEQCAP = 48 };      // max stretches of one candidate path
// (FastCaps, the run time description of a tier, and FSUPCAP / FSUPCAPW: tier_pipeline.hpp)

struct FastBatch
{
	WindowBatch W;
	FastCaps F = {};
	uint64_t const * dpsq_vst = 0;  // [nsup][nrows] transposed fixed-point table (HBM); copied to LDS as 32-bit
	uint32_t * retry = 0;           // [0] = count, [1..] = window indices for the next capacity tier
	uint32_t * gearly = 0;          // same layout: windows no LDS tier can run (w > 63, a string > 64): straight to the generic engine
	uint8_t * gslab = 0;            // gw tiers: global scratch, gstride bytes per workgroup (weights, spill of the build-phase arrays)
	uint64_t gstride = 0;
	uint32_t const * tab32 = 0;     // gw tiers: [nsup+1][nrows+1] 32 bit copy of the fixed-point table, zero row / column at the end
	// round 4: hand-over without restart.  A window that overflows a tier's node table leaves its sorted k-mer instances and last k-mer
	// list in a slot of this buffer (handwords 64 bit words per slot: header {npre, nlast}, instances, last k-mers); the tier that picks
	// the window up loads them instead of generating and sorting them again.  hand == 0: every hand-over restarts from the strings.
	uint64_t * hand = 0; uint32_t * handctr = 0; uint32_t handcap = 0, handwords = 0;
	uint32_t feasneed = 1;          // the product default; 0: stretch feasibility of every (stretch, direction, position), as before the filter (DACC_FEAS_NEED=0: A/B runs and tests)
	uint32_t tiefast = 1;           // the product default; 0: every window with two kept candidates of one weight orders them with lane 0's two heaps, as before the lane-parallel tie rank (DACC_TIE_FAST=0: A/B runs and tests)
#if defined(DACC_LEDGER)
	uint32_t ledger = 0;            // instruction ledger build (scripts/ledger.py): bit p set = phase p of every window runs twice
#endif
};

// once per workgroup: the support bounds of the model table
template<typename CT>
DEV void fast_load_tables(FastLds<CT> const & L, uint32_t const nrows, uint32_t const nsup, DevTables const & T, uint64_t const * vst)
{
	int const lane = wv_lane();
	for ( uint32_t i = lane; i < nsup; i += WSZ ) { L.suplo8()[i] = T.suplo[i]; L.suphi8()[i] = T.suphi[i]; }
	wv_sync();
}

// Instruction ledger (round 6, VERDICT r05 task 1b).  PC sampling is refused on this pool and thread trace has no decoder, but the SQ
// counters are per kernel: a -DDACC_LEDGER build runs the phase whose bit is set in FastBatch::ledger TWICE (every phase listed is
// idempotent: it rewrites the same bytes from inputs it does not modify), so the difference of SQ_INSTS_VALU / _SALU / _LDS / ... and of
// SQ_WAVE_CYCLES between a run with the bit and a run without is that phase's own instruction count and wave time, on the product's code
// generation, at the product's occupancy, with bit-identical output.  What cannot run twice (the lane 0 replay of the pairs, which feeds
// the candidate heap) is the remainder.  The product build compiles LEDGER_REP to nothing.
#if defined(DACC_LEDGER)
#define LEDGER_REP(bit) for ( uint32_t lrep_ = 0, lrn_ = 1u + ((ledger >> (bit)) & 1u); lrep_ < lrn_; ++lrep_ )
#define LEDGER_REPX(E,bit) for ( uint32_t lrep_ = 0, lrn_ = 1u + (((E).ledger >> (bit)) & 1u); lrep_ < lrn_; ++lrep_ )
#else
#define LEDGER_REP(bit)
#define LEDGER_REPX(E,bit)
#endif
#define FW_THRES_FEAS 4294968ull        /* weight >= 1e-3 */
#define FW_THRES_01   429496730ull      /* weight > 0.1 and weight >= 0.1 (no integer lies between) */
#define FW_THRES_05   2147483648ull     /* weight >= 0.5 */

template<typename CT>
struct FastEngine
{
	typedef typename CT::id_t id_t;      // path ids inside one enumeration
	typedef typename CT::sid_t sid_t;    // stretch ids (pool ids of the stretches and pieces of a traversal)
	enum : uint32_t { SB = 8u*sizeof(sid_t), SMASK = (1u<<SB)-1u, SNONE = SMASK, SMAX = CT::smax };      // SNONE: no stretch (SNONE of the 8 bit tiers)
	FastLds<CT> L; DevTables T; DevParams P;
	uint32_t nrows, nsup;
	uint64_t const * vst;        // [nsup][nrows] fixed-point model table in HBM
	enum : bool { GW = (CT::gw != 0) };
	uint8_t * gslab;             // gw: this workgroup's global slab
	uint32_t const * gtab;       // gw: padded 32 bit table in global memory
	struct G4 { uint32_t x, y, z, w; };      // one 16 byte weight record
	int lane; uint32_t flags;
#if defined(DACC_LEDGER)
	uint32_t ledger;
#endif
	uint64_t * prof;
	uint32_t mao, k; uint64_t kmask;
	uint32_t npre, nlast, nn, nmfirst, nmlast;
	uint32_t n0, npool, nlinks, nwF, nwR;
	uint32_t nF, nL;
	uint32_t feasneed;           // FastBatch::feasneed
	uint32_t tiefast;            // FastBatch::tiefast

#if defined(DACC_EMUL)
	// emulation only: the filter's switch is read from the environment at every traversal (a test runs both settings in one process); feascount marks
	// the count-only pass of computeStretchFeasLanes that gives the traversal trace (DACC_EMUL_TRAV) its unfiltered numbers of weight records
	bool feascount, feasapplied; uint32_t nwFall, nwRall;
	DEV bool feasNeedOn() const { char const * e = getenv("DACC_FEAS_NEED"); return !(e && e[0] == '0'); }
	DEV bool tieFastOn() const { char const * e = getenv("DACC_TIE_FAST"); return !(e && e[0] == '0'); }
#else
	static constexpr bool feascount = false;
	DEV bool feasNeedOn() const { return feasneed != 0; }
	DEV bool tieFastOn() const { return tiefast != 0; }
#endif
#if defined(DACC_EMUL)
	// emulation only: DACC_EMUL_OVER=1 reports where a tier overflowed
	DEV void over_(uint32_t b, int line) { flags |= b; static char const * ov = getenv("DACC_EMUL_OVER"); if ( ov ) fprintf(stderr,"[over] tier maxs=%d line %d bits 0x%x nn=%u n0=%u npool=%u nF=%u nL=%u nwF=%u nwR=%u rstop=%u\n",int(CT::maxs)*10000+int(CT::ncap),line,b,nn,n0,npool,nF,nL,nwF,nwR,rstop); }
	#define over(b) over_(b,__LINE__)
#else
	DEV void over(uint32_t b) { flags |= b; }
#endif
#if defined(DACC_PROFILE) && !defined(DACC_EMUL)
	DEV void pcount(int id, uint64_t v) { if ( prof ) atomicAdd(reinterpret_cast<unsigned long long *>(prof+id),static_cast<unsigned long long>(v)); }
	DEV uint64_t pclock() { return clock64(); }
#else
	DEV void pcount(int, uint64_t) {}
	DEV uint64_t pclock() { return 0; }
#endif

#if defined(DACC_PROFILE) && !defined(DACC_EMUL)
	// fine sites (round 5 hot-spot ledger): shader cycles between two probes, charged once per wavefront visit (the first active
	// lane reports; inside lane-divergent code the clock is the wavefront's).  s_memtime waits for the LDS operations in flight, so a
	// site is charged with the round trips it started.
	#define SITE_T0 uint64_t _ps = clock64();
	#define SITE_RESET { _ps = clock64(); }
	#define SITE(id) { uint64_t const _n = clock64(); if ( prof && lane == static_cast<int>(__builtin_ctzll(__builtin_amdgcn_ballot_w64(true))) ) { atomicAdd(reinterpret_cast<unsigned long long *>(prof+32+(id)),static_cast<unsigned long long>(_n-_ps)); atomicAdd(reinterpret_cast<unsigned long long *>(prof+80+(id)),1ull); } _ps = clock64(); }
	#define PROFX_T0 uint64_t _px = clock64();
	#define PROFX(id) { uint64_t const _n = clock64(); if ( lane == 0 && prof ) atomicAdd(reinterpret_cast<unsigned long long *>(prof+(id)),static_cast<unsigned long long>(_n-_px)); _px = _n; }
#else
	#define PROFX_T0
	#define PROFX(id)
	#define SITE_T0
	#define SITE_RESET
	#define SITE(id)
#endif
	DEV int32_t findNode(uint32_t const v) const
	{
		int32_t lo = 0, hi = static_cast<int32_t>(nn)-1;
		while ( lo <= hi )
		{
			int32_t const mid = (lo+hi)>>1;
			uint32_t const x = L.nv()[mid];
			if ( x == v ) return mid;
			if ( x < v ) lo = mid+1; else hi = mid-1;
		}
		return -1;
	}
	DEV uint32_t lowerNode(uint32_t const v) const
	{
		uint32_t lo = 0, hi = nn;
		while ( lo < hi ) { uint32_t const mid = (lo+hi)>>1; if ( L.nv()[mid] < v ) lo = mid+1; else hi = mid; }
		return lo;
	}
	DEV int32_t succNode(uint32_t const z, uint32_t const i) const
	{
		uint32_t const sym = (L.sinfo()[z]>>(2*i))&3;
		uint32_t const target = static_cast<uint32_t>((static_cast<uint64_t>(L.nv()[z])<<2) & kmask) | sym;
		for ( uint32_t q = L.succ0()[z]; q < nn; ++q )
		{
			uint32_t const x = L.nv()[q];
			if ( x == target ) return q;
			if ( x > target ) break;
		}
		return -1;
	}
	DEV uint32_t nsucc(uint32_t z) const { return (L.sinfo()[z]>>8)&7; }
	DEV uint32_t nsuccact(uint32_t z) const { return (L.sinfo()[z]>>11)&7; }

	// ================= build: instances, nodes, successors =================
	DEV void buildInstances()
	{
		PROFX_T0
		// k-mer instances of all strings at once, lane = instance.  String j (lane j%64 of round j/64) has nk k-mers, its first
		// output slot is the exclusive prefix sum off, and among the strings with k-mers it is number rk.  (Round 5: an instance finds
		// its string in two LDS round trips -- a byte per output slot marks where a string begins, so the number of marks up to
		// slot t, counted with a ballot per 64 slots, names the string of slot t in a compact list (string, first slot).  Rounds 1-4
		// compared t against the offsets of all strings, broadcast one by one: 64 x strings scalar steps per 64 instances, 3 % of a
		// window of config 2 and a quarter of one at 54x, profiles/r05c_sites_*.log.)
		enum { NCH = (CT::maxs+WSZ-1)/WSZ };
#if defined(DACC_GEN_MARKS_NONE)
		enum : bool { GENMARKS = false };      // (A/B builds: the broadcast loop of rounds 1-4)
#else
		enum : bool { GENMARKS = true };
#endif
		// compact string list entry: string | first slot << CLB.  8 bit string ids and 24 bit slots; more than 256 strings: 10 bit ids, 16 bit slots
		// (a first slot is below npre <= 65536; the wide tier of more than 256 strings, npre <= 131072: 17 bit slots); more than 1024 strings: 11 bit ids,
		// 17 bit slots (npre <= 131072); more than 2048 strings: 13 bit ids, 18 bit slots (npre <= 262144)
		enum : bool { WIDES = FastLds<CT>::wides, XWIDES = FastLds<CT>::xwides, YWIDES = FastLds<CT>::ywides, HRANGES = FastLds<CT>::hranges };
		enum : uint32_t { CLB = YWIDES ? 13u : (XWIDES ? 11u : (WIDES ? 10u : 8u)), CLSLOTB = YWIDES ? 18u : ((XWIDES || FastLds<CT>::icap > 65536u) ? 17u : (WIDES ? 16u : 24u)), CLMASK = (1u << CLB) - 1u };
		static_assert(4u*CT::maxs <= FastLds<CT>::icap && CT::maxs <= (1u << CLB) && FastLds<CT>::icap <= (1u << CLSLOTB) && CLB + CLSLOTB <= 32u,"compact string list: string | first slot << CLB, in the bytes of irpos");
		static_assert(!WIDES || GENMARKS,"the two-pass generation of more than 256 strings needs the marks");
		LDSQ uint8_t * const marks = L.ipos();                                             // free until buildNodes writes the positions
		LDSQ uint32_t * const clist = reinterpret_cast<LDSQ uint32_t *>(L.irpos());
		// (more than 256 strings: 16 chunks would be 48 live registers -- the chunks are walked twice instead, first for the instance count, then,
		// the marks cleared, for the places; a chunk costs a length byte and two scans)
		enum { NCHR = WIDES ? 1 : NCH };
		uint32_t nkc[NCHR], offc[NCHR], rkc[NCHR]; uint32_t base = 0, nl = 0;
		if constexpr ( WIDES )
		{
			for ( uint32_t c = 0; c*WSZ < mao; ++c )
			{
				uint32_t const j = c*WSZ + lane;
				uint32_t const len = j < mao ? L.slen()[j] : 0u;
				base += wv_sum(len >= k ? (len-k+1) : 0u);
			}
		}
		else
		{
		#pragma unroll
		for ( int c = 0; c < NCH; ++c )
		{
			uint32_t const j = c*WSZ + lane;
			uint32_t const len = j < mao ? L.slen()[j] : 0u;
			nkc[c] = len >= k ? (len-k+1) : 0u;
			uint32_t tot; uint32_t const pre = wv_scan_excl(nkc[c],tot);
			offc[c] = base + pre; base += tot;
			uint32_t t2; rkc[c] = nl + wv_scan_flag(nkc[c] != 0,t2); nl += t2;
		}
		}
		npre = base;
		nlast = 0;
		if ( npre > FastLds<CT>::icap ) { over(1); npre = 0; return; }
		SITE_T0
		if constexpr ( WIDES )
		{
			for ( uint32_t i = 8*lane; i < npre; i += 8*WSZ ) *reinterpret_cast<LDSQ uint64_t *>(marks + i) = 0;
			wv_sync();
			base = 0;
			for ( uint32_t c = 0; c*WSZ < mao; ++c )
			{
				uint32_t const j = c*WSZ + lane;
				uint32_t const len = j < mao ? L.slen()[j] : 0u;
				uint32_t const nk = len >= k ? (len-k+1) : 0u;
				uint32_t tot; uint32_t const pre = wv_scan_excl(nk,tot);
				uint32_t t2; uint32_t const rk = nl + wv_scan_flag(nk != 0,t2);
				if ( nk ) { marks[base+pre] = 1; clist[rk] = j | ((base+pre) << CLB); }
				base += tot; nl += t2;
			}
			wv_sync();
		}
		else if constexpr ( GENMARKS )
		{
			for ( uint32_t i = 8*lane; i < npre; i += 8*WSZ ) *reinterpret_cast<LDSQ uint64_t *>(marks + i) = 0;      // (precap is a multiple of 8)
			wv_sync();
			#pragma unroll
			for ( int c = 0; c < NCH; ++c )
				if ( nkc[c] ) { marks[offc[c]] = 1; clist[rkc[c]] = (c*WSZ + lane) | (offc[c] << CLB); }
			wv_sync();
		}
		uint32_t cum = 0;
		for ( uint32_t t0 = 0; t0 < npre; t0 += WSZ )
		{
			uint32_t const t = t0 + lane;
			uint32_t j = 0, oj = 0, lo = 0;
			if constexpr ( GENMARKS )
			{
				bool const mk = t < npre && marks[t] != 0;
				uint32_t tot; uint32_t const before = wv_scan_flag(mk,tot);
				lo = cum + before + (mk ? 1u : 0u);      // strings with k-mers that begin at or before slot t (slot 0 begins one)
				cum += tot;
				if ( t < npre ) { uint32_t const e = clist[lo-1]; j = e & CLMASK; oj = e >> CLB; }
			}
			else
			{
				// rounds 1-4: t against the offsets of all strings, broadcast one by one (kept for A/B builds; the first measurement of
				// the marks on the shallow tiers, profiles/r05d_ab_generation.log, was 2.6 % slower only because that build also capped
				// the registers with amdgpu_waves_per_eu -- without the cap the marks are 1.9 % faster there, profiles/r05n_*)
				#pragma unroll
				for ( int c = 0; c < NCH; ++c )
					for ( uint32_t jj = 0; jj < WSZ && c*WSZ + jj < mao; ++jj )
					{
						uint32_t const o = wv_bcast(offc[c],jj), n = wv_bcast(nkc[c],jj);
						if ( t >= o ) { j = c*WSZ + jj; oj = o; lo += (n != 0); }
					}
			}
			if ( t < npre )
			{
				uint32_t const i = t - oj;
				uint32_t v = 0;
				if constexpr ( GW )
				{
					// symbols i ... i+k-1 from the pattern masks: low / high bit planes, reversed (symbol i is the most significant) and interleaved
					enum { PW = FastLds<CT>::pw };
					LDSQ uint64_t const * PEQ = L.peq() + 4*PW*j;
					uint32_t const km = (1u << k) - 1u;
					uint32_t lo, hi;
					if constexpr ( PW == 1 )
					{
						uint64_t const e1 = PEQ[1], e2 = PEQ[2], e3 = PEQ[3];
						lo = static_cast<uint32_t>((e1|e3) >> i) & km; hi = static_cast<uint32_t>((e2|e3) >> i) & km;
					}
					else if constexpr ( PW > 2 )
					{
						// (PW words per mask, tier 17: strings of up to 255 bases.  The 16 bits from position i on come from word i >> 6 and, where the run
						// straddles a boundary, from the word behind it; i + k <= 255, so a run that straddles has such a word)
						uint32_t const wq = i >> 6, sh = i & 63u;
						bool const two = sh > 48u && wq+1 < PW;
						uint64_t const l0 = PEQ[1*PW+wq] | PEQ[3*PW+wq], h0 = PEQ[2*PW+wq] | PEQ[3*PW+wq];
						uint64_t const l1 = two ? (PEQ[1*PW+wq+1] | PEQ[3*PW+wq+1]) : 0ull, h1 = two ? (PEQ[2*PW+wq+1] | PEQ[3*PW+wq+1]) : 0ull;
						uint64_t const sl = (l0 >> sh) | (sh ? (l1 << (64u-sh)) : 0ull);
						uint64_t const sx = (h0 >> sh) | (sh ? (h1 << (64u-sh)) : 0ull);
						lo = static_cast<uint32_t>(sl) & km; hi = static_cast<uint32_t>(sx) & km;
					}
					else
					{
						// (two words per mask, strings of up to 128 bases: the 16 bits from position i on may straddle the words)
						uint64_t const l0 = PEQ[1*PW] | PEQ[3*PW], l1 = PEQ[1*PW+1] | PEQ[3*PW+1], h0 = PEQ[2*PW] | PEQ[3*PW], h1 = PEQ[2*PW+1] | PEQ[3*PW+1];
						uint64_t const sl = i < 64 ? ((l0 >> i) | (i ? (l1 << (64u-i)) : 0ull)) : (l1 >> (i-64u));
						uint64_t const sh = i < 64 ? ((h0 >> i) | (i ? (h1 << (64u-i)) : 0ull)) : (h1 >> (i-64u));
						lo = static_cast<uint32_t>(sl) & km; hi = static_cast<uint32_t>(sh) & km;
					}
					v = dacc_spread16(dacc_rev32(lo) >> (32u-k)) | (dacc_spread16(dacc_rev32(hi) >> (32u-k)) << 1);
				}
				else
				{
					LDSQ uint8_t const * sp = L.str() + j*CT::lstr + i;
					#pragma unroll
					for ( uint32_t q = 0; q < 16; ++q ) { uint32_t const c = sp[q]; v = q < k ? ((v<<2) | c) : v; }
				}
				uint64_t const word = (static_cast<uint64_t>(v)<<32) | (static_cast<uint64_t>(i)<<16) | j;
				if constexpr ( WIDES ) L.pregen()[t] = word; else L.pre()[t] = word;
				if ( i + k == L.slen()[j] ) L.lastk()[lo-1] = word;
			}
		}
		nlast = nl;
		uint32_t const lp2 = next_pow2(nlast < 2 ? 2 : nlast);
		for ( uint32_t i = nlast + lane; i < lp2; i += WSZ ) L.lastk()[i] = ~0ull;
		wv_sync();
		SITE(31)      // buildInstances: generation of the k-mer instances (lane = instance)
		wv_sort_keys<FastLds<CT>::keycap>(L.lastk(),nlast);
		SITE(32)      // buildInstances: sort of the last k-mers
		if constexpr ( HRANGES )
		{
			// Up to 8 x precap instances in 64 ranges by the first three symbols of the k-mer (the six highest bits of the key; k >= 3), range r behind
			// range r-1, each sorted on its own with the sort of precap keys.  A histogram pass counts the ranges -- a counter per range in the bytes
			// of the generation's marks, which nothing reads any more, bumped by workgroup atomics --, lane 0 turns the counts into first places, and a
			// second pass takes a place per instance from the same counters: the order inside a range is whatever the atomics gave, the keys are
			// distinct and the sort settles it.  A range of more than precap keys sends the window on like a full instance array.
			// (more than 2048 strings: up to 16 x precap instances in 256 ranges by the first FOUR symbols, k >= 4 -- a k-mer of three symbols has no fourth,
			// and 5001 strings of it would exceed fqmax anyway: the window goes on)
			enum : uint32_t { NRB = YWIDES ? 8u : 6u, NR = 1u << NRB };
			if constexpr ( YWIDES ) { if ( 2u*k < NRB ) { over(1); npre = 0; nlast = 0; return; } }
			static_assert(NR*8u <= FastLds<CT>::icap && (FastLds<CT>::o_ipos & 3u) == 0,"range counters and places: two 32 bit words per range in the bytes of ipos");
			static_assert(FastLds<CT>::icap <= NR*CT::precap,"the ranges can hold every instance");
			LDSQ uint32_t * const rcnt = reinterpret_cast<LDSQ uint32_t *>(L.ipos()), * const rat = rcnt + NR;
			uint32_t const sh = 32u + 2u*k - NRB;
			for ( uint32_t r = lane; r < 2u*NR; r += WSZ ) rcnt[r] = 0;
			wv_sync();
			for ( uint32_t t = lane; t < npre; t += WSZ ) wv_atomic_add(rcnt + (static_cast<uint32_t>(L.pregen()[t] >> sh) & (NR-1u)),1u);
			wv_sync();
			uint32_t big = 0;
			if ( lane == 0 )
			{
				uint32_t o = 0;
				for ( uint32_t r = 0; r < NR; ++r ) { uint32_t const n = rcnt[r]; big |= n > CT::precap; rat[r] = o; o += n; }
			}
			if ( wv_or(big) ) { over(1); npre = 0; nlast = 0; return; }
			wv_sync();
			for ( uint32_t t = lane; t < npre; t += WSZ )
			{
				uint64_t const w = L.pregen()[t];
				L.pre()[wv_atomic_add(rat + (static_cast<uint32_t>(w >> sh) & (NR-1u)),1u)] = w;
			}
			wv_sync();
			// (rat[r] is now the end of range r)
			for ( uint32_t r = 0; r < NR; ++r )
			{
				uint32_t const n = wv_uni(rcnt[r]), e = wv_uni(rat[r]);
				if ( n > 1 ) wv_sort_keys<CT::precap>(L.pre()+(e-n),n);
			}
		}
		else if constexpr ( WIDES )
		{
			// Up to 4 x precap instances: split by the first symbol of the k-mer (the two highest bits of the key) into four ranges, range r behind
			// range r-1, and sort every range on its own with the sort of precap keys; the concatenation is the sorted array.  A range of more than
			// precap keys (a window of one symbol) sends the window on like a full instance array.
			uint32_t const sh = 32u + 2u*k - 2u;
			uint32_t cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
			for ( uint32_t t0 = 0; t0 < npre; t0 += WSZ )
			{
				uint32_t const t = t0 + lane; bool const a = t < npre;
				uint32_t const b = a ? static_cast<uint32_t>(L.pregen()[t] >> sh) & 3u : 4u;
				cnt0 += dacc_popc64(wv_ballot(b == 0)); cnt1 += dacc_popc64(wv_ballot(b == 1)); cnt2 += dacc_popc64(wv_ballot(b == 2)); cnt3 += dacc_popc64(wv_ballot(b == 3));
			}
			if ( cnt0 > CT::precap || cnt1 > CT::precap || cnt2 > CT::precap || cnt3 > CT::precap ) { over(1); npre = 0; nlast = 0; return; }
			uint32_t const o1 = cnt0, o2 = o1 + cnt1, o3 = o2 + cnt2;
			uint32_t p0 = 0, p1 = o1, p2 = o2, p3 = o3;
			uint64_t const ltm = wv_lanemask_lt();
			for ( uint32_t t0 = 0; t0 < npre; t0 += WSZ )
			{
				uint32_t const t = t0 + lane; bool const a = t < npre;
				uint64_t const w = a ? L.pregen()[t] : 0ull;
				uint32_t const b = a ? static_cast<uint32_t>(w >> sh) & 3u : 4u;
				uint64_t const m0 = wv_ballot(b == 0), m1 = wv_ballot(b == 1), m2 = wv_ballot(b == 2), m3 = wv_ballot(b == 3);
				uint64_t const mine = b == 0 ? m0 : (b == 1 ? m1 : (b == 2 ? m2 : m3));
				uint32_t const at = (b == 0 ? p0 : (b == 1 ? p1 : (b == 2 ? p2 : p3))) + dacc_popc64(mine & ltm);
				if ( a ) L.pre()[at] = w;
				p0 += dacc_popc64(m0); p1 += dacc_popc64(m1); p2 += dacc_popc64(m2); p3 += dacc_popc64(m3);
			}
			wv_sync();
			wv_sort_keys<CT::precap>(L.pre(),cnt0);
			wv_sort_keys<CT::precap>(L.pre()+o1,cnt1);
			wv_sort_keys<CT::precap>(L.pre()+o2,cnt2);
			wv_sort_keys<CT::precap>(L.pre()+o3,cnt3);
		}
		else
		wv_sort_keys<CT::precap,(CT::precap == 2048 && CT::ncap == 256)>(L.pre(),npre);      // 2048 keys in registers: the deep tier (FastTier<4>) only
		SITE(33)      // buildInstances: sort of the instances (register bitonic network)
	}

	DEV void buildNodes(uint32_t const f)
	{
		uint32_t base = 0;
		// (round 6, measured and dropped: run lengths from ballots of the head flags instead of every head walking its run: 0.45 % slower --
		// the runs are short (1.3 instances per k-mer), the extra pass over the sorted array is not, profiles/r06n)
		for ( uint32_t c = 0; c < npre; c += WSZ )
		{
			uint32_t const i = c + lane;
			uint32_t keep = 0, e = i;
			if ( i < npre && (i == 0 || (L.pre()[i]>>32) != (L.pre()[i-1]>>32)) )
			{
				uint64_t const km = L.pre()[i]>>32;
				e = i+1;
				while ( e < npre && (L.pre()[e]>>32) == km ) ++e;
				keep = (e-i) >= f;
			}
			uint32_t tot; uint32_t const pre = wv_scan_excl(keep,tot);
			if ( keep )
			{
				uint32_t const z = base+pre;
				if ( z < CT::ncap ) { L.nv()[z] = static_cast<uint32_t>(L.pre()[i]>>32); L.nps()[z] = i; L.nfreq()[z] = (e-i) > FastLds<CT>::fqmax ? FastLds<CT>::fqmax : (e-i); if ( (e-i) > FastLds<CT>::fqmax ) over(2); }
			}
			base += tot;
		}
		nn = base;
		if ( nn > CT::ncap ) { over(2); nn = 0; }
		for ( uint32_t i = lane; i < npre; i += WSZ )
		{
			uint32_t const pos = (L.pre()[i]>>16)&0xFFFF, seq = L.pre()[i]&0xFFFF;
			// positions behind the support of the model table (a string much longer than the error profile makes likely)
			// carry no weight (`pos < first+size`, getKmerPositionWeight :3826-3864): they are stored as nsup, the all-zero
			// row behind the table copy, and count as "beyond the support" in the range lookups below
			uint32_t const rpos = L.slen()[seq]-pos-k;
			L.ipos()[i] = pos < nsup ? pos : nsup; L.irpos()[i] = rpos < nsup ? rpos : nsup;
		}
		wv_sync();
		if ( lane == 0 ) L.nps()[nn] = npre;
		for ( uint32_t z = lane; z < nn; z += WSZ )
		{
			uint32_t const s0 = L.nps()[z], f2 = L.nfreq()[z];
			uint32_t const lo = L.ipos()[s0], hi = L.ipos()[s0+f2-1];
			uint32_t rlo = 255, rhi = 0;
			for ( uint32_t q = 0; q < f2; ++q ) { uint32_t const r = L.irpos()[s0+q]; rlo = r < rlo ? r : rlo; rhi = r > rhi ? r : rhi; }
			uint32_t const pf = lo < nsup ? L.suplo8()[lo] : nrows, pt = hi < nsup ? L.suphi8()[hi] : nrows;
			uint32_t const cf = rlo < nsup ? L.suplo8()[rlo] : nrows, ct = rhi < nsup ? L.suphi8()[rhi] : nrows;
			L.nrange()[z] = pf | (pt<<8) | (cf<<16) | (ct<<24);
		}
		uint32_t const kp2 = next_pow2(CT::maxs < 2 ? 2 : CT::maxs);
		base = 0;
		for ( uint32_t c = 0; c < nn; c += WSZ )
		{
			uint32_t const z = c + lane;
			uint32_t c0 = 0;
			if ( z < nn ) { uint32_t const s = L.nps()[z]; for ( uint32_t q = 0; q < L.nfreq()[z] && L.ipos()[s+q] == 0; ++q ) ++c0; }
			uint32_t tot; uint32_t const pre = wv_scan_excl(c0 ? 1 : 0,tot);
			if ( c0 && base+pre < kp2 ) L.mfirst()[base+pre] = ~((static_cast<uint64_t>(c0)<<32) | L.nv()[z]);
			base += tot;
		}
		nmfirst = base;
		if ( nmfirst > kp2 ) { over(8); nmfirst = 0; }
		uint32_t const p2 = next_pow2(nmfirst < 2 ? 2 : nmfirst);
		for ( uint32_t i = nmfirst + lane; i < p2; i += WSZ ) L.mfirst()[i] = ~0ull;
		base = 0;
		for ( uint32_t c = 0; c < nlast; c += WSZ )
		{
			uint32_t const i = c + lane;
			uint32_t const head = (i < nlast) && (i == 0 || (L.lastk()[i]>>32) != (L.lastk()[i-1]>>32));
			uint32_t tot; uint32_t const pre = wv_scan_excl(head,tot);
			if ( head )
			{
				uint32_t e = i+1;
				while ( e < nlast && (L.lastk()[e]>>32) == (L.lastk()[i]>>32) ) ++e;
				L.mlast()[base+pre] = ~((static_cast<uint64_t>(e-i)<<32) | (L.lastk()[i]>>32));
			}
			base += tot;
		}
		nmlast = base;
		uint32_t const q2 = next_pow2(nmlast < 2 ? 2 : nmlast);
		for ( uint32_t i = nmlast + lane; i < q2; i += WSZ ) L.mlast()[i] = ~0ull;
		wv_sync();
		wv_sort_keys<FastLds<CT>::keycap>(L.mfirst(),nmfirst);
		wv_sort_keys<FastLds<CT>::keycap>(L.mlast(),nmlast);
	}

	DEV void buildSuccessors(uint32_t const no)
	{
		uint32_t const lim = T.klim[(k-P.klow)*T.kln + (no < static_cast<uint32_t>(T.kln) ? no : T.kln-1)];
		for ( uint32_t z = lane; z < nn; z += WSZ )
		{
			uint32_t const masked = static_cast<uint32_t>((static_cast<uint64_t>(L.nv()[z])<<2) & kmask);
			uint32_t const s0 = lowerNode(masked);
			// up to four successors (freq<<8 | symbol), absent = 0; sorted descending by a fixed network (keys are distinct)
			uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0, n = 0;
			for ( uint32_t q = s0; q < nn && L.nv()[q] <= (masked|3); ++q )
			{
				uint32_t const kv = (static_cast<uint32_t>(L.nfreq()[q])<<8) | (L.nv()[q]&3);
				if ( n == 0 ) k0 = kv; else if ( n == 1 ) k1 = kv; else if ( n == 2 ) k2 = kv; else k3 = kv;
				++n;
			}
			#define DACC_CX(a,b) { uint32_t const hi_ = a > b ? a : b, lo_ = a > b ? b : a; a = hi_; b = lo_; }
			DACC_CX(k0,k1) DACC_CX(k2,k3) DACC_CX(k0,k2) DACC_CX(k1,k3) DACC_CX(k1,k2)
			#undef DACC_CX
			uint32_t act = 0;
			if ( n )
			{
				uint32_t const half = (k0>>8)/2;
				bool const a1 = n > 1 && ( ((k1>>8) >= half) || (P.checklim && ((k1>>8) >= lim)) );
				bool const a2 = n > 2 && ( ((k2>>8) >= half) || (P.checklim && ((k2>>8) >= lim)) );
				bool const a3 = n > 3 && ( ((k3>>8) >= half) || (P.checklim && ((k3>>8) >= lim)) );
				act = 1 + (a1 ? (1 + (a2 ? (1 + (a3 ? 1 : 0)) : 0)) : 0);
			}
			uint32_t const order = (k0&3) | ((k1&3)<<2) | ((k2&3)<<4) | ((k3&3)<<6);
			L.succ0()[z] = s0;
			L.sinfo()[z] = order | (n<<8) | (act<<11);
		}
		wv_sync();
		sfresh = true;      // S has been rebuilt (instances / nodes / successors of this pass): the next traversal spills all of it
	}
	// after buildNodes: no first k-mer candidate, or none of the last k-mer candidates (count >= 3/4 of the best, :4774-4784)
	// is a node of the filtered graph
	DEV bool passIsDead() const
	{
		if ( nmfirst == 0 || nmlast == 0 ) return true;
		uint32_t const lastthres = ((static_cast<uint32_t>((~L.mlast()[0])>>32))*3)/4;
		uint32_t any = 0;
		for ( uint32_t i = lane; i < nmlast; i += WSZ )
		{
			uint64_t const e = ~L.mlast()[i];
			if ( static_cast<uint32_t>(e>>32) >= lastthres && findNode(static_cast<uint32_t>(e)) >= 0 ) any = 1;
		}
		return !wv_any(any);
	}
	DEV bool addNextFromHeap()
	{
		uint32_t best = 0;
		for ( uint32_t z = lane; z < nn; z += WSZ )
			if ( nsuccact(z) < nsucc(z) )
			{
				uint32_t const fq = L.nfreq()[succNode(z,nsuccact(z))];
				best = fq > best ? fq : best;
			}
		best = wv_max(best);
		if ( ! best ) return false;
		for ( uint32_t z = lane; z < nn; z += WSZ )
		{
			uint32_t a = nsuccact(z); uint32_t const n = nsucc(z);
			while ( a < n && L.nfreq()[succNode(z,a)] == best ) ++a;
			L.sinfo()[z] = (L.sinfo()[z] & 0x7FF) | (a<<11);
		}
		wv_sync();
		sdirty = true;
		return true;
	}

	// ================= gap filling at filter frequency 0 (getLevelSuccessors(2), :1016-1161) =================
	// feasible position list of node z is implicit: p in [pfrom,pto) with nodeU(z,p) >= 1e-3
	DEV void levelSuccessors2()
	{
		uint32_t const s = 2;
		// (positions here are bytes: the ranges of nrange, the candidate's position under its k-mer (& 0xFF), the instance's position clamped to min(position, nsup) --
		// rows 0 ... 128 of the table of w = 128 and its read offsets fit as those of every narrower table do)
		static_assert(FastLds<CT>::maskrows <= 255u && FastLds<CT>::supcap <= 255u,"gap filling: a feasible position (a row of the model table, up to 129 at w = 128) and a clamped read offset are bytes");
		LDSQ uint64_t * REC = L.gfbuf();          // records (from<<48 | to<<32 | cv)
		uint32_t const cap = FastLds<CT>::gfcap/2;    // second half holds the (cv,pos) candidates
		LDSQ uint64_t * ANE = L.gfbuf() + cap;
		// pass 1: missing intermediate k-mers between nodes two steps apart
		uint32_t base = 0;
		for ( uint32_t c = 0; c < nn; c += WSZ )
		{
			uint32_t const i = c + lane;
			uint32_t cnt = 0; uint32_t lo = 0; uint32_t low = 0, vhigh = 0;
			if ( i < nn )
			{
				uint32_t const v = L.nv()[i];
				low = static_cast<uint32_t>((static_cast<uint64_t>(v)<<(2*s)) & kmask);
				vhigh = static_cast<uint32_t>((static_cast<uint64_t>(v)<<2) & kmask);
				lo = lowerNode(low);
				for ( uint32_t q = lo; q < nn && L.nv()[q] <= (low|0xF); ++q )
					if ( findNode((L.nv()[q]>>2)|vhigh) < 0 ) ++cnt;
			}
			uint32_t tot; uint32_t const pre = wv_scan_excl(cnt,tot);
			if ( i < nn && cnt && base+pre+cnt <= cap )
			{
				uint32_t o = base+pre;
				for ( uint32_t q = lo; q < nn && L.nv()[q] <= (low|0xF); ++q )
				{
					uint32_t const cv = (L.nv()[q]>>2)|vhigh;
					if ( findNode(cv) < 0 ) REC[o++] = (static_cast<uint64_t>(i)<<48) | (static_cast<uint64_t>(q)<<32) | cv;
				}
			}
			base += tot;
		}
		uint32_t const nrec = base;
		if ( nrec > cap ) { over(8192); return; }
		wv_sync();
		// pass 2: best common feasible position of `from` (shifted by s) and `to`
		base = 0;
		for ( uint32_t c = 0; c < nrec; c += WSZ )
		{
			uint32_t const r = c + lane;
			uint32_t have = 0; uint64_t cand = 0;
			if ( r < nrec )
			{
				uint32_t const from = REC[r]>>48, to = (REC[r]>>32)&0xFFFF; uint32_t const cv = static_cast<uint32_t>(REC[r]);
				uint64_t mweight = 0; uint32_t mp = 0;
				// common position pp: from feasible at pp-s, to feasible at pp; ascending pp, strict > keeps the first maximum
				uint32_t const rto = L.nrange()[to], rfrom = L.nrange()[from];
				for ( uint32_t pp = rto & 0xFF; pp < ((rto>>8)&0xFF); ++pp )
				{
					if ( pp < s ) continue;
					uint32_t const pf = pp-s;
					if ( pf < (rfrom&0xFF) || pf >= ((rfrom>>8)&0xFF) ) continue;
					uint64_t const ua = nodeU(from,pf,false), ub = nodeU(to,pp,false);
					if ( ua < FW_THRES_FEAS || ub < FW_THRES_FEAS ) continue;
					uint64_t const weight = ua+ub;
					if ( !have || weight > mweight ) { have = 1; mweight = weight; mp = pp - s + 1; }
				}
				cand = (static_cast<uint64_t>(cv)<<8) | mp;
			}
			uint32_t tot; uint32_t const pre = wv_scan_excl(have,tot);
			if ( have ) ANE[base+pre] = cand;
			base += tot;
		}
		uint32_t const nane = base;
		uint32_t const p2 = next_pow2(nane < 2 ? 2 : nane);
		if ( p2 > cap ) { over(8192); return; }
		for ( uint32_t i = nane + lane; i < p2; i += WSZ ) ANE[i] = ~0ull;
		wv_sync();
		wv_bitonic_sort(ANE,p2);       // (v,pos) ascending, NodeAddElement::operator<
		// pass 3: attach each candidate to the first string that is long enough and append the instance
		base = 0;
		for ( uint32_t c = 0; c < nane; c += WSZ )
		{
			uint32_t const i = c + lane;
			uint32_t ok = 0; uint32_t seqid = 0, pos = 0; uint64_t cv = 0;
			if ( i < nane )
			{
				pos = ANE[i]&0xFF; cv = ANE[i]>>8;
				for ( uint32_t j = 0; j < mao; ++j ) if ( pos + k <= L.slen()[j] ) { seqid = j; ok = 1; break; }
			}
			uint32_t tot; uint32_t const pre = wv_scan_excl(ok,tot);
			if ( ok && npre+base+pre < CT::precap ) L.pre()[npre+base+pre] = (cv<<32) | (static_cast<uint64_t>(pos)<<16) | seqid;
			base += tot;
		}
		// (the whole array is sorted again below with the sort of precap keys: a window of more than 256 strings and more than precap instances that comes
		// down to gap filling goes on to the generic engine here)
		if ( npre + base > CT::precap ) { over(1); return; }
		npre += base;
		wv_sync();
		wv_sort_keys<CT::precap>(L.pre(),npre);
	}

	// ================= stretches, once per activation state =================
	// Active predecessor counts and the walking table of the stretches, both from the successor side: node u adds one to
	// each of its active successors (LDS atomics on a scratch word array) instead of every node searching its four
	// possible predecessors; stepT[z] = the node a walk continues with from z (exactly one active successor and one active
	// predecessor), 0xFFFF where a stretch ends.  Both tables borrow the weight arrays, which are written much later.
	DEV LDSQ uint16_t * stepTable() const { return L.xstep(); }
	DEV void computePredCounts()
	{
		// (round 5: four 8 bit counters per word -- a node has at most four predecessors --, so that the scratch is 3 bytes per node
		// instead of 6 and stops being what binds the tiers' last region when their node tables grow)
		LDSQ uint32_t * const cnt32 = L.xcnt32();
		LDSQ uint16_t * const stepT = stepTable();
		for ( uint32_t z = lane; 4u*z < nn; z += WSZ ) cnt32[z] = 0;
		wv_sync();
		for ( uint32_t u = lane; u < nn; u += WSZ )
		{
			uint32_t const na = nsuccact(u);
			uint32_t first = 0xFFFF;
			for ( uint32_t i = 0; i < na; ++i ) { int32_t const v = succNode(u,i); wv_atomic_add(cnt32+(static_cast<uint32_t>(v)>>2),1u << (8u*(static_cast<uint32_t>(v)&3u))); if ( i == 0 ) first = v; }
			stepT[u] = (na == 1) ? first : 0xFFFF;
		}
		wv_sync();
		for ( uint32_t z = lane; z < nn; z += WSZ )
		{
			uint32_t const c = (cnt32[z>>2] >> (8u*(z&3u))) & 0xFFu;
			L.npred()[z] = c;
			if ( c != 1 ) stepT[z] = 0xFFFF;
		}
		wv_sync();
	}
	// out (if given) receives the first `cap` nodes
	template<typename OUTP>
	DEV uint32_t walkStretch(uint32_t const z, uint32_t const i, OUTP out, uint32_t & lastnode, uint32_t const cap = 0xFFFFFFFFu)
	{
		LDSQ uint16_t const * const stepT = stepTable();
		int32_t cur = succNode(z,i);
		uint32_t len = 2;
		if ( out ) { out[0] = z; out[1] = cur; }
		bool loop = (cur == static_cast<int32_t>(z));
		while ( !loop )
		{
			uint32_t const nx = stepT[cur];
			if ( nx == 0xFFFF ) break;
			cur = nx;
			if ( out && len < cap ) out[len] = cur;
			++len;
			if ( cur == static_cast<int32_t>(z) ) loop = true;
			if ( len > nn+1 ) { over(16); break; }
		}
		lastnode = cur;
		return len;
	}
	// (first, ext, len desc, last) packed into 56 bits: Stretch::operator< (node ids ascend with k-mer value)
	// (8 bit stretch ids: four 14 bit fields = 56 bits next to the id; 16 bit ids: four 12 bit fields = 48 bits)
	// (16 bit ids and more than 4094 nodes -- the device-memory tiers --: four 13 bit fields = 52 bits next to a 12 bit stretch number, QB)
	// (more than 2048 strings -- FastLds<CT>::ywides --: 15 bit node fields.  The base sort there orders (first, ext, stretch number), 15 + 15 + 14 bits: two
	// stretches with the same (first, ext) send the window on, so len and last never decide an order that is kept; poolKey, four fields = 60 bits, has no number)
	enum : bool { KEY2 = FastLds<CT>::ywides };
	enum : uint32_t { KF = (sizeof(sid_t) == 1 ? 14u : (KEY2 ? 15u : (CT::ncap > 4094u ? 13u : 12u))), KFMAX = (1u<<KF)-1u, QB = (KEY2 ? 14u : (KF == 13u ? 12u : static_cast<uint32_t>(SB))), QMASK = (1u<<QB)-1u };
	static_assert((KEY2 ? 2u*KF : 4u*KF) + QB <= 64u && 4u*KF <= 64u && CT::scap <= (1u<<QB) && CT::ncap <= KFMAX,"stretch sort key: its node fields and the stretch number in 64 bits");
	DEV static uint64_t sortKey(uint32_t first, uint32_t ext, uint32_t len, uint32_t last)
	{
		return (static_cast<uint64_t>(first)<<(3*KF)) | (static_cast<uint64_t>(ext)<<(2*KF)) | (static_cast<uint64_t>(KFMAX-len)<<KF) | last;
	}
	DEV uint64_t poolKey(uint32_t const s) const { uint32_t const len = L.sslen()[s]; return sortKey(L.sfirst()[s],L.links()[L.slink()[s]+1],len < KFMAX ? len : KFMAX,L.slast()[s]); }

	// raw stretches of the current activation state, sorted by Stretch::operator< (pool ids 0..n0-1)
	DEV void computeBaseStretches()
	{
		computePredCounts();
		uint32_t base = 0;
		for ( uint32_t c = 0; c < nn; c += WSZ )
		{
			uint32_t const z = c + lane;
			uint32_t cnt = 0;
			if ( z < nn ) { uint32_t const ns = nsuccact(z); if ( ns && (L.npred()[z] != 1 || ns > 1) ) cnt = ns; }
			uint32_t tot; uint32_t const pre = wv_scan_excl(cnt,tot);
			if ( base+pre+cnt <= CT::scap )
				for ( uint32_t i = 0; i < cnt; ++i ) { L.tfirst()[base+pre+i] = z; L.tlast()[base+pre+i] = i; }
			base += tot;
		}
		uint32_t const ns = base;
		if ( ns + 2 > CT::scap || ns > SMAX || nn >= KFMAX ) { over(32); n0 = 0; return; }
		wv_sync();
		// walk every stretch once: the nodes go to a scratch slot of WSLOT entries per stretch in the (not yet used) weight
		// arrays and are compacted into `links` below; a stretch without a slot or longer than it is walked a second time
		enum { WSLOT = 64 };
		// (round 6, measured and dropped: walking every stretch twice instead of sending its nodes through the slab: 0.4 % slower, profiles/r06f)
		uint32_t const nslot = FastLds<CT>::xnslot;     // legacy: the walking table sits behind the slots; gw: slots in the global slab
		for ( uint32_t q = lane; q < ns; q += WSZ )
		{
			uint32_t ln;
			uint32_t const sub = L.tlast()[q];
			if constexpr ( GW )
			{
				uint16_t * const wtmp = reinterpret_cast<uint16_t *>(gslab);
				L.tslen()[q] = walkStretch(L.tfirst()[q],sub,q < nslot ? wtmp + q*WSLOT : static_cast<uint16_t *>(0),ln,WSLOT);
			}
			else
			{
				LDSQ uint16_t * const wtmp = L.xwtmp();
				L.tslen()[q] = walkStretch(L.tfirst()[q],sub,q < nslot ? wtmp + q*WSLOT : static_cast<LDSQ uint16_t *>(0),ln,WSLOT);
			}
			L.skey()[q] = (static_cast<uint64_t>(sub)<<32) | ln;     // successor index (for a second walk) and last node
		}
		wv_sync();
		base = 0;
		for ( uint32_t c = 0; c < ns; c += WSZ )
		{
			uint32_t const q = c + lane;
			uint32_t const len = q < ns ? L.tslen()[q] : 0;
			uint32_t tot; uint32_t const pre = wv_scan_excl(len,tot);
			if ( q < ns ) L.tlink()[q] = base+pre;
			base += tot;
		}
		nlinks = base;
		if ( nlinks > CT::lcap ) { over(64); n0 = 0; return; }
		wv_sync();
		for ( uint32_t q = lane; q < ns; q += WSZ )
		{
			uint32_t const len = L.tslen()[q]; uint64_t const sk = L.skey()[q];
			LDSQ uint16_t * const dst = L.links() + L.tlink()[q];
			if ( q < nslot && len <= WSLOT )
			{
				if constexpr ( GW ) { uint16_t const * src = reinterpret_cast<uint16_t const *>(gslab) + q*WSLOT; for ( uint32_t t = 0; t < len; ++t ) dst[t] = src[t]; }
				else { LDSQ uint16_t const * src = L.xwtmp() + q*WSLOT; for ( uint32_t t = 0; t < len; ++t ) dst[t] = src[t]; }
			}
			else { uint32_t ln; walkStretch(L.tfirst()[q],static_cast<uint32_t>(sk>>32),dst,ln); }
			L.tlast()[q] = static_cast<uint32_t>(sk);
		}
		wv_sync();
		uint32_t const p2 = next_pow2(ns < 2 ? 2 : ns);
		for ( uint32_t q = lane; q < p2; q += WSZ )
		{
			if constexpr ( KEY2 ) L.skey()[q] = q < ns ? ((((static_cast<uint64_t>(L.tfirst()[q])<<KF) | L.links()[L.tlink()[q]+1])<<QB) | q) : ~0ull;
			else
			L.skey()[q] = q < ns ? ((sortKey(L.tfirst()[q],L.links()[L.tlink()[q]+1],L.tslen()[q] < KFMAX ? L.tslen()[q] : KFMAX,L.tlast()[q])<<QB) | q) : ~0ull;
		}
		wv_sync();
		wv_sort_keys<fcpow2(CT::scap)>(L.skey(),ns);
		// distinct (first,ext) by construction; a duplicate would need stretchesUnique's tie handling -> generic engine
		uint32_t dup = 0;
		for ( uint32_t q = lane; q < ns; q += WSZ )
		{
			enum : uint32_t { DUPSH = KEY2 ? QB : QB+2*KF };      // (what stands above it: first, ext)
			if ( q && (L.skey()[q]>>DUPSH) == (L.skey()[q-1]>>DUPSH) ) dup = 1;
			uint32_t const raw = L.skey()[q]&QMASK;
			L.sfirst()[q] = L.tfirst()[raw]; L.slast()[q] = L.tlast()[raw]; L.sslen()[q] = L.tslen()[raw]; L.slink()[q] = L.tlink()[raw];
		}
		if ( wv_any(dup) ) { over(32); n0 = 0; return; }
		n0 = ns;
		wv_sync();
	}
	// lookup of the base stretches by first node (base order is sorted by it) and by last node (ordered by (last, id)).  Nothing in front
	// of the reachability test of traverse() reads them, nor do the over() checks: a state without a first -> last walk never gets them.
	DEV void computeStretchLookups()
	{
		uint32_t const ns = n0, p2 = next_pow2(ns < 2 ? 2 : ns);
		LEDGER_REP(20)
		{
		for ( uint32_t z = lane; z < nn; z += WSZ ) { L.npred()[z] = SNONE; L.lhead()[z] = SNONE; }
		for ( uint32_t q = lane; q < p2; q += WSZ ) L.skey()[q] = q < ns ? ((static_cast<uint64_t>(L.slast()[q])<<SB) | q) : ~0ull;
		wv_sync();
		for ( uint32_t q = lane; q < ns; q += WSZ ) if ( q == 0 || L.sfirst()[q-1] != L.sfirst()[q] ) L.npred()[L.sfirst()[q]] = q;
		wv_sort_keys<fcpow2(CT::scap)>(L.skey(),ns);
		for ( uint32_t q = lane; q < ns; q += WSZ )
		{
			uint64_t const e = L.skey()[q];
			L.lord()[q] = static_cast<uint32_t>(e);
			if ( q == 0 || (L.skey()[q-1]>>SB) != (e>>SB) ) L.lhead()[e>>SB] = q;
		}
		wv_sync();
		}
	}

	// pool stretch id = nodes [a,b] of parent stretch par
	DEV void makePiece(uint32_t const id, uint32_t const par, uint32_t const a, uint32_t const b)
	{
		LDSQ uint16_t const * Lk = L.links() + L.slink()[par];
		L.sfirst()[id] = Lk[a]; L.slast()[id] = Lk[b]; L.sslen()[id] = b-a+1; L.slink()[id] = L.slink()[par]+a;
	}
	// candidates + the pool stretch each one splits (splitStretches :2772-2841: first occurrence strictly inside)
	DEV void findCandidatesAndPieces()
	{
		uint32_t const firstthres = nmfirst ? ((static_cast<uint32_t>((~L.mfirst()[0])>>32))*3)/4 : 0;
		uint32_t const lastthres = nmlast ? ((static_cast<uint32_t>((~L.mlast()[0])>>32))*3)/4 : 0;
		uint32_t cf = 0, cl = 0;
		while ( cf < nmfirst && static_cast<uint32_t>((~L.mfirst()[cf])>>32) >= firstthres ) ++cf;
		while ( cl < nmlast && static_cast<uint32_t>((~L.mlast()[cl])>>32) >= lastthres ) ++cl;
		nF = cf; npool = n0;
		if ( nF > FNC ) { nL = cl; over(8); return; }
		for ( uint32_t i = lane; i < nF; i += WSZ ) { uint32_t const km = static_cast<uint32_t>(~L.mfirst()[i]); L.fkmer()[i] = km; int32_t const z = findNode(km); L.fnode()[i] = z < 0 ? 0xFFFF : z; L.parF()[i] = SNONE; L.pieF()[i] = SNONE; }
		// Last k-mer candidates that are not nodes of the (filtered) graph are left out: their reverse enumeration is empty
		// (prepareTraverse starts from the node of `last`), so none of their pairs can offer a candidate, and the pairs of
		// the others keep their relative order.  In deep piles most strings end in a k-mer of their own, the list of
		// candidates with a count of at least 3/4 of a small best count is then as long as the pile is deep.
		{
			uint32_t nl = 0;
			for ( uint32_t c = 0; c < cl; c += WSZ )
			{
				uint32_t const i = c + lane;
				uint32_t const km = i < cl ? static_cast<uint32_t>(~L.mlast()[i]) : 0u;
				int32_t const z = i < cl ? findNode(km) : -1;
				uint32_t tot; uint32_t const pre = wv_scan_flag(z >= 0,tot);
				uint32_t const o = nl + pre;
				if ( z >= 0 && o < FNC ) { L.lkmer()[o] = km; L.lnode()[o] = z; L.parL()[o] = SNONE; L.pieL()[o] = SNONE; }
				nl += tot;
			}
			nL = nl;
		}
		if ( nL > FNC ) { over(8); return; }
		wv_sync();
		// parents: lanes over base stretches.  An interior node has a unique active predecessor and successor, so it
		// lies strictly inside at most one stretch; anything else goes to the generic engine
		uint32_t multi = 0;
		{
			// node -> (stretch, index) for the interior nodes, in the not yet used weight arrays: one pass over the stretches
			// (lane per stretch, indices downwards so that the first occurrence of a node stays), then one lookup per candidate
			LDSQ uint16_t * const sid = L.xsid();
			LDSQ uint8_t * const spos = L.xspos();
			for ( uint32_t z = lane; z < nn; z += WSZ ) sid[z] = 0xFFFF;
			wv_sync();
			for ( uint32_t s = lane; s < n0; s += WSZ )
			{
				uint32_t const len = L.sslen()[s]; LDSQ uint16_t const * Lk = L.links() + L.slink()[s];
				for ( uint32_t i = len > 2 ? len-2 : 0; i >= 1; --i ) { uint32_t const z = Lk[i]; sid[z] = s; spos[z] = i; }
			}
			wv_sync();
			// safety net: a node strictly inside two stretches cannot be modelled by one parent per candidate
			for ( uint32_t s = lane; s < n0; s += WSZ )
			{
				uint32_t const len = L.sslen()[s]; LDSQ uint16_t const * Lk = L.links() + L.slink()[s];
				for ( uint32_t i = 1; i+1 < len; ++i ) if ( sid[Lk[i]] != s ) multi = 1;
			}
			for ( uint32_t c = lane; c < nF; c += WSZ ) { uint32_t const z = L.fnode()[c]; if ( z != 0xFFFF && sid[z] != 0xFFFF ) { L.parF()[c] = sid[z]; L.posF()[c] = spos[z]; } }
			for ( uint32_t c = lane; c < nL; c += WSZ ) { uint32_t const z = L.lnode()[c]; if ( z != 0xFFFF && sid[z] != 0xFFFF ) { L.parL()[c] = sid[z]; L.posL()[c] = spos[z]; } }
		}
		if ( wv_any(multi) ) { over(32); return; }
		wv_sync();
		{
			uint32_t cnt = 0;
			for ( uint32_t c = 0; c < nF; ++c ) cnt += (L.parF()[c] != SNONE);
			for ( uint32_t c = 0; c < nL; ++c ) cnt += (L.parL()[c] != SNONE);
			if ( n0 + 2*cnt + 1 > CT::scap || n0 + 2*cnt + 1 > SMAX ) { over(32); return; }
			npool = n0 + 2*cnt;      // two pool ids per candidate that splits a stretch: makePieces()
		}
		// Middle pieces.  A first and a last k-mer candidate that lie strictly inside the SAME stretch at different nodes make a
		// pair whose stretch set holds three parts of that stretch (split at first, then at last: splitStretches :2772-2841 applied
		// twice); the part between the two nodes belongs to no candidate alone.  Every such pair is replayed on its exact stretch
		// set (classifyPair: 4), so the middle pieces a traversal will need are known here: they join the pool now and get their
		// feasibility with all other stretches, while the node tables are still in LDS.  (Until round 3 they were appended when
		// their pair came up, with a feasibility pass of their own that read the model table from HBM -- which the gw layout
		// cannot do, its node tables are spilled then, and whose registers cost the gw tiers their second wavefront per SIMD.)
		nmid = 0; midbase = npool;
		{
			uint64_t pm = 0;
			for ( uint32_t c = lane; c < nF; c += WSZ ) { uint32_t const par = L.parF()[c]; if ( par != SNONE ) pm |= 1ull << (par & 63u); }
			pm = wv_or64(pm);
			uint32_t hit = 0;
			for ( uint32_t c = lane; c < nL; c += WSZ ) { uint32_t const par = L.parL()[c]; if ( par != SNONE && ((pm >> (par & 63u)) & 1ull) ) hit = 1; }
			if ( wv_any(hit) )
			{
				uint32_t nm = 0;
				if ( lane == 0 )
				{
					for ( uint32_t f = 0; f < nF && nm <= MIDCAP; ++f )
					{
						uint32_t const pf = L.parF()[f];
						if ( pf == SNONE ) continue;
						for ( uint32_t l = 0; l < nL && nm <= MIDCAP; ++l )
						{
							if ( L.parL()[l] != pf ) continue;
							uint32_t const a = L.posF()[f], b = L.posL()[l];
							if ( a == b ) continue;
							uint32_t const lo = a < b ? a : b, hi = a < b ? b : a;
							uint32_t m = 0;
							while ( m < nm && !(L.midpar()[m] == pf && L.midA()[m] == lo && L.midB()[m] == hi) ) ++m;
							if ( m < nm ) continue;
							if ( nm < MIDCAP ) { L.midpar()[nm] = pf; L.midA()[nm] = lo; L.midB()[nm] = hi; }
							++nm;      // MIDCAP+1: more middle pieces than the list holds
						}
					}
				}
				wv_sync();
				nm = wv_bcast(nm,0);
				if ( nm > MIDCAP || npool + nm > CT::scap || npool + nm > SMAX ) { over(32); return; }
				nmid = nm; npool += nm;      // (their nodes: makePieces())
			}
		}
	}
	// The pieces of the pool: what findCandidatesAndPieces() counted and listed, for a state that has a first -> last walk
	// (traverse(): behind the reachability test, which reads the candidates' parents and positions only).
	DEV void makePieces()
	{
		LEDGER_REP(20)
		{
		{
			// pieces of the candidates that split a stretch, one lane per candidate (first k-mers, then last k-mers): two
			// pool ids each, numbered in candidate order
			uint32_t id = n0;
			for ( uint32_t c0 = 0; c0 < nF + nL; c0 += WSZ )
			{
				uint32_t const c = c0 + lane;
				bool const isF = c < nF, act = c < nF + nL;
				uint32_t const ci = isF ? c : c - nF;
				uint32_t const par = act ? (isF ? L.parF()[ci] : L.parL()[ci]) : static_cast<uint32_t>(SNONE);
				bool const has = act && par != SNONE;
				uint32_t tot; uint32_t const pre = wv_scan_flag(has,tot);
				if ( has )
				{
					uint32_t const pid = id + 2*pre, pos = isF ? L.posF()[ci] : L.posL()[ci];
					if ( isF ) L.pieF()[ci] = pid; else L.pieL()[ci] = pid;
					makePiece(pid,par,0,pos); makePiece(pid+1,par,pos,L.sslen()[par]-1);
				}
				id += 2*tot;
			}
		}
		wv_sync();
		for ( uint32_t m = lane; m < nmid; m += WSZ ) makePiece(midbase+m,L.midpar()[m],L.midA()[m],L.midB()[m]);      // (nmid <= MIDCAP < 64: one round on the device; the 1-lane emulation needs the loop)
		wv_sync();
		for ( uint32_t id = n0 + lane; id < npool; id += WSZ ) L.ppos()[id] = basePos(id);
		wv_sync();
		}
	}

	// Can any (first, last) candidate pair of this activation state offer a candidate at all?  A candidate is a chain of
	// view stretches from the first k-mer to the last k-mer (forward path, junction, reverse path: traverse :4838-5097), i.e.
	// a walk of at least one active edge from the node of `first` to the node of `last`.  Base stretches cover every active
	// edge that can be reached from a branch node (computeStretches :2844-2986), pieces are parts of them, so a breadth first
	// search over the base stretches from the first k-mer candidates decides it: if it reaches no last k-mer candidate,
	// traverse() has nothing to enumerate and returns false (ACCo == 0) -- feasibility, both enumerations and the pairs are
	// skipped.  The condition is necessary only (feasibility and the length bounds are not looked at): a reachable pair
	// goes through the enumerations as before.  Scratch: the weight arrays, which are written after this.
	DEV bool pairReachable()
	{
		LDSQ uint8_t * const seedN = L.xreach();
		LDSQ uint8_t * const reachN = seedN + CT::ncap;
		LDSQ uint8_t * const vis = reachN + CT::ncap;
		if ( nF == 0 || nL == 0 ) return false;
		for ( uint32_t z = lane; z < nn; z += WSZ ) { seedN[z] = 0; reachN[z] = 0; }
		for ( uint32_t s = lane; s < n0; s += WSZ ) vis[s] = 0;
		wv_sync();
		// a first k-mer at a stretch end starts the stretches that begin there; one strictly inside a stretch leads to its end
		for ( uint32_t c = lane; c < nF; c += WSZ )
		{
			uint32_t const z = L.fnode()[c], par = L.parF()[c];
			if ( z == 0xFFFF ) continue;
			if ( par == SNONE ) seedN[z] = 1; else reachN[L.slast()[par]] = 1;
		}
		wv_sync();
		while ( true )
		{
			uint32_t changed = 0;
			for ( uint32_t s = lane; s < n0; s += WSZ )
				if ( !vis[s] )
				{
					uint32_t const f = L.sfirst()[s];
					if ( seedN[f] | reachN[f] ) { vis[s] = 1; reachN[L.slast()[s]] = 1; changed = 1; }
				}
			wv_sync();
			if ( !wv_any(changed) ) break;
		}
		uint32_t ok = 0;
		for ( uint32_t c = lane; c < nL; c += WSZ )
		{
			uint32_t const z = L.lnode()[c], par = L.parL()[c];
			if ( z == 0xFFFF ) continue;
			if ( par == SNONE ) ok |= reachN[z];
			else
			{
				ok |= vis[par];      // entered through its first node
				uint32_t const pl = L.posL()[c];
				for ( uint32_t f = 0; f < nF; ++f ) if ( L.parF()[f] == par && L.posF()[f] < pl ) ok = 1;     // a first k-mer before it inside the same stretch
			}
		}
		bool const res = wv_any(ok) != 0;
		wv_sync();
		return res;
	}

	// Shortest distances, in k-mer steps, from the first k-mer candidates to every node (dF) and from every node to the last k-mer
	// candidates (dR), over the base stretches; FEASINF = none (or 255 steps and more: no path, position or start position gets there).
	// A forward path that enters a stretch at position p has walked p steps from a first candidate, so p >= dF of the stretch's
	// first node; a reverse path that enters one at p has walked p steps back from a last candidate, p >= dR of its last node.
	// The enumerations extend a path only in the first half of the window (forwardEnumerateLane, reverseEnumerateLane: (lmax+1)/2),
	// which bounds the positions they can ask computeStretchFeasLanes' records for.  Pieces are parts of base stretches: a walk over
	// them is a walk over their parents.  A candidate strictly inside a stretch leads to that stretch's end (forward) / start (reverse).
	// Same scratch as pairReachable, whose tables are dead; the two byte tables live until the unit set-up of computeStretchFeasLanes
	// has read them (nothing between the two writes there: loadTab's copy lies elsewhere).  Lost updates of lanes that relax the same
	// node in one step are made up for in the next: the loop ends when a whole pass changes nothing, at the one fixed point there is.
	enum : uint32_t { FEASINF = 255u };
	DEV void feasDistances()
	{
		LDSQ uint8_t * const dF = L.xreach();
		LDSQ uint8_t * const dR = dF + CT::ncap;
		for ( uint32_t z = lane; z < nn; z += WSZ ) { dF[z] = FEASINF; dR[z] = FEASINF; }
		wv_sync();
		for ( uint32_t c = lane; c < nF; c += WSZ ) { uint32_t const z = L.fnode()[c]; if ( z != 0xFFFF ) dF[z] = 0; }
		for ( uint32_t c = lane; c < nL; c += WSZ ) { uint32_t const z = L.lnode()[c]; if ( z != 0xFFFF ) dR[z] = 0; }
		wv_sync();
		while ( true )
		{
			uint32_t changed = 0;
			for ( uint32_t c = lane; c < nF; c += WSZ )
			{
				uint32_t const par = L.parF()[c];
				if ( L.fnode()[c] == 0xFFFF || par == SNONE ) continue;
				uint32_t const l = L.slast()[par], d = L.sslen()[par]-1u-L.posF()[c];
				if ( d < dF[l] ) { dF[l] = d; changed = 1; }
			}
			for ( uint32_t c = lane; c < nL; c += WSZ )
			{
				uint32_t const par = L.parL()[c];
				if ( L.lnode()[c] == 0xFFFF || par == SNONE ) continue;
				uint32_t const f = L.sfirst()[par], d = L.posL()[c];
				if ( d < dR[f] ) { dR[f] = d; changed = 1; }
			}
			for ( uint32_t s = lane; s < n0; s += WSZ )
			{
				uint32_t const f = L.sfirst()[s], l = L.slast()[s], step = L.sslen()[s]-1u;
				uint32_t const a = dF[f] + step, b = dR[l] + step;      // (>= FEASINF: never below a table entry)
				if ( a < dF[l] ) { dF[l] = a; changed = 1; }
				if ( b < dR[f] ) { dR[f] = b; changed = 1; }
			}
			wv_sync();
			FEAS_NEED_PASS()
			if ( !wv_any(changed) ) break;
		}
	}

	// copy of the model table in LDS, row stride nrows+1: the extra row is zero so that positions beyond the table can be
	// clamped instead of branched on; one more all-zero position (nsup) for read positions behind the support
	DEV void loadTab()
	{
		if constexpr ( GW ) return;      // gw tiers read the padded 32 bit table from global memory (L1 / L2 resident) where they need it
		else {
		uint32_t const stride = nrows+1;
		uint32_t pos = static_cast<uint32_t>(lane) / stride, row = static_cast<uint32_t>(lane) - pos*stride;     // the one division of the copy
		uint32_t const dpos = WSZ / stride, drow = WSZ - dpos*stride;
		for ( uint32_t i = lane; i < stride*(nsup+1); i += WSZ )
		{
			L.tab()[i] = (row < nrows && pos < nsup) ? static_cast<uint32_t>(vst[pos*nrows+row]) : 0u;
			pos += dpos; row += drow; if ( row >= stride ) { row -= stride; ++pos; }
		}
		wv_sync();
		}
	}
	// entry [pos][pc] of the padded table (row stride nrows+1, zero row nrows, zero position nsup)
	DEV uint32_t tabR(uint32_t const idx) const
	{
		if constexpr ( GW ) return gtab[idx];
		else return L.tab()[idx];
	}
	// ---- stretch feasibility, one LANE per (stretch, direction, start position) ----
	// The wavefront-per-stretch form above walks the stretches one after the other with lanes = start positions and leaves
	// most lanes idle (few positions survive the node supports).  Here one lane per (stretch, direction) first intersects
	// the support ranges of its nodes; the surviving (stretch, direction, position) triples are then numbered and
	// evaluated 64 at a time, a stretch after the other in each direction, so that the feasible ones can be appended to
	// the weight lists with a ballot.  Same sums in the same order as computeStretchFeas, entries in ascending start
	// position.  The loads of a node (link -> node -> first instance -> table) run ahead of the table reads.
	DEV auto unitRecords() const
	{
		if constexpr ( GW ) return L.urec();
		else { static_assert(2*CT::scap < 512,"unit ids are packed into 9 bits of a 16 bit record"); return reinterpret_cast<LDSQ uint16_t *>(L.ulo()); }
	}
	// (need: only what the enumerations of this traversal can ask for -- feasDistances() has run.  A forward unit of a base stretch starts at
	// position dF of its first node at the earliest and, like every forward unit, below H = (lmax+1)/2, the bound of the paths that are extended
	// (the roots' extensions ask for position 0 whatever H is); a reverse unit of a base stretch is read when a path of base length dR + k < H
	// reaches its last node, or as a root's extension (dR = 0), and then at ALL of its positions: linkOk takes the maximum over every
	// common position of two masks, so reverse units are kept or dropped whole.  A unit that is not needed gets width 0 and leaves the
	// order like a unit without a task; its mask stays empty.
	// Which tier finishes a window must not depend on the filter: a traversal is handed on when its weight records overflow the tier (wcap, the
	// task offsets), and that is decided by the records of ALL triples.  They are at most as many as the tasks: the set-up computes both widths
	// of every unit, and where the unfiltered tasks of a direction exceed wcap (or all of them the task offsets) the traversal runs without the
	// filter and overflows, or not, as it always did; below that bound neither form can overflow.)
	DEV void computeStretchFeasLanes(uint32_t const sfrom, uint32_t const sto, int64_t const lmax, bool const need)
	{
		PROFX_T0
		uint32_t const ns = sto-sfrom, nu = 2*ns;          // units: forward stretches, then reverse stretches
		uint32_t const stride = nrows+1;
		// (two uniform bounds, dF < max(H,1) and dR < max(H-k,1), compared in 32 bits cost the shallow tiers four more registers than this form)
		int64_t const H = (lmax+1)/2;
		int32_t const hcap = H < 1 ? 1 : (H < static_cast<int64_t>(nrows) ? static_cast<int32_t>(H) : static_cast<int32_t>(nrows));      // forward start positions: below max(H,1)
		LDSQ uint8_t const * const dF = L.xreach();
		LDSQ uint8_t const * const dR = dF + CT::ncap;
		// The tasks of a round run in lock step for as long as the longest of them walks its stretch, so the units are
		// processed in classes of decreasing stretch length (lock step iterations per traversal at config 2: 248 in pool
		// order, 97 sorted by length, about 105 in these classes; 65 is the sum of the iterations over 64).  Any order of
		// the units gives the same weights: a unit's entries stay consecutive and ascending in its own list, only the place
		// of the list in the weight arrays changes.  Position q of the order holds (lo | unit << 7) in the bytes of ulo/uhi.
		enum { NCHU = (2*CT::scap + WSZ - 1)/WSZ, NCLS = 12 };
		// task offsets: 16 bits, at most 65535 tasks per traversal; 32 bits with more than 1024 strings (FastLds<CT>::toff_t) -- a task there is one of
		// at most 2 x scap x nrows <= 2^19 triples, and the running sum below is a 32 bit word either way
		typedef typename FastLds<CT>::toff_t toff_t;
		enum : uint32_t { TOFFMAX = sizeof(toff_t) == 2 ? 0xFFFFu : 0xFFFFFFu };
		static_assert(sizeof(toff_t) == 2 || 2ull*CT::scap*128ull <= TOFFMAX,"task offsets: every (stretch, direction, position) triple can be named");
		// (legacy layout: 16 bit records over the bytes of ulo / uhi, at most 511 units; gw layout: 32 bit records)
		auto const urec = unitRecords();
		// (start position field of a unit record: 7 bits, positions up to 127; the tier of w = 128 -- rows 0 ... 128 -- takes 8, its 2 x scap units leave room in the 32 bit record)
		enum : uint32_t { ULOB = FastRows3<CT>::value ? 8u : 7u, ULOMASK = (1u << ULOB) - 1u };
		static_assert(!FastRows3<CT>::value || (GW && 2ull*CT::scap < (1ull << (32u-ULOB))),"unit records of the three-word tier: 8 bit start position under the unit number");
		// (the four words of unit cc*WSZ + lane: registers, every loop over the chunks is unrolled.  More than 2048 strings -- 384 chunks --: words of device
		// memory instead, in the bytes of the generation's instance array, which nothing reads between two builds of the instances; a lane reads back
		// only what it wrote itself)
		// (the wide tier of more than 256 strings, 4096 stretches of up to 128 start positions: device memory as well -- 128 chunks would be 512 registers)
		enum : bool { UMEM = FastLds<CT>::ywides || (FastLds<CT>::wides && CT::wide != 0) };
		struct UTab { LDSQ uint32_t * p; DEV uint32_t & operator[](uint32_t const cc) const { return p[cc*WSZ]; } };
		typedef typename FWideSel<UMEM,UTab,uint32_t[NCHU]>::type utab_t;
		utab_t ulo_r, uw_r, ucls_r, upos_r;
		if constexpr ( UMEM )
		{
			static_assert(!UMEM || 4ull*NCHU*WSZ*sizeof(uint32_t) <= 8ull*FastLds<CT>::icap,"the unit table borrows the generation's instance array");
			LDSQ uint32_t * const ut = reinterpret_cast<LDSQ uint32_t *>(L.pregen()) + lane;
			ulo_r.p = ut; uw_r.p = ut + NCHU*WSZ; ucls_r.p = ut + 2*NCHU*WSZ; upos_r.p = ut + 3*NCHU*WSZ;
		}
		// (chunks walked: all of them where they are registers, a constant the loops unroll by; the chunks that hold a unit where they are memory)
		uint32_t const nchu = UMEM ? (nu + WSZ - 1)/WSZ : static_cast<uint32_t>(NCHU);
		uint32_t allF = 0, allR = 0;          // this lane's tasks without the filter, by direction
		#pragma unroll
		for ( uint32_t cc = 0; cc < nchu; ++cc )
		{
			uint32_t const u = cc*WSZ + lane;
			uint32_t w = 0, lo_ = 0, cls = NCLS;
			if ( u < nu )
			{
				bool const rev = u >= ns; uint32_t const s = sfrom + (rev ? u-ns : u);
				uint32_t const len = L.sslen()[s]; LDSQ uint16_t const * Lk = L.links() + L.slink()[s];
				int32_t lo = 0, hi = static_cast<int32_t>(nrows);
				uint32_t const sh = rev ? 16 : 0;
				for ( uint32_t j = 0; j < len; ++j )
				{
					uint32_t const g = L.nrange()[Lk[rev ? (len-1-j) : j]] >> sh;
					int32_t const jj = static_cast<int32_t>(j);
					int32_t const a = static_cast<int32_t>(g&0xFF)-jj, b = static_cast<int32_t>((g>>8)&0xFF)-jj;
					lo = a > lo ? a : lo; hi = b < hi ? b : hi;
				}
				if ( hi < lo ) hi = lo;
				if ( need )
				{
					// (both forms of the unit in its two registers, the unfiltered one in bits 8 ...: widths and start positions are at most 128)
					w = static_cast<uint32_t>(hi-lo) << 8; lo_ = static_cast<uint32_t>(lo) << 8;
					if ( rev ) allR += static_cast<uint32_t>(hi-lo); else allF += static_cast<uint32_t>(hi-lo);
					if ( !rev ) hi = hi < hcap ? hi : hcap;
					if ( s < n0 )
					{
						int32_t const d = rev ? dR[L.slast()[s]] : dF[L.sfirst()[s]];
						bool const wanted = rev ? (d == 0 || static_cast<int64_t>(d) + static_cast<int64_t>(k) < H) : true;      // (forward: hi <= hcap decides)
						if ( !rev ) lo = d > lo ? d : lo;
						if ( d == static_cast<int32_t>(FEASINF) || !wanted ) hi = 0;
					}
					if ( hi <= lo ) { lo = 0; hi = 0; }
				}
				w |= static_cast<uint32_t>(hi-lo); lo_ |= static_cast<uint32_t>(lo);
				cls = len >= 49 ? 0u : len >= 33 ? 1u : len >= 25 ? 2u : len >= 17 ? 3u : len >= 13 ? 4u : len >= 9 ? 5u : len >= 7 ? 6u : len >= 5 ? 7u : len == 4 ? 8u : len == 3 ? 9u : len == 2 ? 10u : 11u;
				if ( !feascount )
				{
				if ( rev ) { L.maskR()[s] = 0; L.woffR()[s] = 0; } else { L.maskF()[s] = 0; L.woffF()[s] = 0; }
				if constexpr ( CT::wide != 0 ) { if ( rev ) L.maskRh()[s] = 0; else L.maskFh()[s] = 0; }
				if constexpr ( FastRows3<CT>::value != 0 ) { if ( rev ) L.maskRx()[s] = 0; else L.maskFx()[s] = 0; }
				}
			}
			ulo_r[cc] = lo_; uw_r[cc] = w; ucls_r[cc] = cls; upos_r[cc] = 0;
		}
		{
			uint32_t run = 0;
			for ( uint32_t k = 0; k < NCLS; ++k )
			{
				#pragma unroll
				for ( uint32_t cc = 0; cc < nchu; ++cc )
				{
					if ( cc*WSZ >= nu ) break;
					bool const mine = ucls_r[cc] == k;
					uint32_t tot; uint32_t const pre = wv_scan_flag(mine,tot);
					if ( mine ) upos_r[cc] = run + pre;
					run += tot;
				}
			}
		}
		// the filter stands where no direction's unfiltered tasks, hence records, can overflow the tier
		bool filt = false;
		if ( need ) { uint32_t const tF = wv_sum(allF), tR = wv_sum(allR); filt = tF <= CT::wcap && tR <= CT::wcap && static_cast<uint64_t>(tF) + tR <= TOFFMAX; }
	#if defined(DACC_EMUL)
		if ( !feascount ) feasapplied = filt;
	#endif
		#pragma unroll
		for ( uint32_t cc = 0; cc < nchu; ++cc )
		{
			uint32_t const u = cc*WSZ + lane;
			if ( u < nu )
			{
				uint32_t const usel = (need && !filt) ? 8u : 0u, umask = need ? 0xFFu : ~0u;
				uint32_t const wsel = (uw_r[cc] >> usel) & umask, lsel = (ulo_r[cc] >> usel) & umask;
				FEAS_NEED_UNIT(sfrom + (u >= ns ? u-ns : u),u >= ns,need ? (ulo_r[cc] >> 8) : lsel,need ? (ulo_r[cc] >> 8) + (uw_r[cc] >> 8) : lsel+wsel,lsel,lsel+wsel)
				urec[upos_r[cc]] = lsel | (u << ULOB); L.toff()[upos_r[cc]] = static_cast<toff_t>(wsel);
			}
		}
		wv_sync();
		FEAS_UNITS(L.toff(),nu)
		uint32_t tbase = 0;
		// widths -> first tasks, and the units without a task leave the order: position p of the compacted order (p <= q, so it is
		// written in place behind the reads of its chunk) holds the record and the first task of the p-th unit that has tasks.
		// The first tasks are strictly increasing; toff[ncu] = number of tasks ends the list.
		uint32_t ncu = 0;
		for ( uint32_t c = 0; c < nu; c += WSZ )
		{
			uint32_t const q = c + lane;
			uint32_t const w = q < nu ? L.toff()[q] : 0u;
			uint32_t const r = q < nu ? urec[q] : 0u;
			uint32_t tot; uint32_t const pre = wv_scan_excl(w,tot);
			uint32_t ntot; uint32_t const npre = wv_scan_flag(w != 0,ntot);
			if ( w != 0 ) { urec[ncu+npre] = r; L.toff()[ncu+npre] = static_cast<toff_t>(tbase + pre); }
			tbase += tot; ncu += ntot;
		}
		PROFX(18)
		if ( tbase > TOFFMAX ) { FEAS_OVER() return; }
		if ( lane == 0 ) L.toff()[ncu] = static_cast<toff_t>(tbase);
		wv_sync();
		uint32_t const ntask = tbase;
		uint64_t const ltmask = wv_lanemask_lt();
		uint32_t ubase = 0;          // wave-uniform: the unit (position in the compacted order) of the round's first task
		for ( uint32_t c = 0; c < ntask; c += WSZ )
		{
			uint32_t const t = c + lane;
			bool const act = t < ntask;
			uint32_t u = 0;
			{
				// unit of task t without a search: the tasks of a unit are consecutive, so u = ubase + the number of units that start
				// in (c,t].  Every unit has a task, so at most WSZ of them start in (c,c+WSZ]: lane i looks at unit ubase+1+i (the
				// end of the list stands in for the units behind it) and sets bit (first task - c - 1) of a mask the lanes OR together.
				uint32_t const qi = ubase + 1u + static_cast<uint32_t>(lane);
				uint32_t const d = static_cast<uint32_t>(L.toff()[qi < ncu ? qi : ncu]) - c - 1u;
				uint64_t const starts = wv_or64(d < static_cast<uint32_t>(WSZ) ? (1ull << d) : 0ull);
				u = ubase + dacc_popc64(starts & ltmask);
				ubase += dacc_popc64(starts);          // a start at c+WSZ (bit WSZ-1) is the next round's first task
			}
			uint32_t const ur = act ? urec[u] : 0u;          // u = position in the processing order
			uint32_t const uu = ur >> ULOB;
			bool const rev = uu >= ns; uint32_t const s = sfrom + (rev ? uu-ns : uu);
			uint32_t const t0 = act ? L.toff()[u] : 0u;
			uint32_t const P = act ? ((ur & ULOMASK) + (t-t0)) : 0u;
			bool ok = act;
			uint64_t sum = 0, f1 = 0, fl = 0;
			if ( act )
			{
				uint32_t const len = L.sslen()[s]; LDSQ uint16_t const * Lk = L.links() + L.slink()[s];
				LDSQ uint8_t const * IP = rev ? L.irpos() : L.ipos();
				#define DACC_LKN(J) static_cast<uint32_t>(Lk[rev ? (len-1-(J)) : (J)])
				// software pipeline over the nodes, every stage one node ahead of the next: link j+4, first instance and frequency
				// of node j+3, position byte of node j+2, table word of node j+1 -- the word of node j is in a register when its
				// iteration starts, so the test waits for a load issued a whole iteration ago.  Behind the stretch's end the
				// stages run on node 0 and on the clamp row: loads of valid indices whose values nothing reads.
				uint32_t z_d = len > 3 ? DACC_LKN(3) : 0u;
				uint32_t i0_a, f_a, i0_b, f_b, ip_b, i0_c, f_c;
				uint32_t U_a;
				{
					uint32_t const z_a = DACC_LKN(0), z_b = len > 1 ? DACC_LKN(1) : 0u, z_c = len > 2 ? DACC_LKN(2) : 0u;
					i0_a = L.nps()[z_a]; f_a = L.nfreq()[z_a]; i0_b = L.nps()[z_b]; f_b = L.nfreq()[z_b]; i0_c = L.nps()[z_c]; f_c = L.nfreq()[z_c];
					uint32_t const ip_a = IP[i0_a]; ip_b = IP[i0_b];
					U_a = tabR(ip_a*stride + (P < nrows ? P : nrows));
				}
				for ( uint32_t j = 0; j < len; ++j )
				{
					uint32_t const z_e = j+4 < len ? DACC_LKN(j+4) : 0u;
					uint32_t const i0_d = L.nps()[z_d], f_d = L.nfreq()[z_d];
					uint32_t const ip_c = IP[i0_c];
					uint32_t const pp = P+j;
					uint32_t const pc = pp < nrows ? pp : nrows, pn = pp+1 < nrows ? pp+1 : nrows;
					uint32_t const U_b = tabR(ip_b*stride + pn);
					uint64_t U = U_a;
					// (round 5) the other instances of the node four at a time: their position bytes, then their table words, are in
					// flight together -- one instance per step was two dependent round trips (LDS byte, table word in L1 / L2) each
					for ( uint32_t q = 1; q < f_a; q += 4 )
					{
						uint32_t const m = f_a - q;
						uint32_t const b0 = IP[i0_a+q], b1 = IP[i0_a+q+(m > 1 ? 1u : 0u)], b2 = IP[i0_a+q+(m > 2 ? 2u : 0u)], b3 = IP[i0_a+q+(m > 3 ? 3u : 0u)];
						uint32_t const t0 = tabR(b0*stride + pc), t1 = tabR(b1*stride + pc), t2 = tabR(b2*stride + pc), t3 = tabR(b3*stride + pc);
						U += t0; U += m > 1 ? t1 : 0u; U += m > 2 ? t2 : 0u; U += m > 3 ? t3 : 0u;
					}
					FEAS_NODE(j,len,pp,nrows,f_a)
					if ( U < FW_THRES_FEAS ) { ok = false; FEAS_ITERS(t,len,j+1) FEAS_FAIL(j,len) break; }
					sum += U;
					if ( j == 0 ) f1 = U;
					fl = U;
					i0_a = i0_b; f_a = f_b; U_a = U_b; i0_b = i0_c; f_b = f_c; ip_b = ip_c; i0_c = i0_d; f_c = f_d; z_d = z_e;
				}
				if ( ok ) { FEAS_ITERS(t,len,len) }
				#undef DACC_LKN
			}
			// append the feasible ones: forward tasks precede reverse tasks, the tasks of a stretch are consecutive
			uint64_t const okb = wv_ballot(ok);
			uint64_t const revb = wv_ballot(act && rev);
			uint64_t const mydir = rev ? revb : ~revb;
			uint32_t const base = rev ? nwR : nwF;
			if ( ok && !feascount )
			{
				uint32_t const o = base + dacc_popc64(okb & mydir & ltmask);
				if ( o < CT::wcap )
				{
					if ( rev ) putR(o,sum,f1); else putF(o,sum,f1,fl);
				}
			}
			if ( act && !feascount )
			{
				// the first lane of a stretch in this round adds the round's bits to its mask; the lane with the stretch's first
				// task sets the offset of its list
				uint32_t const firstlane = (t0 > c) ? (t0-c) : 0u;
				if ( static_cast<uint32_t>(lane) == firstlane )
				{
					uint32_t const tend = L.toff()[u+1];
					uint32_t const lastlane = (tend-c < WSZ) ? (tend-c) : static_cast<uint32_t>(WSZ);     // exclusive
					uint64_t const span = (lastlane-firstlane >= 64) ? ~0ull : ((1ull << (lastlane-firstlane))-1ull);
					if constexpr ( FastRows3<CT>::value != 0 )
					{
						// start positions up to 191: the round's bits (at most 64, from position P on) lie in word P/64 and, shifted out of it, in the next one.
						// All three words in unconditional selects: which word a bit goes to is data, not control flow
						uint64_t const seg = (okb >> firstlane) & span;
						uint32_t const wd = P >> 6, sh = P & 63u;
						uint64_t const lo_ = seg << sh, hi_ = sh ? (seg >> (64u-sh)) : 0ull;
						uint64_t const b0 = wd == 0 ? lo_ : 0ull, b1 = wd == 1 ? lo_ : (wd == 0 ? hi_ : 0ull), b2 = wd == 2 ? lo_ : (wd == 1 ? hi_ : 0ull);
						if ( rev ) { L.maskR()[s] |= b0; L.maskRh()[s] |= b1; L.maskRx()[s] |= b2; } else { L.maskF()[s] |= b0; L.maskFh()[s] |= b1; L.maskFx()[s] |= b2; }
					}
					else if constexpr ( CT::wide != 0 )
					{
						// start positions up to 127: the round's bits (at most 64, from position P on) may straddle the two words
						uint64_t const seg = (okb >> firstlane) & span;
						uint64_t const blo = P < 64u ? (seg << P) : 0ull, bhi = P < 64u ? (P ? (seg >> (64u-P)) : 0ull) : (seg << (P-64u));
						if ( rev ) { L.maskR()[s] |= blo; L.maskRh()[s] |= bhi; } else { L.maskF()[s] |= blo; L.maskFh()[s] |= bhi; }
					}
					else
					{
					uint64_t const bits = ((okb >> firstlane) & span) << P;
					if ( rev ) L.maskR()[s] |= bits; else L.maskF()[s] |= bits;
					}
					if ( t == t0 ) { uint32_t const wo = base + dacc_popc64(okb & mydir & ltmask); if ( rev ) L.woffR()[s] = wo; else L.woffF()[s] = wo; }
				}
			}
			nwF += dacc_popc64(okb & ~revb); nwR += dacc_popc64(okb & revb);
			if ( nwF > CT::wcap || nwR > CT::wcap ) { FEAS_OVER() FEAS_DUMP() return; }
		}
		FEAS_DUMP()
		wv_sync();
		FEAS_CASES_DUMP()
		FEAS_NEED_DUMP()
	}
	// weights of feasible (stretch, position) entry i.  A node weight is a sum of at most fqmax table words of < 2^32: 255 of them stay below 2^40
	// (8 bit high part), 1023 below 2^42 (10 bits, the tier of more than 256 strings); a feasible stretch has at most nrows <= 64 nodes: < 2^46 / 2^48
	// (16 bit high part either way).  Everything summed from these -- link weights, path weights rc_w / f_w, score intervals, candidates -- is a 64 bit
	// word: a path has at most FSEQCAP stretches (< 2^54).
	// (more than 1024 strings, fqmax = 4095: node weight < 2^44, 12 bit high part; stretch weight < 2^50, 18 bit high part -- SWHB; the forward record
	// of that tier holds whole 64 bit words, the reverse record's third word 18 + 12 bits)
	// (the nodes of a feasible stretch: one per row of the model table the tier admits -- nrows <= 128 in a wide tier, 64 otherwise (resolveTiers).  A wide tier of
	// more than 256 strings, fqmax = 1023 at 128 nodes: stretch weight < 2^49, 17 bit high part, the reverse record's third word 17 + 10 bits; the wide tiers of
	// up to 250 strings, fqmax = 255 at 128 nodes, stay below 2^47 and keep their 16 bits; so does the tier of w = 128, 129 nodes of at most 255: SROWS = 192 there, 192 x 255 < 2^16)
	enum : uint32_t { FQMAX = FastLds<CT>::fqmax, NWHB = FQMAX <= 255u ? 8u : (FQMAX <= 1023u ? 10u : 12u), NWHMASK = (1u << NWHB) - 1u,
		SROWS = FastLds<CT>::maskrows,
		SWHB = FQMAX <= 1023u ? ((SROWS*FQMAX) >> 16 ? 17u : 16u) : 18u, SWHMASK = (1u << SWHB) - 1u };
	static_assert((static_cast<uint64_t>(FQMAX)*0xFFFFFFFFull) >> (32u+NWHB) == 0,"high part of a node weight: fqmax table words");
	static_assert((static_cast<uint64_t>(SROWS)*static_cast<uint64_t>(FQMAX)*0xFFFFFFFFull) >> (32u+SWHB) == 0,"high part of a stretch weight: SROWS nodes of fqmax table words each, SROWS = the rows of the model table the tier's position masks name: 64, 128 in a wide tier, 192 in the tier of w = 128 (whose table has 129: 129 x 255 table words < 2^47, and 192 x 255 still < 2^48, the 16 bit high part)");
	static_assert(!FastLds<CT>::xwides || CT::wide == 0,"more than 1024 strings in a wide tier: 128 x 4095 table words need a 19 bit high part");
	static_assert(SWHB + NWHB <= 32u,"reverse record: both high parts in its third word");
	static_assert(SWHB == 16u || FastLds<CT>::wides,"a stretch weight of more than 48 bits needs the 32 byte forward record");
	static_assert(CT::maxs <= 1024 || (FastLds<CT>::fqmax == 4095u && FastLds<CT>::icap == (FastLds<CT>::ywides ? 16u : 8u)*CT::precap && FastLds<CT>::xwides),"more than 1024 strings: the widths of FastLds<CT>::xwides");
	static_assert(CT::maxs <= 2048 || (FastLds<CT>::ywides && CT::ncap <= 0xFFFEu && CT::scap <= 0xFFFEu && CT::lcap <= 0xFFFFu && CT::smax <= CT::scap),"more than 2048 strings: node ids, stretch ids and link offsets (links, tlink, slink) are 16 bit words, 0xFFFF is none");
	static_assert(FastLds<CT>::wides || 16u + 2u*NWHB <= 32u,"forward record: three high parts in its fourth word, or the 32 byte record");
	struct G8 { G4 a, b; };      // the 32 byte forward record of more than 256 strings: w, w1 | wl, unused (two 16 byte loads)
	// One record per feasible (stretch, position) entry.  Forward: whole stretch (w), its first node at the start position
	// (w1), its last node at the end position (wl); reverse: whole stretch and its last node (= first in reverse direction).
	// gw tiers: 16 byte records in the workgroup's global slab (one load per lookup); legacy tiers: split LDS arrays.
	struct WF { uint64_t w, w1, wl; };
	struct WR { uint64_t w, w1; };
	DEV WF recF(uint32_t const i) const
	{
		WF r;
		if constexpr ( GW && FastLds<CT>::wides )
		{
			G8 const v = reinterpret_cast<G8 const *>(gslab + FastLds<CT>::g_wF)[i];
			r.w = v.a.x | (static_cast<uint64_t>(v.a.y)<<32); r.w1 = v.a.z | (static_cast<uint64_t>(v.a.w)<<32); r.wl = v.b.x | (static_cast<uint64_t>(v.b.y)<<32);
		}
		else if constexpr ( GW )
		{
			G4 const v = reinterpret_cast<G4 const *>(gslab + FastLds<CT>::g_wF)[i];
			r.w = v.x | (static_cast<uint64_t>(v.w & 0xFFFFu)<<32); r.w1 = v.y | (static_cast<uint64_t>((v.w>>16)&0xFFu)<<32); r.wl = v.z | (static_cast<uint64_t>(v.w>>24)<<32);
		}
		else
		{
			r.w = L.wF_lo()[i] | (static_cast<uint64_t>(L.wF_hi()[i])<<32);
			r.w1 = L.wF1_lo()[i] | (static_cast<uint64_t>(L.wF1_hi()[i])<<32);
			r.wl = L.wFl_lo()[i] | (static_cast<uint64_t>(L.wFl_hi()[i])<<32);
		}
		return r;
	}
	DEV WR recR(uint32_t const i) const
	{
		WR r;
		if constexpr ( GW )
		{
			G4 const v = reinterpret_cast<G4 const *>(gslab + FastLds<CT>::g_wR)[i];
			r.w = v.x | (static_cast<uint64_t>(v.z & SWHMASK)<<32); r.w1 = v.y | (static_cast<uint64_t>((v.z>>SWHB)&NWHMASK)<<32);
		}
		else
		{
			r.w = L.wR_lo()[i] | (static_cast<uint64_t>(L.wR_hi()[i])<<32);
			r.w1 = L.wR1_lo()[i] | (static_cast<uint64_t>(L.wR1_hi()[i])<<32);
		}
		return r;
	}
	DEV void putF(uint32_t const o, uint64_t const sum, uint64_t const f1, uint64_t const fl) const
	{
		if constexpr ( GW && FastLds<CT>::wides )
		{
			G8 v; v.a.x = static_cast<uint32_t>(sum); v.a.y = static_cast<uint32_t>(sum>>32); v.a.z = static_cast<uint32_t>(f1); v.a.w = static_cast<uint32_t>(f1>>32);
			v.b.x = static_cast<uint32_t>(fl); v.b.y = static_cast<uint32_t>(fl>>32); v.b.z = 0; v.b.w = 0;
			reinterpret_cast<G8 *>(gslab + FastLds<CT>::g_wF)[o] = v;
		}
		else if constexpr ( GW )
		{
			G4 v; v.x = static_cast<uint32_t>(sum); v.y = static_cast<uint32_t>(f1); v.z = static_cast<uint32_t>(fl);
			v.w = (static_cast<uint32_t>(sum>>32)&0xFFFFu) | ((static_cast<uint32_t>(f1>>32)&0xFFu)<<16) | ((static_cast<uint32_t>(fl>>32)&0xFFu)<<24);
			reinterpret_cast<G4 *>(gslab + FastLds<CT>::g_wF)[o] = v;
		}
		else
		{
			L.wF_lo()[o] = static_cast<uint32_t>(sum); L.wF_hi()[o] = static_cast<uint16_t>(sum>>32);
			L.wF1_lo()[o] = static_cast<uint32_t>(f1); L.wF1_hi()[o] = static_cast<uint8_t>(f1>>32);
			L.wFl_lo()[o] = static_cast<uint32_t>(fl); L.wFl_hi()[o] = static_cast<uint8_t>(fl>>32);
		}
	}
	DEV void putR(uint32_t const o, uint64_t const rsum, uint64_t const r1) const
	{
		if constexpr ( GW )
		{
			G4 v; v.x = static_cast<uint32_t>(rsum); v.y = static_cast<uint32_t>(r1);
			v.z = (static_cast<uint32_t>(rsum>>32)&SWHMASK) | ((static_cast<uint32_t>(r1>>32)&NWHMASK)<<SWHB); v.w = 0;
			reinterpret_cast<G4 *>(gslab + FastLds<CT>::g_wR)[o] = v;
		}
		else
		{
			L.wR_lo()[o] = static_cast<uint32_t>(rsum); L.wR_hi()[o] = static_cast<uint16_t>(rsum>>32);
			L.wR1_lo()[o] = static_cast<uint32_t>(r1); L.wR1_hi()[o] = static_cast<uint8_t>(r1>>32);
		}
	}
	DEV uint64_t wuF(uint32_t const i) const { return recF(i).w; }
	DEV uint64_t wuR(uint32_t const i) const { return recR(i).w; }
	// fixed-point weight of a single node at (reverse) position p
	DEV uint64_t nodeU(uint32_t const z, uint32_t const p, bool const rev) const
	{
		if ( p >= nrows ) return 0;
		uint32_t const i0 = L.nps()[z], f = L.nfreq()[z];
		LDSQ uint8_t const * IP = rev ? L.irpos() : L.ipos();
		uint64_t u = 0;
		for ( uint32_t q = 0; q < f; ++q ) u += tabR(static_cast<uint32_t>(IP[i0+q])*(nrows+1) + p);
		return u;
	}
	// (wide tier) is position p set in the two-word mask (m0: positions 0-63, m1: 64-127), and how many positions below it are
	DEV static bool mask2Test(uint64_t const m0, uint64_t const m1, uint32_t const p) { return p < 64u ? ((m0 >> p) & 1ull) != 0 : ((m1 >> (p-64u)) & 1ull) != 0; }
	DEV static uint32_t mask2Rank(uint64_t const m0, uint64_t const m1, uint32_t const p)
	{
		return p < 64u ? dacc_popc64(m0 & ((1ull<<p)-1ull)) : dacc_popc64(m0) + dacc_popc64(m1 & ((1ull<<(p-64u))-1ull));
	}
	// (tier of w = 128) the same over three words (m2: positions 128-191); the words are chosen by selects
	DEV static bool mask3Test(uint64_t const m0, uint64_t const m1, uint64_t const m2, uint32_t const p)
	{
		uint32_t const wd = p >> 6; uint64_t const m = wd == 0 ? m0 : (wd == 1 ? m1 : m2);
		return ((m >> (p & 63u)) & 1ull) != 0;
	}
	DEV static uint32_t mask3Rank(uint64_t const m0, uint64_t const m1, uint64_t const m2, uint32_t const p)
	{
		uint32_t const wd = p >> 6; uint64_t const below = (1ull << (p & 63u)) - 1ull;
		uint64_t const m = wd == 0 ? m0 : (wd == 1 ? m1 : m2);
		return (wd >= 1 ? dacc_popc64(m0) : 0u) + (wd >= 2 ? dacc_popc64(m1) : 0u) + dacc_popc64(m & below);
	}
	DEV int32_t sfFind(uint32_t const s, uint32_t const p) const
	{
		FEAS_NEED_PROBE(s,false,p)
		if constexpr ( FastRows3<CT>::value != 0 )
		{
			if ( p >= 192 ) return -1;
			uint64_t const m0 = L.maskF()[s], m1 = L.maskFh()[s], m2 = L.maskFx()[s];
			if ( !mask3Test(m0,m1,m2,p) ) return -1;
			return L.woffF()[s] + mask3Rank(m0,m1,m2,p);
		}
		else if constexpr ( CT::wide != 0 )
		{
			if ( p >= 128 ) return -1;
			uint64_t const m0 = L.maskF()[s], m1 = L.maskFh()[s];
			if ( !mask2Test(m0,m1,p) ) return -1;
			return L.woffF()[s] + mask2Rank(m0,m1,p);
		}
		if ( p >= 64 ) return -1;
		uint64_t const m = L.maskF()[s];
		if ( !((m>>p)&1) ) return -1;
		return L.woffF()[s] + dacc_popc64(m & ((1ull<<p)-1));
	}
	DEV int32_t csfFind(uint32_t const s, uint32_t const p) const
	{
		FEAS_NEED_PROBE(s,true,p)
		if constexpr ( FastRows3<CT>::value != 0 )
		{
			if ( p >= 192 ) return -1;
			uint64_t const m0 = L.maskR()[s], m1 = L.maskRh()[s], m2 = L.maskRx()[s];
			if ( !mask3Test(m0,m1,m2,p) ) return -1;
			return L.woffR()[s] + mask3Rank(m0,m1,m2,p);
		}
		else if constexpr ( CT::wide != 0 )
		{
			if ( p >= 128 ) return -1;
			uint64_t const m0 = L.maskR()[s], m1 = L.maskRh()[s];
			if ( !mask2Test(m0,m1,p) ) return -1;
			return L.woffR()[s] + mask2Rank(m0,m1,p);
		}
		if ( p >= 64 ) return -1;
		uint64_t const m = L.maskR()[s];
		if ( !((m>>p)&1) ) return -1;
		return L.woffR()[s] + dacc_popc64(m & ((1ull<<p)-1));
	}
	// getReverseStretchLinkWeight(A=i,B=b) >= 0.1 (computeStretchLinks :3388-3480), evaluated on demand
	DEV bool linkOk(uint32_t const i, uint32_t const b) const
	{
		FEAS_NEED_LINK(i,b)
		uint32_t const shift = L.sslen()[b]-1;
		if constexpr ( FastRows3<CT>::value != 0 )
		{
			if ( shift >= 192 ) return false;
			uint64_t const a0 = L.maskR()[i], a1 = L.maskRh()[i], a2 = L.maskRx()[i], b0 = L.maskR()[b], b1 = L.maskRh()[b], b2 = L.maskRx()[b];
			// (b0,b1,b2) << shift over 192 bits: by whole words first, then by the bits left, every word in a select
			uint32_t const wsh = shift >> 6, bsh = shift & 63u;
			uint64_t const w0 = wsh == 0 ? b0 : 0ull, w1 = wsh == 0 ? b1 : (wsh == 1 ? b0 : 0ull), w2 = wsh == 0 ? b2 : (wsh == 1 ? b1 : b0);
			uint64_t const s0 = w0 << bsh;
			uint64_t const s1 = (w1 << bsh) | (bsh ? (w0 >> (64u-bsh)) : 0ull);
			uint64_t const s2 = (w2 << bsh) | (bsh ? (w1 >> (64u-bsh)) : 0ull);
			uint64_t c0 = a0 & s0, c1 = a1 & s1, c2 = a2 & s2;
			uint64_t weight = 0;
			while ( c0 | c1 | c2 )
			{
				uint32_t const wd = c0 ? 0u : (c1 ? 1u : 2u);
				uint64_t const cw = wd == 0 ? c0 : (wd == 1 ? c1 : c2);
				uint32_t const pa = 64u*wd + static_cast<uint32_t>(__builtin_ctzll(cw));
				uint64_t const cn = cw & (cw-1);
				c0 = wd == 0 ? cn : c0; c1 = wd == 1 ? cn : c1; c2 = wd == 2 ? cn : c2;
				uint32_t const ia = L.woffR()[i] + mask3Rank(a0,a1,a2,pa);
				uint32_t const pb = pa-shift;
				uint32_t const ib = L.woffR()[b] + mask3Rank(b0,b1,b2,pb);
				WR const ra = recR(ia);
				uint64_t const lweight = wuR(ib) + (ra.w - ra.w1);
				weight = lweight > weight ? lweight : weight;
			}
			return weight >= FW_THRES_01;
		}
		else if constexpr ( CT::wide != 0 )
		{
			if ( shift >= 128 ) return false;
			uint64_t const a0 = L.maskR()[i], a1 = L.maskRh()[i], b0 = L.maskR()[b], b1 = L.maskRh()[b];
			// (b0,b1) << shift over 128 bits
			uint64_t const s0 = shift < 64u ? (b0 << shift) : 0ull;
			uint64_t const s1 = shift < 64u ? ((b1 << shift) | (shift ? (b0 >> (64u-shift)) : 0ull)) : (b0 << (shift-64u));
			uint64_t c0 = a0 & s0, c1 = a1 & s1;
			uint64_t weight = 0;
			while ( c0 | c1 )
			{
				uint32_t pa;
				if ( c0 ) { pa = __builtin_ctzll(c0); c0 &= c0-1; } else { pa = 64u + static_cast<uint32_t>(__builtin_ctzll(c1)); c1 &= c1-1; }
				uint32_t const ia = L.woffR()[i] + mask2Rank(a0,a1,pa);
				uint32_t const pb = pa-shift;
				uint32_t const ib = L.woffR()[b] + mask2Rank(b0,b1,pb);
				WR const ra = recR(ia);
				uint64_t const lweight = wuR(ib) + (ra.w - ra.w1);
				weight = lweight > weight ? lweight : weight;
			}
			return weight >= FW_THRES_01;
		}
		if ( shift >= 64 ) return false;
		uint64_t const mA = L.maskR()[i], mB = L.maskR()[b];
		uint64_t common = mA & (mB<<shift);
		uint64_t weight = 0;
		while ( common )
		{
			uint32_t const pa = __builtin_ctzll(common); common &= common-1;
			uint32_t const ia = L.woffR()[i] + dacc_popc64(mA & ((1ull<<pa)-1));
			uint32_t const pb = pa-shift;
			uint32_t const ib = L.woffR()[b] + dacc_popc64(mB & ((1ull<<pb)-1));
			WR const ra = recR(ia);
			uint64_t const lweight = wuR(ib) + (ra.w - ra.w1);
			weight = lweight > weight ? lweight : weight;
		}
		return weight >= FW_THRES_01;
	}

	// ================= views: the stretch set of a pair in sorted order =================
	// view = base stretches (pool ids 0..n0-1, already in Stretch::operator< order) minus the split parents plus the
	// pieces.  It is never materialised: the enumerations look stretches up by first / last node (fhead = npred region,
	// lhead/lord) and merge the <= 4 inserted pieces by their position ppos among the base stretches.  A view lives in
	// registers (every lane has its own): e[i] = piece | position << 8 | first node << 16 | last node << 32.
	struct View { uint32_t nadd; uint32_t r0, r1; uint64_t e0, e1, e2, e3; };
	struct MIt { uint32_t i, a, target; };
	// number of base stretches whose key is smaller than the key of pool stretch s
	DEV uint32_t basePos(uint32_t const s) const
	{
		uint64_t const key = poolKey(s);
		uint32_t lo = 0, hi = n0;
		while ( lo < hi ) { uint32_t const mid = (lo+hi)>>1; if ( poolKey(mid) < key ) lo = mid+1; else hi = mid; }
		return lo;
	}
	DEV static void viewClear(View & V) { V.nadd = 0; V.r0 = 0xFFFF; V.r1 = 0xFFFF; V.e0 = V.e1 = V.e2 = V.e3 = 0; }
	DEV static void viewRemove(View & V, uint32_t const s) { if ( V.r0 == 0xFFFF ) V.r0 = s; else V.r1 = s; }
	// (masks instead of selects: a select chain over four registers is turned into an indexed access of a scratch array)
	DEV static uint64_t viewE(View const & V, uint32_t const i)
	{
		uint64_t const m0 = 0ull - static_cast<uint64_t>(i == 0), m1 = 0ull - static_cast<uint64_t>(i == 1), m2 = 0ull - static_cast<uint64_t>(i == 2), m3 = 0ull - static_cast<uint64_t>(i == 3);
		return (V.e0 & m0) | (V.e1 & m1) | (V.e2 & m2) | (V.e3 & m3);
	}
	DEV static uint32_t vAdd(uint64_t const e) { return static_cast<uint32_t>(e) & SMASK; }
	DEV static uint32_t vPos(uint64_t const e) { return static_cast<uint32_t>(e>>SB) & SMASK; }
	DEV static uint32_t vFn(uint64_t const e) { return static_cast<uint32_t>(e>>(2*SB)) & 0xFFFF; }
	DEV static uint32_t vLn(uint64_t const e) { return static_cast<uint32_t>(e>>(2*SB+16)) & 0xFFFF; }
	DEV void viewAdd(View & V, uint32_t const s) const
	{
		uint32_t const pos = L.ppos()[s];
		uint64_t const key = poolKey(s);
		uint64_t const ne = s | (static_cast<uint64_t>(pos)<<SB) | (static_cast<uint64_t>(L.sfirst()[s])<<(2*SB)) | (static_cast<uint64_t>(L.slast()[s])<<(2*SB+16));
		// keep the insertions sorted by (position, key)
		uint32_t i = V.nadd;
		#define DACC_VSHIFT(Q,PE,DST) if ( i == Q ) { uint64_t const pe = PE; if ( vPos(pe) > pos || (vPos(pe) == pos && poolKey(vAdd(pe)) > key) ) { DST = pe; i = Q-1; } }
		DACC_VSHIFT(3,V.e2,V.e3) DACC_VSHIFT(2,V.e1,V.e2) DACC_VSHIFT(1,V.e0,V.e1)
		#undef DACC_VSHIFT
		{
			uint64_t const m0 = 0ull - static_cast<uint64_t>(i == 0), m1 = 0ull - static_cast<uint64_t>(i == 1), m2 = 0ull - static_cast<uint64_t>(i == 2), m3 = 0ull - static_cast<uint64_t>(i == 3);
			V.e0 = (V.e0 & ~m0) | (ne & m0); V.e1 = (V.e1 & ~m1) | (ne & m1); V.e2 = (V.e2 & ~m2) | (ne & m2); V.e3 = (V.e3 & ~m3) | (ne & m3);
		}
		++V.nadd;
	}
	DEV static bool viewRemoved(View const & V, uint32_t const s) { return s == V.r0 || s == V.r1; }
	// view stretches whose first node is `node`, in view order
	DEV void byFirstBegin(View const &, MIt & it, uint32_t const node) const { it.i = fheadOf(node); it.a = 0; it.target = node; }
	DEV int32_t byFirstNext(View const & V, MIt & it) const
	{
		while ( true )
		{
			while ( it.a < V.nadd && vFn(viewE(V,it.a)) != it.target ) ++it.a;
			bool const haveb = it.i < n0 && L.sfirst()[it.i] == it.target;
			if ( it.a < V.nadd && ( !haveb || vPos(viewE(V,it.a)) <= it.i ) ) return vAdd(viewE(V,it.a++));
			if ( !haveb ) return -1;
			uint32_t const sx = it.i++;
			if ( !viewRemoved(V,sx) ) return sx;
		}
	}
	// view stretches whose last node is `node`, in view order
	DEV void byLastBegin(View const &, MIt & it, uint32_t const node) const { it.i = L.lhead()[node]; it.a = 0; it.target = node; }
	DEV int32_t byLastNext(View const & V, MIt & it) const
	{
		while ( true )
		{
			while ( it.a < V.nadd && vLn(viewE(V,it.a)) != it.target ) ++it.a;
			uint32_t const e = it.i < n0 ? L.lord()[it.i] : 0xFFFFFFFFu;
			bool const haveb = (e>>SB) == it.target;
			uint32_t const sx = e & SMASK;
			if ( it.a < V.nadd && ( !haveb || vPos(viewE(V,it.a)) <= sx ) ) return vAdd(viewE(V,it.a++));
			if ( !haveb ) return -1;
			++it.i;
			if ( !viewRemoved(V,sx) ) return sx;
		}
	}
	DEV uint32_t fheadOf(uint32_t const node) const { return L.npred()[node]; }   // npred is free once the stretches are walked

	// 16 byte records are moved as two 64 bit words (struct copies cannot bind LDS lvalues to generic references)
	template<typename TT> DEV static TT ldget(LDSQ TT const * p)
	{
		static_assert(sizeof(TT) == 16,"record size");
		LDSQ uint64_t const * q = reinterpret_cast<LDSQ uint64_t const *>(p);
		uint64_t u[2]; u[0] = q[0]; u[1] = q[1];
		TT t; __builtin_memcpy(&t,u,16); return t;
	}
	template<typename TT> DEV static void ldput(LDSQ TT * p, TT const & t)
	{
		uint64_t u[2]; __builtin_memcpy(u,&t,16);
		LDSQ uint64_t * q = reinterpret_cast<LDSQ uint64_t *>(p);
		q[0] = u[0]; q[1] = u[1];
	}
	template<typename TT> DEV static void ldswap(LDSQ TT * a, LDSQ TT * b)
	{
		LDSQ uint64_t * x = reinterpret_cast<LDSQ uint64_t *>(a); LDSQ uint64_t * y = reinterpret_cast<LDSQ uint64_t *>(b);
		uint64_t const x0 = x[0], x1 = x[1], y0 = y[0], y1 = y[1];
		x[0] = y0; x[1] = y1; y[0] = x0; y[1] = x1;
	}
	// ---- heaps (same sift algorithm as oracle/o_heap.hpp) ----
	template<bool MINHEAP> DEV static bool hless(uint64_t a, uint64_t b) { return MINHEAP ? (a < b) : (a > b); }
	// (id heaps: a version that keeps the moving id and its weight in registers measured 7 % slower in the forward trees --
	// the re-read of W[H[i]] is in flight together with the children's weights, it costs no round trip)
	template<bool MINHEAP>
	DEV void ipush(LDSQ id_t * H, uint32_t & f, id_t const id, LDSQ uint64_t const * W)
	{
		uint32_t i = f++; H[i] = id;
		while ( i )
		{
			uint32_t const p = (i-1)>>1;
			if ( hless<MINHEAP>(W[H[i]],W[H[p]]) ) { id_t const t = H[i]; H[i] = H[p]; H[p] = t; i = p; }
			else break;
		}
	}
	template<bool MINHEAP>
	DEV void ipop(LDSQ id_t * H, uint32_t & f, LDSQ uint64_t const * W)
	{
		H[0] = H[--f];
		uint32_t i = 0, r;
		while ( (r = 2*i+2) < f )
		{
			uint32_t const m = hless<MINHEAP>(W[H[r-1]],W[H[r]]) ? (r-1) : r;
			if ( hless<MINHEAP>(W[H[i]],W[H[m]]) ) return;
			id_t const t = H[i]; H[i] = H[m]; H[m] = t; i = m;
		}
		uint32_t const l = 2*i+1;
		if ( l < f && !hless<MINHEAP>(W[H[i]],W[H[l]]) ) { id_t const t = H[i]; H[i] = H[l]; H[l] = t; }
	}
	// The record that moves stays in registers and the records it passes are shifted (same comparisons and the same final
	// arrangement as swapping level by level): one LDS round trip per level.
	template<typename TT, bool MINHEAP>
	DEV void spush(LDSQ TT * H, uint32_t & f, TT const & e)
	{
		uint32_t i = f++;
		while ( i )
		{
			uint32_t const p = (i-1)>>1;
			TT const ep = ldget(H+p);
			if ( hless<MINHEAP>(e.w,ep.w) ) { ldput(H+i,ep); i = p; }
			else break;
		}
		ldput(H+i,e);
	}
	template<typename TT, bool MINHEAP>
	DEV void spop(LDSQ TT * H, uint32_t & f)
	{
		--f; TT const e = ldget(H+f);
		uint32_t i = 0, r;
		while ( (r = 2*i+2) < f )
		{
			TT const a = ldget(H+r-1), b = ldget(H+r);
			bool const pa = hless<MINHEAP>(a.w,b.w);
			uint64_t const wm = pa ? a.w : b.w;
			if ( hless<MINHEAP>(e.w,wm) ) { ldput(H+i,e); return; }
			if ( pa ) { ldput(H+i,a); i = r-1; } else { ldput(H+i,b); i = r; }
		}
		uint32_t const l = 2*i+1;
		if ( l < f )
		{
			TT const el = ldget(H+l);
			if ( !hless<MINHEAP>(e.w,el.w) ) { ldput(H+i,el); i = l; }
		}
		ldput(H+i,e);
	}

	// ================= per-lane path enumerations =================
	// The reverse enumeration of every last k-mer candidate and the forward enumeration of every first k-mer candidate
	// are independent of each other, so they run on one lane each (lane = candidate), all candidates of a window at once;
	// the same routines run on lane 0 alone for the rare pair that needs its exact stretch set.  Paths live in shared
	// pools (rc_* / f_*, indexed by a pool-wide id); a lane takes pool entries in chunks of RCH / FCH through an LDS
	// counter and keeps its chunk list in registers (entry i of an enumeration -> clSlot).
	enum { RCH = CT::rch, RNW = 4, FCH = CT::fch, FNW = CT::fnw, FNC = CT::fnc };         // entries per chunk, 64 bit words of chunk ids (8 per word)
	// The chunk ids of an enumeration are a row of bytes in LDS (a register array indexed at run time would end up in
	// scratch memory): NW*8 chunks per enumeration.
	template<int NW> struct ChunkList { LDSQ uint8_t * ids; uint32_t n; };
	template<int NW> DEV static void clInit(ChunkList<NW> & C, LDSQ uint8_t * row) { C.ids = row; C.n = 0; }
	template<int PCH, int NW> DEV static uint32_t clSlot(ChunkList<NW> const & C, uint32_t const i) { return static_cast<uint32_t>(C.ids[i/PCH])*PCH + (i%PCH); }
	// slot of entry i, taking a new chunk from the pool when i starts one; ~0u: pool or chunk list exhausted
	template<int PCH, int NW> DEV uint32_t clEnsure(ChunkList<NW> & C, uint32_t const i, LDSQ uint32_t * ctr, uint32_t const nchunks)
	{
		uint32_t const ch = i/PCH;
		if ( ch >= C.n )
		{
			if ( ch >= 8*NW ) return ~0u;
			uint32_t const id = wv_atomic_add(ctr,1u);
			if ( id >= nchunks || id > 255 ) return ~0u;
			C.ids[ch] = id;
			C.n = ch+1;
			return id*PCH + (i%PCH);
		}
		return clSlot<PCH>(C,i);
	}

	// ---- reverse enumeration (prepareTraverse :3582-3765) of one last k-mer on view V ----
	struct REnum { ChunkList<RNW> C; uint32_t nrp, narp, lastk; };
	// extendReversePath :4058-4105 with the parent's fields and the feasible entry sfo = csfFind(s,ppos) in registers
	// (checkReversePathFeasiblePosition :4130-4159 looks the same entry up again: the check position is the parent's)
	DEV int32_t extendReversePath(REnum & R, uint32_t const parent, uint32_t const s, uint32_t const ppos, uint32_t const plen, uint64_t const pw, uint32_t const pbl, int32_t const sfo, uint64_t const wr, uint64_t const wr1)
	{
		uint32_t const slot = clEnsure<RCH>(R.C,R.nrp,L.ctr()+0,CT::rccap/RCH);
		if ( slot == ~0u ) { over(512|0x4000); return -1; }
		uint32_t const slen = L.sslen()[s];
		uint64_t weight = pw; uint32_t baselen = pbl;
		if ( plen == 0 ) { baselen = slen+k-1; weight = sfo >= 0 ? wr : 0; }
		else { baselen += slen-1; if ( sfo >= 0 ) weight += wr - wr1; }
		uint32_t const npos = ppos + slen-1;
		if ( baselen > 255 || npos > 255 || plen+1 > 255 ) { over(2048); return -1; }
		++R.nrp;
		L.rc_parent()[slot] = parent; L.rc_stretch()[slot] = s; L.rc_len()[slot] = plen+1; L.rc_pos()[slot] = npos;
		L.rc_w()[slot] = weight; L.rc_baselen()[slot] = baselen;
		return slot;
	}
	DEV uint32_t rpFront(uint32_t const id, uint32_t const lastk) const { return L.rc_len()[id] ? L.nv()[L.sfirst()[L.rc_stretch()[id]]] : lastk; }
	// accepted paths are listed in acceptance order in the enumeration's own slots (rc_acc); rpst = the lane's heap
	DEV void reverseEnumerateLane(REnum & R, LDSQ uint8_t * chunkrow, View const & V, uint32_t const lastkmer, int32_t const lastnode, int64_t const lmax, LDSQ id_t * rpst, uint32_t const rpstcap)
	{
		clInit(R.C,chunkrow); R.nrp = 0; R.narp = 0; R.lastk = lastkmer;
		uint32_t nrpst = 0;
		if ( lastnode >= 0 )
		{
			uint32_t const slot = clEnsure<RCH>(R.C,0,L.ctr()+0,CT::rccap/RCH);
			if ( slot == ~0u ) { over(512|0x4000); return; }
			R.nrp = 1;
			L.rc_parent()[slot] = 0; L.rc_stretch()[slot] = SNONE; L.rc_len()[slot] = 0; L.rc_pos()[slot] = 0; L.rc_w()[slot] = 0; L.rc_baselen()[slot] = k;
			rpst[nrpst++] = slot;
		}
		LDSQ uint64_t const * W = L.rc_w();
		SITE_T0
		while ( nrpst )
		{
			uint32_t const rp = rpst[0];
			ipop<false>(rpst,nrpst,W);
			uint32_t const bl = L.rc_baselen()[rp], ppos = L.rc_pos()[rp], plen = L.rc_len()[rp];
			uint64_t const pw = W[rp];
			SITE(17)      // reverse enumeration: pop of the heaviest pending path + its fields
			// ARPH[bl] (:3626-3665) keeps the 12 heaviest accepted paths of a base length and admits a path only if it is
			// heavier than the lightest of them: a path is dropped iff 12 accepted paths of its length weigh at least as much
			if ( R.narp >= 12 )
			{
				uint32_t cnt = 0;
				for ( uint32_t i = 0; i < R.narp; ++i )
				{
					uint32_t const a = L.rc_acc()[clSlot<RCH>(R.C,i)];
					cnt += (L.rc_baselen()[a] == bl && W[a] >= pw) ? 1 : 0;
				}
				SITE(18)      // reverse enumeration: the 12 heaviest accepted paths of this base length
				if ( cnt >= 12 ) continue;
			}
			L.rc_acc()[clSlot<RCH>(R.C,R.narp)] = rp; ++R.narp;
			if ( plen == 0 )
			{
				MIt it; byLastBegin(V,it,lastnode);
				for ( int32_t sx = byLastNext(V,it); sx >= 0; sx = byLastNext(V,it) )
				{
					int32_t const sfo = csfFind(sx,ppos);
					WR rr; rr.w = 0; rr.w1 = 0; if ( sfo >= 0 ) rr = recR(sfo);
					uint64_t const wr = rr.w;
					if ( !(sfo >= 0 && wr >= FW_THRES_05) ) continue;     // the new path would be dropped right away
					int32_t const rpe = extendReversePath(R,rp,sx,ppos,plen,pw,bl,sfo,wr,rr.w1);
					if ( rpe < 0 ) return;
					if ( nrpst >= rpstcap ) { over(512|0x8000); return; }
					ipush<false>(rpst,nrpst,static_cast<id_t>(rpe),W);
				}
				SITE(19)      // reverse enumeration: the root's extensions
			}
			else if ( static_cast<int64_t>(bl) < (lmax+1)/2 )
			{
				uint32_t const b = L.rc_stretch()[rp];
				uint32_t const bf = L.sfirst()[b];
				MIt it; byLastBegin(V,it,bf);
				for ( int32_t ax = byLastNext(V,it); ax >= 0; ax = byLastNext(V,it) )
				{
					uint32_t const a = ax;
					if ( linkOk(a,b) )
					{
						int32_t const sfo = csfFind(a,ppos);
						WR rr; rr.w = 0; rr.w1 = 0; if ( sfo >= 0 ) rr = recR(sfo);
						uint64_t const wr = rr.w;
						if ( !(sfo >= 0 && wr >= FW_THRES_05) ) continue;
						int32_t const rpe = extendReversePath(R,rp,a,ppos,plen,pw,bl,sfo,wr,rr.w1);
						if ( rpe < 0 ) return;
						if ( nrpst >= rpstcap ) { over(512|0x8000); return; }
						ipush<false>(rpst,nrpst,static_cast<id_t>(rpe),W);
					}
					SITE(20)      // reverse enumeration: one predecessor stretch of a popped path (iterator, link weight, record, push)
				}
			}
			SITE_RESET
		}
	}
	// ---- block of a finished reverse enumeration in sorted order at rc_ord/rc_arw/rc_sbl/rc_front[sbase..sbase+narp) ----
	DEV bool arpLess(uint32_t const a, uint32_t const b, uint32_t const lastk) const
	{
		uint32_t const fa = rpFront(a,lastk), fb = rpFront(b,lastk);
		if ( fa != fb ) return fa < fb;
		return L.rc_baselen()[a] < L.rc_baselen()[b];
	}
	DEV void arpULI(LDSQ id_t * last, uint32_t const lk) { id_t const val = *last; LDSQ id_t * next = last-1; while ( arpLess(val,*next,lk) ) { *last = *next; last = next; --next; } *last = val; }
	DEV void arpIns(LDSQ id_t * first, LDSQ id_t * last, uint32_t const lk)
	{
		if ( first == last ) return;
		for ( LDSQ id_t * i = first+1; i != last; ++i )
		{
			if ( arpLess(*i,*first,lk) ) { id_t const val = *i; for ( LDSQ id_t * q = i; q != first; --q ) *q = *(q-1); *first = val; }
			else arpULI(i,lk);
		}
	}
	// libstdc++ std::sort permutation (introsort + final insertion sort), see dbg_window.hpp arpSort; more than 16
	// elements need the (single) explicit stack L.sstack, so only one lane at a time may sort such a block.  At introsort's depth
	// limit the window is handed on with flag 1024: the heapsort fallback is reproduced in the generic engine only
	DEV void arpSort(LDSQ id_t * first, LDSQ id_t * last, uint32_t const lk)
	{
		if ( first == last ) return;
		int32_t const n = last-first;
		if ( n > 16 )
		{
			int depth = 0; { int32_t t = n; while ( t > 1 ) { t >>= 1; ++depth; } depth *= 2; }
			LDSQ uint16_t * stF = L.sstack(); LDSQ uint16_t * stL = stF+24; LDSQ uint16_t * stD = stF+48; int sp = 0;   // offsets from first
			stF[0] = 0; stL[0] = n; stD[0] = depth; sp = 1;
			while ( sp )
			{
				--sp;
				LDSQ id_t * f = first+stF[sp]; LDSQ id_t * l = first+stL[sp]; int d = stD[sp];
				while ( l-f > 16 )
				{
					if ( d == 0 ) { over(1024); return; }
					--d;
					LDSQ id_t * mid = f + (l-f)/2; LDSQ id_t * a = f+1; LDSQ id_t * b = mid; LDSQ id_t * c = l-1;
					if ( arpLess(*a,*b,lk) )
					{
						if ( arpLess(*b,*c,lk) ) { id_t t = *f; *f = *b; *b = t; }
						else if ( arpLess(*a,*c,lk) ) { id_t t = *f; *f = *c; *c = t; }
						else { id_t t = *f; *f = *a; *a = t; }
					}
					else if ( arpLess(*a,*c,lk) ) { id_t t = *f; *f = *a; *a = t; }
					else if ( arpLess(*b,*c,lk) ) { id_t t = *f; *f = *c; *c = t; }
					else { id_t t = *f; *f = *b; *b = t; }
					LDSQ id_t * lo = f+1; LDSQ id_t * hi = l;
					while ( true )
					{
						while ( arpLess(*lo,*f,lk) ) ++lo;
						--hi;
						while ( arpLess(*f,*hi,lk) ) --hi;
						if ( !(lo < hi) ) break;
						id_t t = *lo; *lo = *hi; *hi = t;
						++lo;
					}
					if ( sp < 24 ) { stF[sp] = lo-first; stL[sp] = l-first; stD[sp] = d; ++sp; } else { over(1024); return; }
					l = lo;
				}
			}
			arpIns(first,first+16,lk);
			for ( LDSQ id_t * i = first+16; i != last; ++i ) arpULI(i,lk);
		}
		else arpIns(first,last,lk);
	}
	// The same sort on (id, key) pairs: key = front k-mer << 8 | base length, so that key order is arpLess order and a comparison is two
	// independent loads instead of two chains of four (path -> stretch -> first node -> k-mer).  Same comparisons with the same
	// outcomes in the same order, hence the same permutation.  I / K: ids and keys of the block, indexed from its start.
	DEV static void arpSwapK(LDSQ id_t * I, LDSQ uint64_t * K, int32_t const a, int32_t const b) { id_t const t = I[a]; I[a] = I[b]; I[b] = t; uint64_t const u = K[a]; K[a] = K[b]; K[b] = u; }
	DEV static void arpULIK(LDSQ id_t * I, LDSQ uint64_t * K, int32_t last) { id_t const vi = I[last]; uint64_t const vk = K[last]; int32_t next = last-1; while ( vk < K[next] ) { I[last] = I[next]; K[last] = K[next]; last = next; --next; } I[last] = vi; K[last] = vk; }
	DEV static void arpInsK(LDSQ id_t * I, LDSQ uint64_t * K, int32_t const first, int32_t const last)
	{
		if ( first == last ) return;
		for ( int32_t i = first+1; i != last; ++i )
		{
			if ( K[i] < K[first] ) { id_t const vi = I[i]; uint64_t const vk = K[i]; for ( int32_t q = i; q != first; --q ) { I[q] = I[q-1]; K[q] = K[q-1]; } I[first] = vi; K[first] = vk; }
			else arpULIK(I,K,i);
		}
	}
	DEV void arpSortK(LDSQ id_t * I, LDSQ uint64_t * K, int32_t const n)
	{
		if ( n == 0 ) return;
		if ( n > 16 )
		{
			int depth = 0; { int32_t t = n; while ( t > 1 ) { t >>= 1; ++depth; } depth *= 2; }
			LDSQ uint16_t * stF = L.sstack(); LDSQ uint16_t * stL = stF+24; LDSQ uint16_t * stD = stF+48; int sp = 0;
			stF[0] = 0; stL[0] = n; stD[0] = depth; sp = 1;
			while ( sp )
			{
				--sp;
				int32_t f = stF[sp], l = stL[sp]; int d = stD[sp];
				while ( l-f > 16 )
				{
					if ( d == 0 ) { over(1024); return; }
					--d;
					int32_t const mid = f + (l-f)/2, a = f+1, b = mid, c = l-1;
					if ( K[a] < K[b] )
					{
						if ( K[b] < K[c] ) arpSwapK(I,K,f,b);
						else if ( K[a] < K[c] ) arpSwapK(I,K,f,c);
						else arpSwapK(I,K,f,a);
					}
					else if ( K[a] < K[c] ) arpSwapK(I,K,f,a);
					else if ( K[b] < K[c] ) arpSwapK(I,K,f,c);
					else arpSwapK(I,K,f,b);
					int32_t lo = f+1, hi = l;
					while ( true )
					{
						while ( K[lo] < K[f] ) ++lo;
						--hi;
						while ( K[f] < K[hi] ) --hi;
						if ( !(lo < hi) ) break;
						arpSwapK(I,K,lo,hi);
						++lo;
					}
					if ( sp < 24 ) { stF[sp] = lo; stL[sp] = l; stD[sp] = d; ++sp; } else { over(1024); return; }
					l = lo;
				}
			}
			arpInsK(I,K,0,16);
			for ( int32_t i = 16; i != n; ++i ) arpULIK(I,K,i);
		}
		else arpInsK(I,K,0,n);
	}
	// copy the accepted list to its block (acceptance order)
	DEV void reverseBlockCopy(REnum const & R, uint32_t const sbase)
	{
		for ( uint32_t i = 0; i < R.narp; ++i ) L.rc_ord()[sbase+i] = L.rc_acc()[clSlot<RCH>(R.C,i)];
	}
	// sort the block and derive what the score intervals need; slot li of the per-candidate tables gets the summary
	// WTMP: the forward pools are not in use yet (the cached blocks are finished before the first batch of trees): the block's weights
	// are laid out in block order in the forward weight array first, so that the quadratic rank loop reads one value per step, four
	// steps at a time, instead of two dependent loads per step (round 5: site 21 of the ledger, 3 % of a window of config 2)
	template<bool WTMP = false>
	DEV void reverseBlockFinish(REnum const & R, uint32_t const sbase, uint32_t const li, int32_t const lastnode, int64_t const lmax)
	{
		uint32_t const narp = R.narp;
		LDSQ uint64_t const * W = L.rc_w();
		constexpr bool TMP = WTMP && CT::rccap <= CT::fcap;
		LDSQ uint64_t * const WT = L.f_w() + sbase;
		uint64_t rmaxw = 0, rfm = 0;
		for ( uint32_t i = 0; i < narp; ++i ) { uint64_t const w = W[L.rc_ord()[sbase+i]]; rmaxw = w > rmaxw ? w : rmaxw; }
		if constexpr ( TMP )
		{
			// keys of the block in acceptance order, then the sort on (id, key); WT holds the keys until the ranks need it for the weights
			for ( uint32_t i = 0; i < narp; ++i ) { uint32_t const rp = L.rc_ord()[sbase+i]; WT[i] = (static_cast<uint64_t>(rpFront(rp,R.lastk)) << 8) | L.rc_baselen()[rp]; }
			arpSortK(L.rc_ord()+sbase,WT,static_cast<int32_t>(narp));
			for ( uint32_t i = 0; i < narp; ++i ) { uint64_t const key = WT[i]; L.rc_front()[sbase+i] = static_cast<uint32_t>(key >> 8); L.rc_sbl()[sbase+i] = static_cast<uint8_t>(key & 0xFF); }
			for ( uint32_t i = 0; i < narp; ++i ) WT[i] = W[L.rc_ord()[sbase+i]];
		}
		else arpSort(L.rc_ord()+sbase,L.rc_ord()+sbase+narp,R.lastk);
		// rank of every entry by (weight, sorted position); one bit per scan target (node id mod 64) of the enumeration
		uint64_t tm = lastnode >= 0 ? (1ull << (lastnode & 63)) : 0ull;
		for ( uint32_t i = 0; i < narp; ++i )
		{
			uint32_t const rp = L.rc_ord()[sbase+i];
			uint64_t const wi = W[rp];
			uint32_t r = 0;
			if constexpr ( TMP )
			{
				uint32_t j = 0;
				for ( ; j+4 <= narp; j += 4 )
				{
					uint64_t const w0 = WT[j], w1 = WT[j+1], w2 = WT[j+2], w3 = WT[j+3];
					r += (w0 < wi || (w0 == wi && j < i)) ? 1u : 0u; r += (w1 < wi || (w1 == wi && j+1 < i)) ? 1u : 0u;
					r += (w2 < wi || (w2 == wi && j+2 < i)) ? 1u : 0u; r += (w3 < wi || (w3 == wi && j+3 < i)) ? 1u : 0u;
				}
				for ( ; j < narp; ++j ) { uint64_t const wj = WT[j]; if ( wj < wi || (wj == wi && j < i) ) ++r; }
			}
			else
			for ( uint32_t j = 0; j < narp; ++j )
			{
				uint64_t const wj = W[L.rc_ord()[sbase+j]];
				if ( wj < wi || (wj == wi && j < i) ) ++r;
			}
			L.rc_arw()[sbase+i] = r;
			uint32_t fr;
			if constexpr ( TMP ) fr = L.rc_front()[sbase+i];      // (written from the sort keys above)
			else { fr = rpFront(rp,R.lastk); L.rc_front()[sbase+i] = fr; L.rc_sbl()[sbase+i] = L.rc_baselen()[rp]; }
			rfm |= 1ull << (fr & 63);
			if ( L.rc_len()[rp] && static_cast<int64_t>(L.rc_baselen()[rp]) < (lmax+1)/2 ) tm |= 1ull << (L.sfirst()[L.rc_stretch()[rp]] & 63);
		}
		L.rbase()[li] = sbase; L.rn()[li] = narp; L.rmaxw()[li] = rmaxw; L.rtmask()[li] = tm; L.rfmask()[li] = rfm;
	}
	// can the cached reverse block (computed on the view of `last` alone) be used when stretch `par` is split at node `fn`?
	// the scans of the enumeration look for stretches whose last node equals a target; the split changes the answer
	// only for targets par.last (parent vs second piece) and fn (first piece)
	DEV bool reverseUnaffected(uint32_t const sbase, uint32_t const nacc2, int32_t const lastnode, uint32_t const par, uint32_t const fn, int64_t const lmax) const
	{
		uint32_t const plast = L.slast()[par];
		if ( lastnode >= 0 && (static_cast<uint32_t>(lastnode) == plast || static_cast<uint32_t>(lastnode) == fn) ) return false;
		for ( uint32_t i = 0; i < nacc2; ++i )
		{
			uint32_t const rp = L.rc_ord()[sbase+i];
			if ( L.rc_len()[rp] && static_cast<int64_t>(L.rc_baselen()[rp]) < (lmax+1)/2 )
			{
				uint32_t const target = L.sfirst()[L.rc_stretch()[rp]];
				if ( target == plast || target == fn ) return false;
			}
		}
		return true;
	}

	// ---- forward enumeration (path tree of traverse :4838-5041) of one first k-mer on view V ----
	// APQ[baselen] (:4851-4862, 5003-5017) are bounded heaps of 12 that are filled completely before they are drained
	// (an extension is strictly longer than its parent and the buckets are drained in increasing base length), so a
	// bucket's heap is rebuilt right before it is drained by pushing its paths in creation order: one 12 entry heap per
	// enumeration instead of one per base length, same heap arrays, same pop order among equal weights.
	// (m0, m1: base lengths with pending paths, a bit per length; wide tiers: m2 for 128 ... 191 -- a forward path of a window of 100 bases and more
	// ends beyond 127 when its last stretch is long, profiles/r06w: 364 of 120 000 windows at w = 104 went to the generic engine on this)
	template<bool W, int DUMMY = 0> struct FEnumHi { }; template<int DUMMY> struct FEnumHi<true,DUMMY> { uint64_t m2; };
	struct FEnum : FEnumHi<(CT::wide != 0)> { ChunkList<FNW> C; uint32_t np, nfpop; uint64_t fmaxw, ffm, m0, m1; };
	enum : uint32_t { FBLMAX = CT::wide ? 191u : 127u };
	DEV static void fblSet(FEnum & F, uint32_t const nbl)
	{
		// (wide tiers only; the other tiers keep their two-word statements in place: moved into a function, the compiler turns their
		// branch into selects -- a different instruction stream than the measured one.  Unconditional updates here: a three-way choice of
		// the word makes the compiler address F in scratch memory)
		if constexpr ( CT::wide != 0 )
		{
			uint64_t const b = 1ull << (nbl & 63u); uint32_t const wd = nbl >> 6;
			F.m0 |= wd == 0 ? b : 0ull; F.m1 |= wd == 1 ? b : 0ull; F.m2 |= wd == 2 ? b : 0ull;
		}
	}
	DEV static bool fblAny(FEnum const & F) { if constexpr ( CT::wide != 0 ) return (F.m0 | F.m1 | F.m2) != 0; else return (F.m0 | F.m1) != 0; }
	// lowest pending base length, removed from the masks
	DEV static uint32_t fblPop(FEnum & F)
	{
		if constexpr ( CT::wide == 0 ) return 0;
		else
		{
			uint32_t const wd = F.m0 ? 0u : (F.m1 ? 1u : 2u);
			uint64_t const m = wd == 0 ? F.m0 : (wd == 1 ? F.m1 : F.m2);
			uint64_t const c = m & (m-1);
			F.m0 = wd == 0 ? c : F.m0; F.m1 = wd == 1 ? c : F.m1; F.m2 = wd == 2 ? c : F.m2;
			return 64u*wd + static_cast<uint32_t>(__builtin_ctzll(m));
		}
	}
	DEV int32_t extendPath(FEnum & F, uint32_t const parent, uint32_t const s, uint32_t const ppos, uint32_t const plen, uint64_t const pw, uint32_t const pbl,
		int32_t const sfo, uint64_t const wf, uint64_t const wf1, uint32_t & npos, uint32_t & nbl, uint64_t & nw)
	{
		uint32_t const slot = clEnsure<FCH>(F.C,F.np,L.ctr()+1,CT::fcap/FCH);
		if ( slot == ~0u ) { over(512|0x10000); return -1; }
		uint32_t const slen = L.sslen()[s];
		uint64_t weight = pw; uint32_t baselen = pbl;
		if ( plen == 0 ) { baselen = slen+k-1; weight = sfo >= 0 ? wf : 0; }
		else { baselen += slen-1; if ( sfo >= 0 ) weight += wf - wf1; }
		npos = ppos + (slen-1); nbl = baselen; nw = weight;
		if ( baselen > FBLMAX || npos > 255 || plen+1 > 255 ) { over(2048); return -1; }
		++F.np;
		L.f_parent()[slot] = parent; L.f_stretch()[slot] = s; L.f_len()[slot] = plen+1; L.f_pos()[slot] = npos;
		L.f_w()[slot] = weight; L.f_baselen()[slot] = baselen;
		return slot;
	}
	DEV void forwardEnumerateLane(FEnum & F, LDSQ uint8_t * chunkrow, View const & V, int32_t const firstnode, int64_t const lmax, LDSQ id_t * hp)
	{
		clInit(F.C,chunkrow); F.np = 0; F.nfpop = 0; F.fmaxw = 0; F.ffm = 0; F.m0 = 0; F.m1 = 0; if constexpr ( CT::wide != 0 ) F.m2 = 0;
		if ( firstnode < 0 ) return;
		PROFX_T0      // profiling builds: lane 0's tree, split into filling the bucket heap (19) and draining it (20)
		SITE_T0
		{
			MIt it; byFirstBegin(V,it,firstnode);
			for ( int32_t sx = byFirstNext(V,it); sx >= 0; sx = byFirstNext(V,it) )
			{
				int32_t const sfo = sfFind(sx,0);
				uint64_t const wf = sfo >= 0 ? wuF(sfo) : 0;
				uint32_t npos, nbl; uint64_t nw;
				int32_t const id = extendPath(F,0,sx,0,0,0,0,sfo,wf,0,npos,nbl,nw);
				if ( id < 0 ) return;
				if constexpr ( CT::wide == 0 ) { if ( nbl < 64 ) F.m0 |= 1ull << nbl; else F.m1 |= 1ull << (nbl-64); } else fblSet(F,nbl);
			}
		}
		LDSQ uint64_t const * W = L.f_w();
		SITE(11)      // forward tree: the root's extensions
		// (round 6, measured and dropped: starting a bucket's scan behind the leading entries whose base lengths are already drained -- three
		// more registers and a compare per group of four made the window kernels 0.6 % slower, profiles/r06d)
		while ( fblAny(F) )
		{
			uint32_t zz;
			if constexpr ( CT::wide == 0 )
			{
				zz = F.m0 ? static_cast<uint32_t>(__builtin_ctzll(F.m0)) : 64u + static_cast<uint32_t>(__builtin_ctzll(F.m1));
				if ( zz < 64 ) F.m0 &= F.m0-1; else F.m1 &= F.m1-1;
			}
			else zz = fblPop(F);
			uint32_t hn = 0;
			for ( uint32_t i0 = 0; i0 < F.np; i0 += 64 )
			{
				// members of the bucket among entries i0..i0+63 (loads only, so that they overlap), then the pushes in order
				uint64_t mem = 0;
				uint32_t const ie = (F.np-i0 < 64) ? (F.np-i0) : 64u;
				// four consecutive entries lie in one chunk (FCH is a multiple of four): one chunk id and one 32 bit load of
				// their base lengths
				static_assert(FCH % 4 == 0,"entries per chunk");
				for ( uint32_t i = 0; i < ie; i += 4 )
				{
					uint32_t const slot = clSlot<FCH>(F.C,i0+i);
					uint32_t const b4 = *reinterpret_cast<LDSQ uint32_t const *>(L.f_baselen() + slot);
					#pragma unroll
					for ( uint32_t u = 0; u < 4; ++u ) if ( i+u < ie ) mem |= static_cast<uint64_t>(((b4 >> (8*u)) & 0xFF) == zz) << (i+u);
				}
				SITE(12)      // forward tree: members of the bucket among 64 entries (base length loads)
				while ( mem )
				{
					uint32_t const i = __builtin_ctzll(mem); mem &= mem-1;
					uint32_t const e = clSlot<FCH>(F.C,i0+i);
					if ( hn == 12 )
					{
						if ( W[e] > W[hp[0]] ) { ipop<true>(hp,hn,W); ipush<true>(hp,hn,static_cast<id_t>(e),W); }
					}
					else ipush<true>(hp,hn,static_cast<id_t>(e),W);
				}
				SITE(13)      // forward tree: pushes of the bucket's members into the heap of 12
			}
			PROFX(19)
			while ( hn )
			{
				uint32_t const path = hp[0];
				ipop<true>(hp,hn,W);
				uint32_t const ps = L.f_stretch()[path], ppos = L.f_pos()[path], plen = L.f_len()[path], pbl = zz;
				uint64_t const pw = W[path];
				uint32_t const lastn = L.slast()[ps];
				SITE(14)      // forward tree: pop of the heaviest path of the bucket + its fields
				{
					// what the score intervals need of this path: junction k-mer, candidate length, weight without the junction node
					int32_t const psfo = sfFind(ps,ppos - (L.sslen()[ps]-1));
					uint32_t const pfront = L.nv()[lastn];
					uint32_t const o = clSlot<FCH>(F.C,F.nfpop);
					L.fp_id()[o] = path; L.fp_front()[o] = pfront; L.fp_cl()[o] = ppos; F.ffm |= 1ull << (pfront & 63);
					L.fp_adj()[o] = psfo >= 0 ? (pw - recF(psfo).wl) : pw;
					if ( pw > F.fmaxw ) F.fmaxw = pw;
					++F.nfpop;
				}
				SITE(15)      // forward tree: the popped path's record for the score intervals (weight record from the slab)
				if ( pbl < k || ( static_cast<int64_t>(pbl-k) < ((lmax+1)/2) ) )
				{
					MIt it; byFirstBegin(V,it,lastn);
					for ( int32_t sx = byFirstNext(V,it); sx >= 0; sx = byFirstNext(V,it) )
					{
						uint32_t const s = sx;
						int32_t const sfo = sfFind(s,ppos);
						WF fr; fr.w = 0; fr.w1 = 0; fr.wl = 0; if ( sfo >= 0 ) fr = recF(sfo);
						uint64_t const eweight = fr.w;
						if ( eweight >= FW_THRES_01 )
						{
							uint32_t npos, nbl; uint64_t nw;
							int32_t const ep = extendPath(F,path,s,ppos,plen,pw,pbl,sfo,eweight,fr.w1,npos,nbl,nw);
							if ( ep < 0 ) return;
							if ( nw >= FW_THRES_01 && static_cast<int64_t>(npos) + k <= lmax )
							{
								if constexpr ( CT::wide == 0 ) { if ( nbl < 64 ) F.m0 |= 1ull << nbl; else F.m1 |= 1ull << (nbl-64); } else fblSet(F,nbl);
							}
							else --F.np;
						}
						SITE(16)      // forward tree: one successor stretch of a popped path (view iterator, weight record, new path)
					}
				}
				SITE_RESET
			}
			SITE_RESET      // (lanes that left the drain loop early wait here for the others: not the scan's time)
			PROFX(20)
		}
	}
	// summary of a finished forward tree in slot fi of the per-candidate tables; one bit per scan target
	DEV void forwardTreeFinish(FEnum const & F, uint32_t const fi, int32_t const firstnode, int64_t const lmax)
	{
		uint64_t m = firstnode >= 0 ? (1ull << (firstnode & 63)) : 0ull;
		for ( uint32_t i = 0; i < F.nfpop; ++i )
		{
			uint32_t const path = L.fp_id()[clSlot<FCH>(F.C,i)];
			uint32_t const pbl = L.f_baselen()[path];
			if ( pbl < k || ( static_cast<int64_t>(pbl-k) < ((lmax+1)/2) ) ) m |= 1ull << (L.slast()[L.f_stretch()[path]] & 63);
		}
		L.fnp()[fi] = F.nfpop; L.ffm()[fi] = F.ffm; L.ftm()[fi] = m; L.fmx()[fi] = F.fmaxw;
	}
	DEV void forwardTreeLoad(ChunkList<FNW> & C, uint32_t const fi) const { C.ids = L.fchb() + 8*FNW*fi; C.n = 8*FNW; }
	// scans of the forward enumeration look for stretches whose first node equals a target; splitting `par` at `ln`
	// changes the answer only for targets par.first (parent vs first piece) and ln (second piece)
	DEV bool forwardUnaffected(ChunkList<FNW> const & C, uint32_t const nfpop, int32_t const firstnode, uint32_t const par, uint32_t const ln, int64_t const lmax) const
	{
		uint32_t const pfirst = L.sfirst()[par];
		if ( static_cast<uint32_t>(firstnode) == pfirst || static_cast<uint32_t>(firstnode) == ln ) return false;
		for ( uint32_t i = 0; i < nfpop; ++i )
		{
			uint32_t const path = L.fp_id()[clSlot<FCH>(C,i)];
			uint32_t const pbl = L.f_baselen()[path];
			if ( pbl < k || ( static_cast<int64_t>(pbl-k) < ((lmax+1)/2) ) )
			{
				uint32_t const target = L.slast()[L.f_stretch()[path]];
				if ( target == pfirst || target == ln ) return false;
			}
		}
		return true;
	}

	// ================= combining a forward tree with a reverse block (score intervals) =================
	// capacities of this tier that rounds 1-4 had as globals (tier 0 trades them for nodes, round 5): stretches of a candidate, bytes of a decoded candidate's row
	enum : uint32_t { FSEQCAP = CT::seqcap, CONSROW = CT::consrow };
	static_assert(CONSROW <= FastLds<CT>::consmax && (CONSROW & 7u) == 0,"rows of the decoded candidates: read as 64 bit words");
	uint32_t cfree;   // free candidate sequence slots
	// A candidate is kept as its sequence of view stretches (forward chain, then reverse chain).  Within one view two
	// candidates spell the same string iff their sequences are equal (nodes are distinct k-mers and every edge lies on
	// exactly one stretch of the view), so the duplicate test of traverse (:5098-5110) compares sequences; strings are
	// decoded once, for the final candidates (decodePathPair :4267-4300).
	DEV uint32_t buildSeq(uint32_t const path, uint32_t const rp, LDSQ sid_t * dst, uint32_t & conslen)
	{
		uint32_t const nf = L.f_len()[path], nr = L.rc_len()[rp];
		if ( nf + nr > FSEQCAP ) { over(4096); return ~0u; }
		conslen = static_cast<uint32_t>(L.f_pos()[path]) + k + L.rc_pos()[rp];
		if ( conslen > CONSROW ) { over(4096); return ~0u; }
		// the two parent chains are walked in one loop, so that their dependent loads are in flight together (rc_len drops
		// by one per step and is zero at the root: the reverse chain has nr steps)
		uint32_t qf = path, qr = rp;
		uint32_t const ns = nf > nr ? nf : nr;
		for ( uint32_t t = 0; t < ns; ++t )
		{
			if ( t < nf ) { dst[nf-1-t] = L.f_stretch()[qf]; qf = L.f_parent()[qf]; }
			if ( t < nr ) { dst[nf+t] = L.rc_stretch()[qr]; qr = L.rc_parent()[qr]; }
		}
		return nf+nr;
	}
	DEV uint32_t decodeSeq(LDSQ sid_t const * seq, uint32_t const n, LDSQ uint8_t * dst) const
	{
		uint32_t o = 0;
		uint32_t const firstv = L.nv()[L.sfirst()[seq[0]]];
		for ( uint32_t i = 0; i < k; ++i ) dst[o++] = (firstv >> (2*(k-1-i))) & 3;
		for ( uint32_t ii = 0; ii < n; ++ii )
		{
			uint32_t const s = seq[ii]; LDSQ uint16_t const * Lk = L.links() + L.slink()[s];
			uint32_t const len = L.sslen()[s];
			for ( uint32_t j = 1; j < len; ++j ) dst[o++] = L.nv()[Lk[j]] & 3;
		}
		return o;
	}
	// matching interval [sub,sup) of popped path pi (junction k-mer `front`, candidate length candlen) in the sorted
	// reverse block and its heaviest entry (:4864-4950)
	DEV bool scoreInterval(uint32_t const sbase, uint32_t const nacc2, uint32_t const front, int64_t const candlen, int64_t const lmin, int64_t const lmax,
		uint32_t & sub, uint32_t & sup, uint32_t & mi) const
	{
		uint32_t lo = 0, hi = nacc2;
		while ( lo < hi ) { uint32_t const mid = (lo+hi)>>1; if ( L.rc_front()[sbase+mid] < front ) lo = mid+1; else hi = mid; }
		uint32_t e = lo;
		while ( e < nacc2 && L.rc_front()[sbase+e] == front ) ++e;
		if ( e == lo ) return false;
		int64_t bllo = lmin + static_cast<int64_t>(k) - candlen; if ( bllo < 0 ) bllo = 0;
		int64_t blhi = lmax + static_cast<int64_t>(k) - candlen; if ( blhi < 0 ) blhi = 0;
		uint32_t const bllo16 = static_cast<uint16_t>(bllo), blhi16 = static_cast<uint16_t>(blhi);
		sub = lo;
		while ( sub < e && L.rc_sbl()[sbase+sub] < bllo16 ) ++sub;
		sup = sub;
		while ( sup < e && !(blhi16 < L.rc_sbl()[sbase+sup]) ) ++sup;
		if ( sub == sup ) return false;
		mi = sub; uint32_t mr = L.rc_arw()[sbase+sub];
		for ( uint32_t i = sub+1; i < sup; ++i ) { uint32_t const r = L.rc_arw()[sbase+i]; if ( r > mr ) { mi = i; mr = r; } }
		return true;
	}
	// next lighter entry of a score interval (nextScoreInterval :3513-3534)
	DEV bool scoreNext(uint32_t const sbase, uint32_t const left, uint32_t const right, uint32_t const current, uint32_t & bi) const
	{
		uint32_t const v = L.rc_arw()[sbase+current];
		if ( !v ) return false;
		bool found = false; uint32_t bu = 0;
		for ( uint32_t i = left; i < right; ++i )
		{
			uint32_t const r = L.rc_arw()[sbase+i];
			if ( r <= v-1 && (!found || r > bu) ) { found = true; bu = r; bi = i; }
		}
		return found;
	}
	// one candidate offered to the candidate heap CDH (:5049-5092, including the shrink quirk); false: stop (error)
	//
	// Round 5: a candidate enters the heap as its pair of pool ids (forward path | reverse path << 16, flag UNMAT) and its stretch
	// sequence is written to a slot only if the candidate is still in the heap when its pools are about to be reused (materializeKept,
	// one lane per candidate, at the end of a batch of forward trees; materializeSerial after a pair on its exact stretch set).  The
	// duplicate test (:5077-5088: same string as the previous candidate kept of this pair <=> same stretch sequence) needs the two
	// sequences only when their stretch counts AND consensus lengths agree, both of which follow from the ids with four loads.
	// Rounds 1-4 walked the two parent chains of EVERY offered candidate on lane 0 (33 walks of 2 300 cycles per window of config 2,
	// 5.6 % of its time: site 6 of profiles/r05b_sites_cfg2_256piles_first_ledger.log) and copied the sequence twice.
	enum : uint32_t { UNMAT = 0x80000000u };
	uint32_t pvpath, pvrp, pvcl, pvnf;      // lane 0: the previous candidate kept of the current pair (pool ids, consensus length, stretches of its forward part); its stretch count is `pn`
	// Do (forward entry pa with na stretches, reverse entry ra) and (pb with nb, rb) spell the same stretch sequence, given equal
	// totals and na != nb?  The pool entries of an enumeration are the nodes of a tree (one entry per (parent, stretch)), so two
	// entries of one enumeration are equal sequences iff they are the same entry.  With na < nb = na + d the sequences are equal iff
	// pa is the d-th ancestor of pb, rb is the d-th ancestor of ra, and the d stretches in between agree: d steps along two parent
	// chains (d = distance of the two junctions, mostly 1) instead of both full chains.  Half of the offered candidates of config 2
	// are such duplicates -- the same chain met at a neighbouring junction k-mer.
	DEV bool seqEqual(uint32_t pa, uint32_t ra, uint32_t na, uint32_t pb, uint32_t rb, uint32_t nb)
	{
		if ( na > nb ) { uint32_t t = pa; pa = pb; pb = t; t = ra; ra = rb; rb = t; t = na; na = nb; nb = t; }
		uint32_t const d = nb - na;
		if ( static_cast<uint32_t>(L.rc_len()[ra]) < d ) return false;      // (equal totals: ra has d stretches more than rb)
		LDSQ sid_t * mid = L.cseq() + 16*FSEQCAP;      // the first d stretches of ra in candidate order
		uint32_t qr = ra;
		for ( uint32_t t = 0; t < d; ++t ) { mid[t] = L.rc_stretch()[qr]; qr = L.rc_parent()[qr]; }
		if ( qr != rb ) return false;
		uint32_t qf = pb;
		for ( uint32_t t = 0; t < d; ++t )
		{
			if ( L.f_stretch()[qf] != mid[d-1-t] ) return false;
			qf = L.f_parent()[qf];
		}
		return qf == pa;
	}
	DEV bool offerCandidate(uint64_t const weight, uint32_t const path, uint32_t const rp, uint32_t & pn)
	{
		FSTAT_ADD(18,1);
		SITE_T0
		if ( ncdh == 16 ) { uint32_t const to = L.cdh()[0].o, tl = L.cdh()[0].l; if ( !(tl & UNMAT) ) cfree |= 1u << to; spop<FCC,true>(L.cdh(),ncdh); SITE(5) }   // weight > top here
		uint32_t const nf = L.f_len()[path], nr = L.rc_len()[rp];
		uint32_t const conslen = static_cast<uint32_t>(L.f_pos()[path]) + k + L.rc_pos()[rp];
		if ( nf + nr > FSEQCAP || conslen > CONSROW ) { over(4096); return false; }      // (the checks of buildSeq, in its order)
		uint32_t const n = nf+nr;
		SITE(6)      // offerCandidate: stretch count and consensus length of the candidate
		// Within a pair both candidates come from one forward tree and one reverse enumeration, whose pool entries are the nodes of
		// a tree each: two entries of the same enumeration are different stretch sequences.  So equal strings need equal stretch counts
		// and consensus lengths, a different forward entry AND a different reverse entry, and forward parts of different lengths (the
		// same chain cut at another junction); half of the offers of config 2 pass the first two tests, hardly any all of them.
		if ( n == pn && conslen == pvcl && path != pvpath && rp != pvrp && nf != pvnf )
		{
			bool const same = seqEqual(path,rp,nf,pvpath,pvrp,pvnf);
			SITE(7)      // offerCandidate: comparison with the previous kept candidate (the stretches between the two junctions)
			if ( same ) return true;
		}
		pn = n; pvpath = path; pvrp = rp; pvcl = conslen; pvnf = nf;
		FCC cc; cc.w = weight; cc.o = path | (rp << 16); cc.l = n | (conslen<<8) | UNMAT;
		FSTAT_ADD(19,1);
		spush<FCC,true>(L.cdh(),ncdh,cc);
		SITE(8)      // offerCandidate: push
		return true;
	}
	// all lanes: the kept candidates that are still pool ids get a sequence slot each and their sequences, one lane per candidate
	DEV void materializeKept()
	{
		wv_sync();
		uint32_t const n = wv_bcast(ncdh,0);
		if ( !n ) return;
		uint32_t const cf = wv_bcast(cfree,0);
		uint32_t taken = 0, done = 0;
		for ( uint32_t c0 = 0; c0 < n; c0 += WSZ )
		{
			uint32_t const c = c0 + lane;
			FCC e; e.w = 0; e.o = 0; e.l = 0;
			if ( c < n ) e = ldget(L.cdh()+c);
			bool const um = c < n && (e.l & UNMAT) != 0;
			uint32_t tot; uint32_t const rank = done + wv_scan_flag(um,tot);
			done += tot;
			if ( um )
			{
				uint32_t m = cf; for ( uint32_t i = 0; i < rank; ++i ) m &= m-1;      // the rank-th free slot
				uint32_t const slot = __builtin_ctz(m);
				uint32_t cl;
				buildSeq(e.o & 0xFFFFu,e.o >> 16,L.cseq() + FSEQCAP*slot,cl);
				e.o = slot; e.l &= ~static_cast<uint32_t>(UNMAT); ldput(L.cdh()+c,e);
				taken |= 1u << slot;
			}
		}
		taken = wv_or(taken);
		if ( lane == 0 ) cfree &= ~taken;
		wv_sync();
	}
	// lane 0: the same for the candidates that name pool entries from slot f0 (forward) / r0 (reverse) on -- the enumerations of a
	// pair on its exact stretch set, whose pool space the next such pair reuses
	DEV void materializeSerial(uint32_t const f0, uint32_t const r0)
	{
		for ( uint32_t c = 0; c < ncdh; ++c )
		{
			uint32_t const l = L.cdh()[c].l;
			if ( !(l & UNMAT) ) continue;
			uint32_t const o = L.cdh()[c].o, pa = o & 0xFFFFu, ra = o >> 16;
			if ( pa < f0 && ra < r0 ) continue;
			uint32_t const slot = __builtin_ctz(cfree); cfree &= cfree-1;
			uint32_t cl;
			buildSeq(pa,ra,L.cseq() + FSEQCAP*slot,cl);
			L.cdh()[c].o = slot; L.cdh()[c].l = l & ~static_cast<uint32_t>(UNMAT);
		}
	}
	// serial form (lane 0): score intervals in the shared heap L.siq, candidates offered as they are popped
	// skip: that many pops have been offered already (recorded sequence of the lane form), pn: sequence length of the last
	// candidate kept from them
	DEV void combinePair(ChunkList<FNW> const & FC, uint32_t const nfpop, uint32_t const sbase, uint32_t const nacc2, uint64_t const rfm, int64_t const lmin, int64_t const lmax, uint32_t const maxfullpath,
		uint32_t const skip = 0, uint32_t pn = ~0u)
	{
		nsiq = 0;
		if ( !skip ) { pvpath = pvrp = pvnf = 0; pvcl = ~0u; }      // a pair of its own: no previous candidate
		for ( uint32_t pi = 0; pi < nfpop; ++pi )
		{
			uint32_t const o = clSlot<FCH>(FC,pi);
			uint32_t const front = L.fp_front()[o];
			if ( !((rfm >> (front & 63)) & 1) ) continue;   // no reverse path starts at this k-mer
			uint32_t sub, sup, mi;
			if ( scoreInterval(sbase,nacc2,front,static_cast<int64_t>(L.fp_cl()[o]) + k,lmin,lmax,sub,sup,mi) )
			{
				if ( nsiq >= CT::siqcap ) { over(512|0x40000); return; }
				FSI si; si.left = sub; si.right = sup; si.current = mi; si.path = pi; si.w = L.fp_adj()[o] + L.rc_w()[L.rc_ord()[sbase+mi]];
				spush<FSI,false>(L.siq(),nsiq,si);
			}
		}
		for ( uint32_t numfullpath = 0; nsiq && numfullpath < maxfullpath; ++numfullpath )
		{
			FSI const si = ldget(L.siq());
			// the score intervals leave the heap in non increasing weight order and everything still inside is not
			// heavier, so once the candidate heap is full and its top cannot be beaten, nothing of this pair can enter
			if ( numfullpath >= skip && ncdh == 16 && si.w <= L.cdh()[0].w ) break;
			spop<FSI,false>(L.siq(),nsiq);
			uint32_t bi;
			if ( scoreNext(sbase,si.left,si.right,si.current,bi) )
			{
				FSI sic = si; sic.current = bi; sic.w = L.fp_adj()[clSlot<FCH>(FC,si.path)] + L.rc_w()[L.rc_ord()[sbase+bi]];
				if ( nsiq >= CT::siqcap ) { over(512|0x40000); return; }
				spush<FSI,false>(L.siq(),nsiq,sic);
			}
			if ( numfullpath < skip ) continue;
			if ( !offerCandidate(si.w,L.fp_id()[clSlot<FCH>(FC,si.path)],L.rc_ord()[sbase+si.current],pn) ) return;
		}
	}
	// lane form: the same pops without the candidate heap; the (forward pool slot, reverse pool id) sequence goes to `out`
	// (at most 16 pairs of ids) and is offered to the candidate heap later, in pair order (replayPair).  The lane's heap holds the intervals
	// as (path, current, left, right); weights are recomputed from the tables.  Returns the count or 0xFF if the heap
	// is too small (the pair is then combined serially).
	struct PSI { id_t path, current, left, right; };
	// (round 4: 10 intervals per lane and 8 recorded pops per pair instead of 20 / 16, so that the same lane scratch and the same
	// record area serve 64 pairs per round instead of 32: a window has 96 pairs on average, its lanes are the pairs; 0.24 % of the
	// pairs have more than 10 matching intervals and are combined serially, a pair with more than 8 pops continues serially)
	enum { PSIQ = CT::psiq, POUTE = 8 };
	static constexpr id_t PSENT = static_cast<id_t>(~static_cast<id_t>(0));      // forward pop index no path has (8 bit ids: fewer than 255 pops per tree)
	static_assert(sizeof(id_t) > 1 || 8u*FNW*FCH < 255u,"the end mark of a lane's interval heap must not be a forward pop index");
	bool lscrdirty;      // lane 0: the lane scratch of the current round has been overwritten (an exact pair's enumerations, a serial combine)
	DEV uint64_t psiW(PSI const & e, ChunkList<FNW> const & FC, uint32_t const sbase) const { return L.fp_adj()[clSlot<FCH>(FC,e.path)] + L.rc_w()[L.rc_ord()[sbase+e.current]]; }
	DEV uint32_t combineLane(ChunkList<FNW> const & FC, uint32_t const nfpop, uint32_t const sbase, uint32_t const nacc2, uint64_t const rfm, int64_t const lmin, int64_t const lmax,
		uint32_t const maxfullpath, LDSQ PSI * H, LDSQ id_t * out, bool const prune, uint64_t const T0)
	{
		uint32_t n = 0;
		SITE_T0
		for ( uint32_t pi = 0; pi < nfpop; ++pi )
		{
			uint32_t const o = clSlot<FCH>(FC,pi);
			uint32_t const front = L.fp_front()[o];
			if ( !((rfm >> (front & 63)) & 1) ) continue;
			uint32_t sub, sup, mi;
			if ( scoreInterval(sbase,nacc2,front,static_cast<int64_t>(L.fp_cl()[o]) + k,lmin,lmax,sub,sup,mi) )
			{
				if ( n >= PSIQ || sup > 255 && sizeof(id_t) == 1 ) return 0xFF;
				PSI e; e.path = pi; e.current = mi; e.left = sub; e.right = sup;
				// FiniteSizeHeap push (max heap on the weight)
				uint32_t i = n++; H[i] = e;
				uint64_t const we = psiW(e,FC,sbase);
				while ( i )
				{
					uint32_t const p = (i-1)>>1;
					PSI const ep = H[p];
					if ( we > psiW(ep,FC,sbase) ) { H[i] = ep; H[p] = e; i = p; }
					else break;
				}
			}
		}
		FSTAT_ADD(25,1); FSTAT_ADD(26,n > 8 ? 1u : 0u); FSTAT_ADD(27,n > 10 ? 1u : 0u); FSTAT_ADD(28,n > 12 ? 1u : 0u); FSTAT_ADD(29,n > 16 ? 1u : 0u); FSTAT_MX(30,n);
		SITE(1)      // combineLane: the intervals of the pair (one scoreInterval per forward pop) and their heap
		return combineLanePops(FC,sbase,n,maxfullpath,H,out,prune,T0);
	}
	// the pops of the lane form on a heap of n intervals (second half of combineLane)
	DEV uint32_t combineLanePops(ChunkList<FNW> const & FC, uint32_t const sbase, uint32_t n, uint32_t const maxfullpath, LDSQ PSI * H, LDSQ id_t * out, bool const prune, uint64_t const T0)
	{
		SITE_T0
		uint32_t cnt = 0;
		for ( uint32_t numfullpath = 0; n && numfullpath < maxfullpath; ++numfullpath )
		{
			PSI const top = H[0];
			// the candidate heap was full with lightest weight T0 when the round began: as long as that still holds when
			// the pair is offered, nothing from here on can enter (replayRound checks it and continues serially otherwise)
			// (round 5: a cut pair leaves its heap behind -- the entry behind the last one marked -- and is continued from it, continueLane)
			if ( prune && psiW(top,FC,sbase) <= T0 ) { if ( n < PSIQ ) H[n].path = PSENT; return cnt | 0x20; }
			// the record of a pair holds POUTE pops: the rest of this pair's sequence is produced serially at its place in the pair order
			if ( cnt == POUTE ) { if ( n < PSIQ ) H[n].path = PSENT; return cnt | 0x10; }
			// pop
			{
				--n; PSI const last = H[n]; H[0] = last;
				uint32_t i = 0, r;
				while ( (r = 2*i+2) < n )
				{
					uint32_t const m = psiW(H[r-1],FC,sbase) > psiW(H[r],FC,sbase) ? (r-1) : r;
					PSI const em = H[m], ei = H[i];
					if ( psiW(ei,FC,sbase) > psiW(em,FC,sbase) ) break;
					H[i] = em; H[m] = ei; i = m;
				}
				if ( r >= n )
				{
					uint32_t const l = 2*i+1;
					if ( l < n ) { PSI const el = H[l], ei = H[i]; if ( !(psiW(ei,FC,sbase) > psiW(el,FC,sbase)) ) { H[i] = el; H[l] = ei; } }
				}
			}
			uint32_t bi;
			if ( scoreNext(sbase,top.left,top.right,top.current,bi) )
			{
				PSI e = top; e.current = bi;
				uint32_t i = n++; H[i] = e;
				uint64_t const we = psiW(e,FC,sbase);
				while ( i )
				{
					uint32_t const p = (i-1)>>1;
					PSI const ep = H[p];
					if ( we > psiW(ep,FC,sbase) ) { H[i] = ep; H[p] = e; i = p; }
					else break;
				}
			}
			out[2*cnt] = static_cast<id_t>(clSlot<FCH>(FC,top.path)); out[2*cnt+1] = L.rc_ord()[sbase+top.current]; ++cnt;
			SITE(2)      // combineLane: one pop (sift down, next lighter entry, push, record)
		}
		return cnt;
	}
	// Round 5: the interval construction of a round of pairs as a flat task list.  The lane form above walks a pair's forward pops and runs
	// scoreInterval for every pop whose junction k-mer (mod 64) the reverse block knows -- 64 lanes with different trees, different match
	// patterns and data dependent scan lengths, so the wavefront pays, iteration by iteration, for its slowest lane (site 1 of the ledger:
	// 6 % of a window).  Here a pair only LISTS its matching pops (matchPops: two loads per pop), the (pair, pop) matches of the whole
	// round become tasks dealt 64 at a time to the lanes (intervalTask: every lane runs one scoreInterval), and the pair then pushes its
	// valid intervals in pop order (heapOfList) -- the same pushes in the same order as before, hence the same heap.  A pair with more
	// than PSIQ matches, or a round with more tasks than the task list holds, takes the lane form as before.
	DEV uint32_t matchPops(ChunkList<FNW> const & FC, uint32_t const nfpop, uint64_t const rfm, LDSQ PSI * H) const
	{
		uint32_t nm = 0;
		for ( uint32_t pi = 0; pi < nfpop; ++pi )
		{
			uint32_t const front = L.fp_front()[clSlot<FCH>(FC,pi)];
			if ( !((rfm >> (front & 63)) & 1) ) continue;
			if ( nm < PSIQ ) H[nm].path = static_cast<id_t>(pi);
			++nm;
		}
		return nm;
	}
	// one (pair, matching pop) task: the pop's interval in the pair's reverse block, written over the list entry; false: the interval does
	// not fit an 8 bit id (the pair is combined serially, as in the lane form)
	DEV bool intervalTask(ChunkList<FNW> const & FC, uint32_t const sbase, uint32_t const nacc2, int64_t const lmin, int64_t const lmax, LDSQ PSI * e) const
	{
		uint32_t const pi = e->path;
		uint32_t const o = clSlot<FCH>(FC,pi);
		uint32_t sub, sup, mi;
		if ( scoreInterval(sbase,nacc2,L.fp_front()[o],static_cast<int64_t>(L.fp_cl()[o]) + k,lmin,lmax,sub,sup,mi) )
		{
			if ( sup > 255 && sizeof(id_t) == 1 ) return false;
			PSI v; v.path = static_cast<id_t>(pi); v.current = static_cast<id_t>(mi); v.left = static_cast<id_t>(sub); v.right = static_cast<id_t>(sup);
			*e = v;
		}
		else e->path = PSENT;
		return true;
	}
	// the valid entries of a pair's list, pushed in list (= pop) order: FiniteSizeHeap pushes as in combineLane; returns the heap's size
	DEV uint32_t heapOfList(ChunkList<FNW> const & FC, uint32_t const sbase, LDSQ PSI * H, uint32_t const nm) const
	{
		uint32_t n = 0;
		for ( uint32_t j = 0; j < nm; ++j )
		{
			PSI const e = H[j];
			if ( e.path == PSENT ) continue;
			uint32_t i = n++; H[i] = e;
			uint64_t const we = psiW(e,FC,sbase);
			while ( i )
			{
				uint32_t const p = (i-1)>>1;
				PSI const ep = H[p];
				if ( we > psiW(ep,FC,sbase) ) { H[i] = ep; H[p] = e; i = p; }
				else break;
			}
		}
		return n;
	}
	// offers the recorded sequence of a pair to the candidate heap, exactly as combinePair would have
	// returns true if the sequence was used up (false: ended at an entry that cannot enter the full heap, or error)
	DEV bool replayPair(ChunkList<FNW> const & FC, uint32_t const sbase, LDSQ id_t const * out, uint32_t const cnt, uint32_t & pn)
	{
		pn = ~0u; pvpath = pvrp = pvnf = 0; pvcl = ~0u;      // (dead between pairs: the compiler must not keep them alive across the enumerations)
		FSTAT_ADD(16,1); FSTAT_ADD(17,cnt);
		SITE_T0
		for ( uint32_t e = 0; e < cnt; ++e )
		{
			uint32_t const o = out[2*e];
			uint32_t const rp = out[2*e+1];
			uint64_t const w = L.fp_adj()[o] + L.rc_w()[rp];
			if ( ncdh == 16 && w <= L.cdh()[0].w ) { if ( e == 0 ) FSTAT_ADD(20,1); SITE(4) return false; }
			uint32_t const fid = L.fp_id()[o];
			SITE(4)      // replayPair: recorded entry -> weight, comparison with the lightest kept candidate
			if ( !offerCandidate(w,fid,rp,pn) ) return false;
			SITE_RESET
		}
		return true;
	}

	// lane 0: a pair whose recorded sequence was cut (record full, or pruned at a weight that no longer prunes) goes on from the heap
	// its lane left behind in the lane scratch -- the state combinePair would reach by building every interval again and popping `cnt`
	// times (same heap mechanics: FiniteSizeHeap push / pop on the same weights).  Rounds 1-4 did exactly that: 43 k cycles per
	// continued pair, 0.7 of them per window of config 2 (site 9 of the ledger).
	DEV void continueLane(ChunkList<FNW> const & FC, uint32_t const sbase, LDSQ PSI * H, uint32_t const cnt, uint32_t pn)
	{
		uint32_t n = 0;
		while ( n < PSIQ && H[n].path != PSENT ) ++n;
		for ( uint32_t numfullpath = cnt; n && numfullpath < 16; ++numfullpath )
		{
			PSI const top = H[0];
			uint64_t const wtop = psiW(top,FC,sbase);
			if ( ncdh == 16 && wtop <= L.cdh()[0].w ) break;
			{
				--n; PSI const last = H[n]; H[0] = last;
				uint32_t i = 0, r;
				while ( (r = 2*i+2) < n )
				{
					uint32_t const m = psiW(H[r-1],FC,sbase) > psiW(H[r],FC,sbase) ? (r-1) : r;
					PSI const em = H[m], ei = H[i];
					if ( psiW(ei,FC,sbase) > psiW(em,FC,sbase) ) break;
					H[i] = em; H[m] = ei; i = m;
				}
				if ( r >= n )
				{
					uint32_t const l = 2*i+1;
					if ( l < n ) { PSI const el = H[l], ei = H[i]; if ( !(psiW(ei,FC,sbase) > psiW(el,FC,sbase)) ) { H[i] = el; H[l] = ei; } }
				}
			}
			uint32_t bi;
			if ( scoreNext(sbase,top.left,top.right,top.current,bi) )
			{
				PSI e = top; e.current = bi;
				uint32_t i = n++; H[i] = e;
				uint64_t const we = psiW(e,FC,sbase);
				while ( i )
				{
					uint32_t const p = (i-1)>>1;
					PSI const ep = H[p];
					if ( we > psiW(ep,FC,sbase) ) { H[i] = ep; H[p] = e; i = p; }
					else break;
				}
			}
			if ( !offerCandidate(wtop,L.fp_id()[clSlot<FCH>(FC,top.path)],L.rc_ord()[sbase+top.current],pn) ) return;
		}
	}

	// text: 8 byte aligned, readable up to the next multiple of 8 behind n (a row of consL).  The pattern masks and the
	// text (eight symbols per load) are fetched up front, so the column loop runs from registers.
	DEV uint32_t myersDistance(uint32_t const j, LDSQ uint8_t const * text, uint32_t const n) const
	{
		uint32_t const m = L.slen()[j];
		if ( m == 0 ) return n;
		if constexpr ( FastLds<CT>::pw > 2 ) return myersDistanceN(j,text,n,m);
		else {
		if ( FastLds<CT>::pw == 2 ) return myersDistance2(j,text,n,m);
		LDSQ uint64_t const * PEQ = L.peq() + 4*j;
		uint64_t const e0 = PEQ[0], e1 = PEQ[1], e2 = PEQ[2], e3 = PEQ[3];
		LDSQ uint64_t const * T8 = reinterpret_cast<LDSQ uint64_t const *>(text);
		uint32_t score = m;
		uint64_t Pv = ~0ull, Mv = 0;
		uint64_t const top = 1ull<<(m-1);
		uint64_t w = n ? T8[0] : 0ull;
		for ( uint32_t c0 = 0; c0 < n; c0 += 8 )
		{
			uint64_t const wn = (c0+8 < n) ? T8[(c0>>3)+1] : 0ull;      // next word, in flight during these eight columns
			uint32_t const cnt = (n-c0 < 8) ? (n-c0) : 8u;
			for ( uint32_t u = 0; u < cnt; ++u )
			{
				uint32_t const ch = static_cast<uint32_t>(w >> (8*u)) & 3u;
				uint64_t const Eq = (ch & 2) ? ((ch & 1) ? e3 : e2) : ((ch & 1) ? e1 : e0);
				uint64_t const Xv = Eq | Mv;
				uint64_t const Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
				uint64_t Ph = Mv | ~(Xh | Pv);
				uint64_t Mh = Pv & Xh;
				if ( Ph & top ) ++score; else if ( Mh & top ) --score;
				Ph = (Ph<<1) | 1ull; Mh <<= 1;
				Pv = Mh | ~(Xv | Ph);
				Mv = Ph & Xv;
			}
			w = wn;
		}
		return score;
		}
	}
	// the same for strings of up to 128 bases (tier 5): two words per pattern mask, block-wise Myers (the horizontal deltas
	// of the top row of word 0 are the carries into word 1), the score follows bit m-1
	DEV uint32_t myersDistance2(uint32_t const j, LDSQ uint8_t const * text, uint32_t const n, uint32_t const m) const
	{
		LDSQ uint64_t const * PEQ = L.peq() + 8*j;
		uint64_t const a0 = PEQ[0], a1 = PEQ[1], c0_ = PEQ[2], c1_ = PEQ[3], g0 = PEQ[4], g1 = PEQ[5], t0 = PEQ[6], t1 = PEQ[7];
		LDSQ uint64_t const * T8 = reinterpret_cast<LDSQ uint64_t const *>(text);
		bool const two = m > 64;
		uint64_t const top = two ? (1ull<<(m-65)) : (1ull<<(m-1));
		uint32_t score = m;
		uint64_t Pv0 = ~0ull, Mv0 = 0, Pv1 = ~0ull, Mv1 = 0;
		uint64_t w = n ? T8[0] : 0ull;
		for ( uint32_t c0 = 0; c0 < n; c0 += 8 )
		{
			uint64_t const wn = (c0+8 < n) ? T8[(c0>>3)+1] : 0ull;
			uint32_t const cnt = (n-c0 < 8) ? (n-c0) : 8u;
			for ( uint32_t u = 0; u < cnt; ++u )
			{
				uint32_t const ch = static_cast<uint32_t>(w >> (8*u)) & 3u;
				uint64_t const Eq0 = (ch & 2) ? ((ch & 1) ? t0 : g0) : ((ch & 1) ? c0_ : a0);
				uint64_t const Eq1 = (ch & 2) ? ((ch & 1) ? t1 : g1) : ((ch & 1) ? c1_ : a1);
				uint64_t const Xv0 = Eq0 | Mv0;
				uint64_t const Xh0 = (((Eq0 & Pv0) + Pv0) ^ Pv0) | Eq0;
				uint64_t Ph0 = Mv0 | ~(Xh0 | Pv0);
				uint64_t Mh0 = Pv0 & Xh0;
				uint64_t const phc = Ph0>>63, mhc = Mh0>>63;
				if ( !two ) { if ( Ph0 & top ) ++score; else if ( Mh0 & top ) --score; }
				Ph0 = (Ph0<<1) | 1ull; Mh0 <<= 1;
				Pv0 = Mh0 | ~(Xv0 | Ph0);
				Mv0 = Ph0 & Xv0;
				if ( two )
				{
					uint64_t const Eq1c = Eq1 | mhc;
					uint64_t const Xv1 = Eq1 | Mv1;
					uint64_t const Xh1 = (((Eq1c & Pv1) + Pv1) ^ Pv1) | Eq1c;
					uint64_t Ph1 = Mv1 | ~(Xh1 | Pv1);
					uint64_t Mh1 = Pv1 & Xh1;
					if ( Ph1 & top ) ++score; else if ( Mh1 & top ) --score;
					Ph1 = (Ph1<<1) | phc; Mh1 = (Mh1<<1) | mhc;
					Pv1 = Mh1 | ~(Xv1 | Ph1);
					Mv1 = Ph1 & Xv1;
				}
			}
			w = wn;
		}
		return score;
	}
	// the same for strings of up to 255 bases (tier 17): PW words per pattern mask, block-wise Myers over the nb = ceil(m/64) words the string has (the
	// words above its last one do no work), the horizontal deltas of the top row of a word are the carries into the next one, the score follows bit
	// (m-1) & 63 of word (m-1) >> 6.  The masks of a symbol are picked by mask arithmetic (as k_trace_wide does), not by an indexed select: the 16 mask
	// words and the 8 state words stay in registers
	DEV uint32_t myersDistanceN(uint32_t const j, LDSQ uint8_t const * text, uint32_t const n, uint32_t const m) const
	{
		enum { PW = FastLds<CT>::pw };
		LDSQ uint64_t const * PEQ = L.peq() + 4*PW*j;
		uint64_t E0[PW], E1[PW], E2[PW], E3[PW], Pv[PW], Mv[PW];
		#pragma unroll
		for ( uint32_t b = 0; b < PW; ++b ) { E0[b] = PEQ[b]; E1[b] = PEQ[PW+b]; E2[b] = PEQ[2*PW+b]; E3[b] = PEQ[3*PW+b]; Pv[b] = ~0ull; Mv[b] = 0; }
		LDSQ uint64_t const * T8 = reinterpret_cast<LDSQ uint64_t const *>(text);
		uint32_t const lastw = (m-1) >> 6;
		uint64_t const top = 1ull << ((m-1) & 63u);
		uint32_t score = m;
		uint64_t w = n ? T8[0] : 0ull;
		for ( uint32_t c0 = 0; c0 < n; c0 += 8 )
		{
			uint64_t const wn = (c0+8 < n) ? T8[(c0>>3)+1] : 0ull;
			uint32_t const cnt = (n-c0 < 8) ? (n-c0) : 8u;
			for ( uint32_t u = 0; u < cnt; ++u )
			{
				uint32_t const ch = static_cast<uint32_t>(w >> (8*u)) & 3u;
				uint64_t const s0 = ch == 0 ? ~0ull : 0ull, s1 = ch == 1 ? ~0ull : 0ull, s2 = ch == 2 ? ~0ull : 0ull, s3 = ch == 3 ? ~0ull : 0ull;
				uint64_t phc = 1ull, mhc = 0ull;      // the delta entering row 0: +1 (the first row of the matrix is 0, 1, 2, ...: a global distance)
				#pragma unroll
				for ( uint32_t b = 0; b < PW; ++b )
					if ( b <= lastw )
					{
						uint64_t const Eq = (E0[b] & s0) | (E1[b] & s1) | (E2[b] & s2) | (E3[b] & s3);
						uint64_t const Eqc = Eq | mhc;
						uint64_t const Xv = Eq | Mv[b];
						uint64_t const Xh = (((Eqc & Pv[b]) + Pv[b]) ^ Pv[b]) | Eqc;
						uint64_t Ph = Mv[b] | ~(Xh | Pv[b]);
						uint64_t Mh = Pv[b] & Xh;
						if ( b == lastw ) { if ( Ph & top ) ++score; else if ( Mh & top ) --score; }
						uint64_t const pho = Ph>>63, mho = Mh>>63;
						Ph = (Ph<<1) | phc; Mh = (Mh<<1) | mhc;
						Pv[b] = Mh | ~(Xv | Ph);
						Mv[b] = Ph & Xv;
						phc = pho; mhc = mho;
					}
			}
			w = wn;
		}
		return score;
	}
	DEV void buildPeq()
	{
		if constexpr ( GW ) return;      // the gather built them
		else
		for ( uint32_t j = lane; j < mao; j += WSZ )
		{
			uint32_t const m = L.slen()[j];
			LDSQ uint8_t const * s = L.str() + j*CT::lstr;
			enum { PW = FastLds<CT>::pw };
			#pragma unroll
			for ( uint32_t wq = 0; wq < PW; ++wq )
			{
				uint64_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
				uint32_t const lo = 64*wq, hi = m < lo+64 ? m : lo+64;
				for ( uint32_t i = lo; i < hi; ++i )
				{
					uint32_t const c = s[i]; uint64_t const b = 1ull<<(i-lo);
					e0 |= (c == 0) ? b : 0; e1 |= (c == 1) ? b : 0; e2 |= (c == 2) ? b : 0; e3 |= (c == 3) ? b : 0;
				}
				L.peq()[4*PW*j+0*PW+wq] = e0; L.peq()[4*PW*j+1*PW+wq] = e1; L.peq()[4*PW*j+2*PW+wq] = e2; L.peq()[4*PW*j+3*PW+wq] = e3;
			}
		}
		wv_sync();
	}

	// gw layout: the enumeration pools lie over the build-phase arrays (region S); S goes to the workgroup's global slab
	// before the enumerations and comes back after the pairs (candidate errors need the pattern masks, the next
	// activation state the successor tables, the next traversal all of it)
	// Only the part of S the pools cover is copied.  The spilled image stays valid for the following traversals of the same
	// pass (only the successor flags change between them, addNextFromHeap): sfresh = the build phase has rewritten S,
	// sdirty = the successor flags have changed since the last spill.
	bool sfresh, sdirty;
	DEV void spillS()
	{
		if constexpr ( GW )
		{
			typedef FastLds<CT> LL;
			constexpr uint32_t plen = ((LL::upool - LL::sbase + 15u) & ~15u) < LL::sbytes ? ((LL::upool - LL::sbase + 15u) & ~15u) : LL::sbytes;
			constexpr uint32_t si0 = (LL::o_sinfo - LL::sbase) & ~15u, si1 = ((LL::e_sinfo - LL::sbase + 15u) & ~15u) < plen ? ((LL::e_sinfo - LL::sbase + 15u) & ~15u) : plen;
			LDSQ G4 const * const src = reinterpret_cast<LDSQ G4 const *>(L.base + LL::sbase);
			G4 * const dst = reinterpret_cast<G4 *>(gslab + LL::g_spill);
			wv_sync();
			if ( sfresh ) { for ( uint32_t i = lane; i < plen/16u; i += WSZ ) dst[i] = src[i]; }
			else if ( sdirty && si0 < si1 ) { for ( uint32_t i = si0/16u + lane; i < si1/16u; i += WSZ ) dst[i] = src[i]; }
			sfresh = false; sdirty = false;
			wv_sync();
		}
	}
	// sorted k-mer instances + last k-mer list of the current k <-> the workgroup's slab (gw tiers).  A pass that ran a
	// traversal has overwritten overlay A; the next filter frequency pass of the same k needs the very same arrays.
	DEV void saveInstances()
	{
		if constexpr ( GW )
		{
			typedef FastLds<CT> LL;
			G4 * const dst = reinterpret_cast<G4 *>(gslab + LL::g_inst);
			LDSQ G4 const * const sp = reinterpret_cast<LDSQ G4 const *>(L.pre());
			LDSQ G4 const * const sl = reinterpret_cast<LDSQ G4 const *>(L.lastk());
			for ( uint32_t i = lane; i < (npre+1)/2; i += WSZ ) dst[i] = sp[i];
			for ( uint32_t i = lane; i < (nlast+1)/2; i += WSZ ) dst[FastLds<CT>::icap/2 + i] = sl[i];
		}
	}
	// hand-over slots (FastBatch::hand): slot = number + 1, 0 = none.  A window keeps its slot from tier to tier (the instances of a k
	// do not change), so only the first hand-over writes.
	DEV uint32_t saveHand(FastBatch const & FB, uint32_t hslot)
	{
		if ( hslot ) return hslot;
		if ( npre + 2u*((nlast+1)/2) + 4u > FB.handwords || npre > FB.handwords ) return 0;
		uint32_t sl = 0;
		if ( lane == 0 ) { uint32_t const q = wv_atomic_add_global(FB.handctr,1u); sl = q < FB.handcap ? q+1 : 0u; }
		sl = wv_bcast(sl,0);
		if ( !sl ) return 0;
		uint64_t * const dst = FB.hand + static_cast<uint64_t>(sl-1)*FB.handwords;
		if ( lane == 0 ) { dst[0] = npre | (static_cast<uint64_t>(nlast)<<32); dst[1] = k; }
		uint32_t const po = 2, lo = 2 + ((npre+1)&~1u);
		for ( uint32_t i = lane; i < npre; i += WSZ ) dst[po+i] = L.pre()[i];
		for ( uint32_t i = lane; i < nlast; i += WSZ ) dst[lo+i] = L.lastk()[i];
		return sl;
	}
	DEV bool loadHand(FastBatch const & FB, uint32_t const hslot)
	{
		uint64_t const * const src = FB.hand + static_cast<uint64_t>(hslot-1)*FB.handwords;
		uint64_t const h0 = src[0];
		uint32_t const n = static_cast<uint32_t>(h0), nl = static_cast<uint32_t>(h0>>32);
		if ( n > FastLds<CT>::icap || nl > FastLds<CT>::keycap || src[1] != k ) return false;      // (cannot happen between the tiers of one batch)
		npre = n; nlast = nl;
		FSTAT_ADD(31,1);
		uint32_t const po = 2, lo = 2 + ((n+1)&~1u);
		wv_sync();
		for ( uint32_t i = lane; i < n; i += WSZ ) L.pre()[i] = src[po+i];
		for ( uint32_t i = lane; i < nl; i += WSZ ) L.lastk()[i] = src[lo+i];
		wv_sync();
		return true;
	}
	DEV void restoreInstances()
	{
		if constexpr ( GW )
		{
			typedef FastLds<CT> LL;
			G4 const * const src = reinterpret_cast<G4 const *>(gslab + LL::g_inst);
			LDSQ G4 * const dp = reinterpret_cast<LDSQ G4 *>(L.pre());
			LDSQ G4 * const dl = reinterpret_cast<LDSQ G4 *>(L.lastk());
			wv_sync();
			for ( uint32_t i = lane; i < (npre+1)/2; i += WSZ ) dp[i] = src[i];
			for ( uint32_t i = lane; i < (nlast+1)/2; i += WSZ ) dl[i] = src[FastLds<CT>::icap/2 + i];
			wv_sync();
		}
	}
	DEV void restoreS()
	{
		if constexpr ( GW )
		{
			typedef FastLds<CT> LL;
			constexpr uint32_t plen = ((LL::upool - LL::sbase + 15u) & ~15u) < LL::sbytes ? ((LL::upool - LL::sbase + 15u) & ~15u) : LL::sbytes;
			LDSQ G4 * const dst = reinterpret_cast<LDSQ G4 *>(L.base + LL::sbase);
			G4 const * const src = reinterpret_cast<G4 const *>(gslab + LL::g_spill);
			wv_sync();
			for ( uint32_t i = lane; i < plen/16u; i += WSZ ) dst[i] = src[i];
			wv_sync();
		}
	}

	// ================= traverse (:4496-5170) for one activation state =================
	// (first, last) candidate pairs: the reverse blocks of all last k-mers and the forward trees of a batch of first
	// k-mers are enumerated with one lane each, the score intervals of NPL pairs at a time are popped with one lane per
	// pair into recorded (path, entry) sequences, and lane 0 offers those to the candidate heap in the reference's pair
	// order.  A pair whose cached enumerations may be touched by the other k-mer's split (rare) is enumerated on its
	// exact stretch set by lane 0 at its place in that order.
	enum { NPL = 64, RPSTL = 32, PM_SKIP = 0xF0, PM_SERIAL = 0xF1, PM_EXACT = 0xE0, PM_PEND = 0x80 };      // (PM_PEND | matches: between the phases of a round only)
	static_assert(sizeof(PSI)*PSIQ*NPL <= FastLds<CT>::lscrbytes && 2u*POUTE*NPL <= 32u*32u,"score interval heaps and pop records of a round of pairs");
	enum : uint32_t { MIDCAP = 8 };
	uint32_t nmid, midbase;              // middle pieces of this activation state: pool ids midbase .. midbase+nmid-1
	// pair p of a batch -> (first k-mer candidate p / nL, last k-mer candidate p % nL): one multiplication by ceil(2^32 / nL) (exact while
	// p * nL < 2^32) instead of a 32 bit division -- some 25 VALU instructions -- per pair and phase, and per live pair on lane 0
	uint32_t nLmagic;
	DEV void pairFL(uint32_t const p, uint32_t & f, uint32_t & l) const
	{
		if ( nL <= 1 ) { f = p; l = 0; }
		else
		{
#if defined(DACC_EMUL)
			f = static_cast<uint32_t>((static_cast<uint64_t>(p) * nLmagic) >> 32);
#else
			f = __umulhi(p,nLmagic);
#endif
			l = p - f*nL;
		}
	}
	uint32_t rstop;                      // sorted reverse entries used by the cached blocks
	uint64_t roundT0;                    // lightest weight of the (full) candidate heap when the current round of pairs began
	uint32_t nsiq, ncdh, nacc;

	DEV void viewOfLast(View & V, uint32_t const li) const
	{
		viewClear(V);
		uint32_t const sl = L.parL()[li];
		if ( sl != SNONE ) { viewRemove(V,sl); viewAdd(V,L.pieL()[li]); viewAdd(V,L.pieL()[li]+1); }
	}
	DEV void viewOfFirst(View & V, uint32_t const fi) const
	{
		viewClear(V);
		uint32_t const sf = L.parF()[fi];
		if ( sf != SNONE ) { viewRemove(V,sf); viewAdd(V,L.pieF()[fi]); viewAdd(V,L.pieF()[fi]+1); }
	}
	// are the cached enumerations of (fi, li) valid for the pair?  bit 0: reverse block, bit 1: forward tree, bit 2: both
	// candidates split the same stretch
	DEV uint32_t classifyPair(uint32_t const fi, uint32_t const li, int64_t const lmax) const
	{
		uint32_t const sf = L.parF()[fi], sl = L.parL()[li];
		if ( sf != SNONE && sf == sl ) return 4;
		int32_t const firstnode = L.fnode()[fi] == 0xFFFF ? -1 : L.fnode()[fi];
		int32_t const lastnode = L.lnode()[li] == 0xFFFF ? -1 : L.lnode()[li];
		bool rcached, fcached;
		if ( sf == SNONE ) rcached = true;
		else
		{
			uint64_t const tm = L.rtmask()[li];
			uint32_t const fn = L.fnode()[fi];
			rcached = !((tm >> (L.slast()[sf]&63))&1) && !((tm >> (fn&63))&1);
			if ( !rcached ) rcached = reverseUnaffected(L.rbase()[li],L.rn()[li],lastnode,sf,fn,lmax);
		}
		if ( sl == SNONE ) fcached = true;
		else
		{
			uint64_t const tm = L.ftm()[fi];
			fcached = !((tm >> (L.sfirst()[sl]&63))&1) && !((tm >> (L.lnode()[li]&63))&1);
			if ( !fcached ) { ChunkList<FNW> FC; forwardTreeLoad(FC,fi); fcached = forwardUnaffected(FC,L.fnp()[fi],firstnode,sl,L.lnode()[li],lmax); }
		}
		return (rcached ? 1u : 0u) | (fcached ? 2u : 0u);
	}
	// lane 0: pairs [q, n) of the round starting at pair p0 of the batch that starts at candidate fstart, in order.
	// returns 0 when the round is done,
	// 2 when the forward tree of the exact pair q found no pool space next to the trees of the batch (alone: the batch
	// holds the tree of this first k-mer only)
	// live: bit q set for the pairs of the round that are not PM_SKIP (most pairs share no junction k-mer and are skipped:
	// lane 0 walks the set bits instead of reading every pair's mode)
	DEV uint32_t replayRound(uint32_t & q, uint32_t const n, uint32_t const p0, uint32_t const fstart, int64_t const lmin, int64_t const lmax, bool const alone, uint64_t const live)
	{
		for ( ; q < n; ++q )
		{
			uint64_t const rest = live >> q;
			if ( !rest ) { q = n; break; }
			q += static_cast<uint32_t>(__builtin_ctzll(rest));
			SITE_T0
			uint32_t const mode = L.poutn()[q];
			FSTAT_ADD(13,1);
			if ( mode == PM_SKIP ) { FSTAT_ADD(14,1); continue; }
			uint32_t const p = p0+q;
			uint32_t fi, li; pairFL(p,fi,li); fi += fstart;
			if ( mode < 0x40 || mode == PM_SERIAL )
			{
				// no candidate of this pair can beat the lightest kept candidate: score <= path weight + reverse weight
				if ( ncdh == 16 && L.fmx()[fi] + L.rmaxw()[li] <= L.cdh()[0].w ) { FSTAT_ADD(15,1); SITE(3) continue; }
				ChunkList<FNW> FC; forwardTreeLoad(FC,fi);
				SITE(3)      // replayRound: per live pair, up to the dispatch on its mode
				if ( mode < 0x40 )
				{
					uint32_t const cnt = mode & 0x0F; uint32_t pn;
					bool const used = replayPair(FC,L.rbase()[li],L.pout() + 2*POUTE*q,cnt,pn);
					if ( flags ) return 0;
					SITE_RESET
					// a sequence cut at weight T0 (0x20) is complete only while the candidate heap is full with a top of at least T0; one
					// cut because the record was full (0x10) always goes on
					if ( used && ( (mode & 0x10) || ((mode & 0x20) && !(ncdh == 16 && L.cdh()[0].w >= roundT0)) ) )
					{
						pcount(21,1);
						if ( !lscrdirty ) continueLane(FC,L.rbase()[li],reinterpret_cast<LDSQ PSI *>(L.lscr()) + PSIQ*q,cnt,pn);
						else combinePair(FC,L.fnp()[fi],L.rbase()[li],L.rn()[li],L.rfmask()[li],lmin,lmax,16,cnt,pn);
						SITE(9)      // replayRound: continuation of a cut sequence (from the lane's heap; combinePair with skip if the scratch is gone)
					}
				}
				else { pcount(23,1); lscrdirty = true; combinePair(FC,L.fnp()[fi],L.rbase()[li],L.rn()[li],L.rfmask()[li],lmin,lmax,16); SITE(9) }
				if ( flags ) return 0;
				continue;
			}
			// exact stretch set of the pair (split at first, then at last)
			pcount(22,1);
			lscrdirty = true;      // (its enumerations and its serial combine use the lane scratch)
			bool const rcached = mode & 1, fcached = mode & 2, same = mode & 4;
			uint32_t const sf = L.parF()[fi], sl = L.parL()[li];
			int32_t const firstnode = L.fnode()[fi] == 0xFFFF ? -1 : L.fnode()[fi];
			int32_t const lastnode = L.lnode()[li] == 0xFFFF ? -1 : L.lnode()[li];
			View V; viewClear(V);
			if ( same )
			{
				uint32_t const pf = L.posF()[fi], pl = L.posL()[li];
				viewRemove(V,sf);
				if ( pf == pl ) { viewAdd(V,L.pieF()[fi]); viewAdd(V,L.pieF()[fi]+1); }
				else
				{
					// the middle piece of this pair is in the pool (findCandidatesAndPieces)
					uint32_t const lo = pf < pl ? pf : pl, hi = pf < pl ? pl : pf;
					uint32_t m = 0;
					while ( m+1 < nmid && !(L.midpar()[m] == sf && L.midA()[m] == lo && L.midB()[m] == hi) ) ++m;
					if ( pf < pl ) { viewAdd(V,L.pieF()[fi]); viewAdd(V,L.pieL()[li]+1); } else { viewAdd(V,L.pieL()[li]); viewAdd(V,L.pieF()[fi]+1); }
					viewAdd(V,midbase+m);
				}
			}
			else
			{
				if ( sf != SNONE ) { viewRemove(V,sf); viewAdd(V,L.pieF()[fi]); viewAdd(V,L.pieF()[fi]+1); }
				if ( sl != SNONE ) { viewRemove(V,sl); viewAdd(V,L.pieL()[li]); viewAdd(V,L.pieL()[li]+1); }
			}
			uint32_t const rsave = L.ctr()[0], fsave = L.ctr()[1];
			uint32_t sbase = L.rbase()[li], nacc2 = L.rn()[li]; uint64_t rfm = L.rfmask()[li];
			if ( !rcached )
			{
				REnum RX;
				reverseEnumerateLane(RX,L.rchx(),V,L.lkmer()[li],lastnode,lmax,reinterpret_cast<LDSQ id_t *>(L.lscr()),FastLds<CT>::lscrbytes/sizeof(id_t));
				if ( flags ) return 0;
				if ( rstop + RX.narp > CT::rccap ) { over(512|0x4000); return 0; }
				reverseBlockCopy(RX,rstop);
				reverseBlockFinish(RX,rstop,FNC,lastnode,lmax);
				if ( flags ) return 0;
				sbase = rstop; nacc2 = RX.narp; rfm = L.rfmask()[FNC];
			}
			ChunkList<FNW> FC; uint32_t nfp; uint64_t ffmx;
			if ( !fcached )
			{
				FEnum FX;
				forwardEnumerateLane(FX,L.fchb() + 8*FNW*FNC,V,firstnode,lmax,reinterpret_cast<LDSQ id_t *>(L.lscr()));
				if ( flags == (512|0x10000) && FX.np < 8*FNW*FCH && !alone )
				{
					// the trees of the batch leave no room for this one: the batch is cut here and continues with the tree
					// of this first k-mer alone in the pool
					flags = 0; L.ctr()[0] = rsave; L.ctr()[1] = fsave;
					return 2;
				}
				if ( flags ) return 0;
				FC = FX.C; nfp = FX.nfpop; ffmx = FX.ffm;
			}
			else { forwardTreeLoad(FC,fi); nfp = L.fnp()[fi]; ffmx = L.ffm()[fi]; }
			if ( rfm & ffmx ) combinePair(FC,nfp,sbase,nacc2,rfm,lmin,lmax,16);   // else: no junction k-mer in common
			if ( !flags && (!rcached || !fcached) ) materializeSerial(fcached ? ~0u : fsave*FCH,rcached ? ~0u : rsave*RCH);      // candidates that name this pair's own enumerations
			L.ctr()[0] = rsave; L.ctr()[1] = fsave;
			SITE(10)      // replayRound: a pair on its exact stretch set (enumerations + serial combine)
			if ( flags ) return 0;
		}
		return 0;
	}

	DEV bool traverse(int64_t const lmin, int64_t const lmax)
	{
		PROF_T0
		cfree = 0xFFFFu; ncdh = 0; nacc = 0; nwF = 0; nwR = 0; nsiq = 0; pvpath = pvrp = pvnf = 0; pvcl = ~0u;
		LEDGER_REP(5) computeBaseStretches();
		flags = wv_or(flags); if ( flags ) return false;
		PROF(*this,8)
		LEDGER_REP(6) findCandidatesAndPieces();
		flags = wv_or(flags); if ( flags ) return false;
		nLmagic = nL > 1 ? static_cast<uint32_t>(((1ull<<32) + nL - 1u) / nL) : 0u;
#if !defined(DACC_NO_REACH)
		{
			SITE_T0
			bool reach = false;
			LEDGER_REP(7) reach = pairReachable();
			SITE(23)      // traverse: reachability prune
			if ( !reach ) { FSTAT_ADD(23,1); PROF(*this,16) return false; }
		}
#endif
		// what only a state with a first -> last walk reads: the by-first / by-last lookups of the base stretches, the pieces and their positions
		// (every over() check of the two functions stands in front of the reachability test, so flags and the tier that finishes a window are
		// what they were; the lookups' sort key area and the pieces lie outside the weight arrays the test borrows)
		computeStretchLookups();
		makePieces();
		PROF(*this,16)
		loadTab();
		PROF(*this,17)
		// (the distances are part of the phase: its second run in a ledger build finds their bytes overwritten)
		LEDGER_REP(8) { nwF = 0; nwR = 0; bool const need = feasNeedOn(); if ( need ) feasDistances(); computeStretchFeasLanes(0,npool,lmax,need); }
		flags = wv_or(flags); if ( flags ) return false;
#if defined(DACC_EMUL)
		// the traversal trace (DACC_EMUL_TRAV) describes the unfiltered computation, as it did before there was a filter: where the filtered
		// pass stood, its numbers of weight records come from a second pass that only counts (its task lists are scratch the first pass is
		// done with; it writes no mask, offset or record and cannot overflow: the bound of the set-up held)
		nwFall = nwF; nwRall = nwR;
		if ( ftrav_file() && feasapplied )
		{
			uint32_t const kF = nwF, kR = nwR;
			feascount = true; nwF = 0; nwR = 0; computeStretchFeasLanes(0,npool,lmax,false); feascount = false;
			nwFall = nwF; nwRall = nwR; nwF = kF; nwR = kR;
		}
#endif
		{ SITE_T0 bool const sf0_ = sfresh, sd0_ = sdirty; LEDGER_REP(9) { sfresh = sf0_; sdirty = sd0_; spillS(); } SITE(24) }      // traverse: build-phase arrays to the slab
		PROF(*this,9)

		// ---- reverse blocks of all last k-mer candidates, lane = candidate ----
		LEDGER_REP(10)
		{
		if ( lane == 0 ) { L.ctr()[0] = 0; L.ctr()[1] = 0; }
		wv_sync();
		{
			uint32_t sb = 0;
			for ( uint32_t c = 0; c < nL; c += WSZ )
			{
				uint32_t const li = c + lane;
				bool const ract = li < nL;
				REnum R; clInit(R.C,L.rchb() + 8*RNW*lane); R.nrp = 0; R.narp = 0; R.lastk = 0;
				int32_t lastnode = -1;
				View V; viewClear(V);
				bool rover = false;
				if ( ract )
				{
					viewOfLast(V,li);
					lastnode = L.lnode()[li] == 0xFFFF ? -1 : L.lnode()[li];
					reverseEnumerateLane(R,L.rchb() + 8*RNW*lane,V,L.lkmer()[li],lastnode,lmax,reinterpret_cast<LDSQ id_t *>(L.lscr()) + RPSTL*lane,RPSTL);
					if ( flags == (512|0x8000) ) { rover = true; flags = 0; }
				}
				// an enumeration whose heap of pending paths outgrew the lane's share of the scratch runs again with all of it
				for ( uint64_t ro = wv_ballot(rover); ro; ro &= ro-1 )
				{
					wv_sync();
					if ( lane == static_cast<int>(__builtin_ctzll(ro)) )
						reverseEnumerateLane(R,L.rchb() + 8*RNW*lane,V,L.lkmer()[li],lastnode,lmax,reinterpret_cast<LDSQ id_t *>(L.lscr()),FastLds<CT>::lscrbytes/sizeof(id_t));
				}
				wv_sync();
				flags = wv_or(flags); if ( flags ) return false;
				uint32_t tot; uint32_t const sbase = sb + wv_scan_excl(ract ? R.narp : 0u,tot);
				if ( sb + tot > CT::rccap ) { over(512|0x4000); return false; }
#if defined(DACC_EMUL)
				if ( ract ) { FILE * f = ftrav_file(); if ( f ) fprintf(f,"R %d %u %u 0\n",int(CT::maxs),R.nrp,R.narp); }
#endif
				SITE_T0
				if ( ract ) reverseBlockCopy(R,sbase);
				// blocks of more than 16 entries are sorted with an explicit stack (one lane at a time)
				uint64_t big = wv_ballot(ract && R.narp > 16);
				if ( ract && R.narp <= 16 ) reverseBlockFinish<true>(R,sbase,li,lastnode,lmax);
				while ( big )
				{
					int const b = __builtin_ctzll(big); big &= big-1;
					if ( lane == b ) reverseBlockFinish<true>(R,sbase,li,lastnode,lmax);
				}
				SITE(21)      // traverse: reverse blocks copied, sorted, ranked (lanes = last k-mer candidates)
				sb += tot;
				flags = wv_or(flags); if ( flags ) return false;
			}
			rstop = sb;
		}
		wv_sync();
		}
		PROF(*this,11)

		// ---- batches of forward trees (lane = first k-mer candidate) and their pairs ----
		uint32_t fstart = 0, bw = WSZ, pskip = 0;
		while ( fstart < nF )
		{
			materializeKept();      // the trees of the batch before are about to be overwritten
			uint32_t const fi = fstart + lane;
			bool const fact = static_cast<uint32_t>(lane) < bw && fi < nF;
			FEnum F; int32_t firstnode = -1; uint32_t fover = 0;
			LEDGER_REP(11)
			{
			if ( lane == 0 ) L.ctr()[1] = 0;
			wv_sync();
			clInit(F.C,L.fchb() + 8*FNW*(fi < nF ? fi : static_cast<uint32_t>(FNC))); F.np = 0; F.nfpop = 0; F.fmaxw = 0; F.ffm = 0; F.m0 = 0; F.m1 = 0; if constexpr ( CT::wide != 0 ) F.m2 = 0;
			firstnode = -1;
			fover = 0;
			if ( fact )
			{
				uint32_t const saved = flags; flags = 0;
				View V; viewOfFirst(V,fi);
				firstnode = L.fnode()[fi] == 0xFFFF ? -1 : L.fnode()[fi];
				forwardEnumerateLane(F,L.fchb() + 8*FNW*fi,V,firstnode,lmax,reinterpret_cast<LDSQ id_t *>(L.lscr()) + 12*lane);
				if ( flags == (512|0x10000) && F.np < 8*FNW*FCH ) { fover = 1; flags = saved; }   // no pool space left for this tree
				else flags |= saved;
#if defined(DACC_EMUL)
				{ FILE * f = ftrav_file(); if ( f ) fprintf(f,"T %d %u %u %u\n",int(CT::maxs),F.np,F.nfpop,fover); }
#endif
			}
#if defined(DACC_LEDGER)
			wv_sync();      // (the second run resets the chunk counter: every lane must have left the first)
#endif
			}
			flags = wv_or(flags); if ( flags ) return false;
			uint64_t const fo = wv_ballot(fover);
			uint32_t nb = nF - fstart; if ( nb > bw ) nb = bw;
			if ( fo ) { uint32_t const f0 = __builtin_ctzll(fo); if ( f0 < nb ) nb = f0; }
			if ( nb == 0 )
			{
				// the first tree of the batch lost the race for pool space: run it alone, and give up if even that fails
				if ( bw == 1 ) { over(512|0x10000); return false; }
				bw = 1;
				continue;
			}
			if ( fo )
			{
				// the lanes that lost the race for chunks have left holes in the pool and the chunk counter beyond its end
				if ( nb == 1 && bw != 1 ) { bw = 1; continue; }       // a single tree is kept: run it again with the pool to itself
				uint32_t mx = 0;
				if ( fact && static_cast<uint32_t>(lane) < nb ) for ( uint32_t i = 0; i < F.C.n; ++i ) { uint32_t const id = F.C.ids[i]; mx = id+1 > mx ? id+1 : mx; }
				mx = wv_max(mx);
				if ( lane == 0 ) L.ctr()[1] = mx;      // exact trees of the batch's pairs go behind the kept trees
				wv_sync();
			}
			// a batch that did not fit sets the width of the next ones
			bw = fo ? nb : ((2*bw < WSZ) ? 2*bw : static_cast<uint32_t>(WSZ));
			{ SITE_T0 if ( fact && static_cast<uint32_t>(lane) < nb ) forwardTreeFinish(F,fi,firstnode,lmax); SITE(22) }
			wv_sync();
			PROF(*this,10)
			if ( lane == 0 ) { pcount(26,1); pcount(25,nb*nL); }
			uint32_t const npairs = nb*nL;
			bool restart = false;
			for ( uint32_t p0 = pskip; p0 < npairs && !restart; p0 += NPL )
			{
				uint32_t const nround = (npairs-p0 < NPL) ? (npairs-p0) : static_cast<uint32_t>(NPL);
				bool const cfull = wv_bcast(ncdh == 16 ? 1u : 0u,0) != 0;
				roundT0 = cfull ? L.cdh()[0].w : 0ull;
				uint64_t live = 0;
				static_assert(NPL <= 64,"one bit per pair of a round");
				LEDGER_REP(12)
				{
				live = 0;
				// phase A: classification; a pair that combines cached enumerations lists its matching pops (mode PM_PEND | number of matches)
				LDSQ PSI * const HH = reinterpret_cast<LDSQ PSI *>(L.lscr());
				uint32_t ntask = 0;
				for ( uint32_t t0 = 0; t0 < nround; t0 += WSZ )
				{
					uint32_t const t = t0 + lane;
					uint32_t mode = PM_SKIP;
					if ( t < nround )
					{
						uint32_t const p = p0 + t;
						uint32_t pfi, pli; pairFL(p,pfi,pli); pfi += fstart;
						SITE_T0
						uint32_t const cl = classifyPair(pfi,pli,lmax);
						SITE(26)      // pair generation: classification of a pair (cached enumerations valid?)
						if ( cl != 3 ) mode = PM_EXACT | cl;
						else if ( (L.rfmask()[pli] & L.ffm()[pfi]) == 0 ) mode = PM_SKIP;     // the forward tree and the reverse block share no junction k-mer
						else
						{
							ChunkList<FNW> FC; forwardTreeLoad(FC,pfi);
							uint32_t const nm = matchPops(FC,L.fnp()[pfi],L.rfmask()[pli],HH + PSIQ*t);
							if ( nm == 0 ) mode = PM_SKIP;
							else mode = PM_PEND | (nm <= PSIQ ? nm : 15u);      // 15: more matches than the list holds -- the lane form, in phase B (its records share the task list's bytes)
						}
						L.poutn()[t] = mode;
					}
					uint32_t tot; wv_scan_excl(((mode & 0xF0u) == PM_PEND && (mode & 0x0Fu) != 15u) ? (mode & 0x0Fu) : 0u,tot);
					ntask += tot;
				}
				wv_sync();
				// the task list borrows the pairs' record area (written in phase B): 16 bit entries pair | match << 6
				LDSQ uint16_t * const TL = reinterpret_cast<LDSQ uint16_t *>(L.pout());
				enum : uint32_t { TLCAP = 32u*32u*static_cast<uint32_t>(sizeof(id_t))/2u };
				bool const flat = ntask != 0 && ntask <= TLCAP;
				if ( flat )
				{
					uint32_t tb = 0;
					for ( uint32_t t0 = 0; t0 < nround; t0 += WSZ )
					{
						uint32_t const t = t0 + lane;
						uint32_t const mode = t < nround ? L.poutn()[t] : static_cast<uint32_t>(PM_SKIP);
						uint32_t const nm = ((mode & 0xF0u) == PM_PEND && (mode & 0x0Fu) != 15u) ? (mode & 0x0Fu) : 0u;
						uint32_t tot; uint32_t const pre = tb + wv_scan_excl(nm,tot);
						for ( uint32_t j = 0; j < nm; ++j ) TL[pre+j] = static_cast<uint16_t>(t | (j << 6));
						tb += tot;
					}
					wv_sync();
					// phase T: one scoreInterval per lane and step
					for ( uint32_t q0 = 0; q0 < ntask; q0 += WSZ )
					{
						uint32_t const q = q0 + lane;
						if ( q < ntask )
						{
							uint32_t const en = TL[q], t = en & 63u, j = en >> 6;
							uint32_t const p = p0 + t;
							uint32_t pfi, pli; pairFL(p,pfi,pli); pfi += fstart;
							ChunkList<FNW> FC; forwardTreeLoad(FC,pfi);
							if ( !intervalTask(FC,L.rbase()[pli],L.rn()[pli],lmin,lmax,HH + PSIQ*t + j) ) L.poutn()[t] = PM_SERIAL;
						}
					}
					wv_sync();
				}
				// phase B: heap of the valid intervals and the pops of the lane form (pairs still pending; without the task list: the lane form)
				for ( uint32_t t = lane; t < nround; t += WSZ )
				{
					uint32_t mode = L.poutn()[t];
					if ( (mode & 0xF0u) == PM_PEND )
					{
						uint32_t const p = p0 + t;
						uint32_t pfi, pli; pairFL(p,pfi,pli); pfi += fstart;
						ChunkList<FNW> FC; forwardTreeLoad(FC,pfi);
						uint32_t cnt;
						if ( flat && (mode & 0x0Fu) != 15u )
						{
							uint32_t const n = heapOfList(FC,L.rbase()[pli],HH + PSIQ*t,mode & 0x0Fu);
							cnt = combineLanePops(FC,L.rbase()[pli],n,16,HH + PSIQ*t,L.pout() + 2*POUTE*t,cfull,roundT0);
						}
						else cnt = combineLane(FC,L.fnp()[pfi],L.rbase()[pli],L.rn()[pli],L.rfmask()[pli],lmin,lmax,16,HH + PSIQ*t,L.pout() + 2*POUTE*t,cfull,roundT0);
						mode = cnt == 0xFF ? static_cast<uint32_t>(PM_SERIAL) : (cnt ? cnt : static_cast<uint32_t>(PM_SKIP));
						L.poutn()[t] = mode;
					}
					if ( mode != PM_SKIP ) live |= 1ull << t;
				}
				live = wv_or64(live);
				wv_sync();
				}
				PROF(*this,5)
				if ( lane == 0 ) pcount(27,1);
				uint32_t q = 0;
				while ( true )
				{
					uint32_t req = 0;
					// (round 6, measured and dropped: the replay with every lane in uniform control flow, the candidate heap cached in registers --
					// entry i in lane i, v_readlane in the sift chains -- and a pair's recorded entries fetched by one lane each.  Bit-identical
					// on the 64-lane emulation and on tiers 0 / 1 / 6 of the device, 0.45 % faster there (725.3 -> 722.0 ms at 3000 reads,
					// profiles/r06e): the regular replay is 5 % of a window, not the 13 % the probe-inflated site ledger of round 5 showed.  And
					// WRONG in the deep tiers: a register that holds a different value in every lane and is read with v_readlane does not survive
					// the allocator's spill / reload or live-range copies inside a divergent region (they move the ACTIVE lanes only), and
					// k_window_fast<4|2|3> spill -- test_deep_batch_starts_in_the_deep_tier failed on the device while the emulation passed.)
					if ( lane == 0 ) { lscrdirty = false; req = replayRound(q,nround,p0,fstart,lmin,lmax,nb == 1,live); }
					wv_sync();
					flags = wv_bcast(flags,0); if ( flags ) return false;
					req = wv_bcast(req,0);
					if ( !req ) break;
					if ( req == 2 )
					{
						uint32_t const pq = p0 + wv_bcast(q,0);
						fstart += pq/nL; pskip = pq%nL; bw = 1; restart = true;
						if ( lane == 0 ) pcount(28,1);
						break;
					}
					break;      // (req is 0 or 2: the middle pieces of twice-split stretches are in the pool before the pairs start)
				}
				PROF(*this,7)
			}
			if ( restart ) continue;
			fstart += nb; pskip = 0;
		}
		{ SITE_T0 materializeKept(); SITE(34) }      // the pools give way to the build-phase arrays
		{ SITE_T0 LEDGER_REP(13) restoreS(); SITE(25) }
		PROF(*this,12)
		// CDH -> CH -> ACC (:5099-5136) leaves the kept candidates in descending weight order.  With pairwise distinct
		// weights that order does not depend on the heaps: one lane per candidate counts the heavier ones and stores its
		// candidate at that rank.  Equal weights are common (35 % of the windows of a 20x batch: one path reached through two
		// (first, last) pairs has one weight) and the heaps' mechanics decide their order, but that order reaches the window
		// only through entry 0 of the final sort: the heaviest candidate among those with the smallest error sum.  So equal
		// weights are ranked by their index in CDH first, and lane 0 runs the two heaps -- and decode, errors and sort once
		// more from their order -- only if a candidate ties entry 0 in error sum AND weight and spells another string
		// (0.7 % of the windows; in 0.36 % the heaps' order does change the consensus).  CDH and the stretch sequences are not written in between; CH, the temporary of the
		// final sort, is free again when the heaps need it.  tiefast == 0: every tie takes the heaps, as before.
		wv_sync();
		uint32_t const nkept = wv_bcast(ncdh,0);
		bool const tiefast = tieFastOn();
		bool exact = false;
		uint32_t tie = 0;
		while ( true )
		{
			if ( !exact )
			{
				LEDGER_REP(18)
				{
				tie = 0;
				for ( uint32_t c = lane; c < nkept; c += WSZ )
				{
					FCC const e = ldget(L.cdh()+c);
					uint32_t rank = 0;
					for ( uint32_t j = 0; j < nkept; ++j ) { uint64_t const wj = L.cdh()[j].w; rank += (wj > e.w || (wj == e.w && j < c)) ? 1u : 0u; tie |= (wj == e.w && j != c) ? 1u : 0u; }
					ldput(L.acc()+rank,e);
				}
				tie = wv_any(tie);
				}
				FSTAT_ADD(21,tie ? 1u : 0u); FSTAT_ADD(22,nkept ? 1u : 0u);
				if ( tie && !tiefast ) exact = true;
				wv_sync();
			}
			if ( exact )
			{
#if defined(DACC_LEDGER)
				// (the heaps consume CDH: the second run of a ledger build gets it back from the lanes' registers)
				FCC keep_[WSZ >= 16 ? 1 : 16]; for ( uint32_t c = lane; c < nkept; c += WSZ ) keep_[c/WSZ] = ldget(L.cdh()+c);
#endif
				LEDGER_REP(18)
				{
#if defined(DACC_LEDGER)
				wv_sync(); for ( uint32_t c = lane; c < nkept; c += WSZ ) ldput(L.cdh()+c,keep_[c/WSZ]); wv_sync();
#endif
				if ( lane == 0 )
				{
					uint32_t nh = nkept, nch = 0, na = 0;
					while ( nh ) { FCC const c = ldget(L.cdh()); spop<FCC,true>(L.cdh(),nh); spush<FCC,false>(L.ch(),nch,c); }
					while ( nch ) { ldput(L.acc()+na,ldget(L.ch())); ++na; spop<FCC,false>(L.ch(),nch); }
				}
				}
				if ( lane == 0 ) FSTAT_ADD(32,tiefast ? 1u : 0u);      // audit aid: the exact route behind the fast one (not where the switch sends every tie here)
				wv_sync();
			}
			// decode the kept candidates, one lane each
			for ( uint32_t c = lane; c < nkept; c += WSZ )
			{
				uint32_t const slot = L.acc()[c].o, n = L.acc()[c].l & 0xFF;
				uint32_t len = 0;
				LEDGER_REP(19) len = decodeSeq(L.cseq()+FSEQCAP*slot,n,L.consL()+c*CONSROW);
				L.acc()[c].o = c*CONSROW; L.acc()[c].l = len;
			}
			wv_sync();
			LEDGER_REP(14)
			for ( uint32_t t = lane; t < nkept*mao; t += WSZ )
			{
				uint32_t const c = t / mao, j = t - c*mao;
				L.canderr()[t] = myersDistance(j,L.consL() + L.acc()[c].o,L.acc()[c].l);
			}
			wv_sync();
			// error sum of candidate c on lane c, then the stable sort by error as a rank computation, one lane per candidate
			for ( uint32_t c = lane; c < nkept; c += WSZ )
			{
				uint32_t s = 0;
				for ( uint32_t j = 0; j < mao; ++j ) s += L.canderr()[c*mao+j];
				L.accerr()[c] = s;
			}
			wv_sync();
			// std::sort of at most 16 candidates by error (:5156) = insertion sort = a stable sort: candidate c goes to the
			// number of candidates with a smaller error or the same error and a smaller index (through CH, which is free now;
			// the error sums travel in the bytes of canderr, which have been summed up)
			{
				LDSQ uint32_t * const serr = reinterpret_cast<LDSQ uint32_t *>(L.canderr());
				static_assert(16*CT::maxs >= 64 && (FastLds<CT>::o_canderr & 3) == 0,"sorted error sums borrow the candidate error bytes");
				for ( uint32_t c = lane; c < nkept; c += WSZ )
				{
					uint32_t const e = L.accerr()[c];
					uint32_t rank = 0;
					for ( uint32_t j = 0; j < nkept; ++j ) { uint32_t const ej = L.accerr()[j]; rank += (ej < e || (ej == e && j < c)) ? 1u : 0u; }
					ldput(L.ch()+rank,ldget(L.acc()+c));
					serr[rank] = e;
				}
				wv_sync();
				for ( uint32_t c = lane; c < nkept; c += WSZ ) { ldput(L.acc()+c,ldget(L.ch()+c)); L.accerr()[c] = serr[c]; }
			}
			wv_sync();
			if ( exact || !tie ) break;
			// ambiguous: a candidate behind entry 0 with its error sum and its weight that is another string
			uint32_t amb = 0;
			{
				uint32_t const e0 = L.accerr()[0], l0 = L.acc()[0].l; uint64_t const w0 = L.acc()[0].w;
				LDSQ uint64_t const * const r0 = reinterpret_cast<LDSQ uint64_t const *>(L.consL() + L.acc()[0].o);
				for ( uint32_t c = lane; c < nkept; c += WSZ )
					if ( c != 0 && L.accerr()[c] == e0 && L.acc()[c].w == w0 )
					{
						if ( L.acc()[c].l != l0 ) amb = 1;
						else
						{
							LDSQ uint64_t const * const rc = reinterpret_cast<LDSQ uint64_t const *>(L.consL() + L.acc()[c].o);
							uint64_t x = 0;
							for ( uint32_t i = 0; i < (l0 >> 3); ++i ) x |= r0[i] ^ rc[i];
							if ( l0 & 7u ) x |= (r0[l0 >> 3] ^ rc[l0 >> 3]) & ((1ull << (8u*(l0 & 7u))) - 1ull);
							amb |= x ? 1u : 0u;
						}
					}
			}
			if ( !wv_any(amb) ) break;
			exact = true;
			wv_sync();
		}
		if ( lane == 0 ) ncdh = 0;
		nacc = nkept;
		PROF(*this,13)
		FSTAT_MX(0,mao); FSTAT_MX(1,npre); FSTAT_MX(2,nn); FSTAT_MX(3,n0); FSTAT_MX(4,npool); FSTAT_MX(5,nlinks); FSTAT_MX(6,nwF); FSTAT_MX(7,nwR);
		FSTAT_MX(8,rstop); FSTAT_MX(9,nF); FSTAT_MX(10,nL); FSTAT_ADD(11,1); FSTAT_MX(12,nkept); FSTAT_ADD(24,nkept ? 0u : 1u);
#if defined(DACC_EMUL)
		if ( lane == 0 ) { FILE * f = ftrav_file(); if ( f ) { uint32_t nlv = 0; for ( uint32_t i = 0; i < nL; ++i ) nlv += L.lnode()[i] != 0xFFFF; fprintf(f,"%d %u %u %u %u %u %u %u %u %u %u %u %u\n",int(CT::maxs),mao,npre,nn,n0,npool,nF,nL,nlv,rstop,nwFall,nwRall,nkept); fflush(f); } }
#endif
		return nkept != 0;
	}

	DEV int32_t estimateLength()
	{
		int32_t maxvprodindex = -1;
		uint32_t mn = 0xFFFFFFFFu, mx = 0;
		for ( uint32_t j = lane; j < mao; j += WSZ )
		{
			uint32_t const len = L.slen()[j];
			uint32_t const lastpos = len ? len-1 : 0;
			mn = lastpos < mn ? lastpos : mn; mx = lastpos > mx ? lastpos : mx;
		}
		mn = ~wv_max(~mn); mx = wv_max(mx);
		uint32_t const supStart = mn < static_cast<uint32_t>(T.nsup) ? T.suplo[mn] : T.nrows;
		uint32_t const supEnd = mx < static_cast<uint32_t>(T.nsup) ? T.suphi[mx] : T.nrows;
		uint64_t bestbits = 0; uint32_t besti = 0xFFFFFFFFu;
		for ( uint32_t c = supStart; c < supEnd; c += WSZ )
		{
			uint32_t const i = c + lane;
			double vprod = 0.0;
			if ( i < supEnd )
			{
				double const * row = T.dpnorm + static_cast<uint64_t>(i)*T.nsup;
				vprod = 1.0;
				// same multiplication order as the reference; the table loads of four strings are issued together
				for ( uint32_t j = 0; j < mao; j += 4 )
				{
					uint32_t const l0 = L.slen()[j], l1 = j+1 < mao ? L.slen()[j+1] : 0, l2 = j+2 < mao ? L.slen()[j+2] : 0, l3 = j+3 < mao ? L.slen()[j+3] : 0;
					uint32_t const ns = static_cast<uint32_t>(T.nsup);
					double const r0 = (l0 && (l0-1) < ns) ? row[l0-1] : 0.0, r1 = (l1 && (l1-1) < ns) ? row[l1-1] : 0.0;
					double const r2 = (l2 && (l2-1) < ns) ? row[l2-1] : 0.0, r3 = (l3 && (l3-1) < ns) ? row[l3-1] : 0.0;
					if ( l0 ) vprod *= r0;
					if ( l1 ) vprod *= r1;
					if ( l2 ) vprod *= r2;
					if ( l3 ) vprod *= r3;
				}
			}
			union { double d; uint64_t u; } cv; cv.d = vprod;
			uint64_t const mb = wv_max64(cv.u);
			if ( mb > bestbits )
			{
				uint64_t const fi = wv_min64(cv.u == mb ? i : 0xFFFFFFFFull);
				bestbits = mb; besti = static_cast<uint32_t>(fi);
			}
		}
		union { double d; uint64_t u; } dm; dm.d = DACC_DBL_MIN;
		if ( bestbits > dm.u ) maxvprodindex = besti;
		if ( maxvprodindex == -1 )
		{
			// density fallback (HandleContext.hpp:2103-2155): histogram of lengths (count-1) against the DPnormSquare rows
			int32_t res = -1;
			if ( lane == 0 )
			{
				uint32_t maxlen = 0;
				for ( uint32_t j = 0; j < mao; ++j ) maxlen = L.slen()[j] > maxlen ? L.slen()[j] : maxlen;
				int32_t maxoff = -1; double maxoffv = DACC_DBL_MIN;
				for ( int32_t i = 0; i < T.nrows; ++i )
				{
					uint32_t const fs = T.dpsq_first[i], sz = T.dpsq_size[i];
					double const * V = T.dpsq + static_cast<uint64_t>(i)*T.nsup;
					double sdot = 0;
					for ( uint32_t t = 0; t < sz; ++t )
					{
						uint32_t const jj = fs+t;
						if ( jj < maxlen+1 )
						{
							uint32_t cnt = 0;
							for ( uint32_t j = 0; j < mao; ++j ) cnt += (L.slen()[j] == jj);
							double const o = cnt ? static_cast<double>(cnt-1) : 0.0;
							sdot += V[jj] * o;
						}
						else break;
					}
					if ( sdot > maxoffv ) { maxoff = i; maxoffv = sdot; }
				}
				if ( maxoff != -1 && maxoffv >= 1e-3 ) res = maxoff;
			}
			maxvprodindex = static_cast<int32_t>(wv_bcast(static_cast<uint32_t>(res),0));
		}
		return maxvprodindex;
	}

	// The consensus -> A alignment of a narrow window (w <= 64) is not done here: the tier leaves a pending record (storePending) and k_emit
	// aligns one window per lane (emit_record.hpp).  A wide window (w in 65 ... 127, wide tier) is aligned on lane 0: two words per column
	// (rows 0-63 / 64-m-1; column c at alpv[2c], alpv[2c+1]), the horizontal delta leaving word 0 enters word 1 (as in the two-word distance
	// kernel); traceback priority diagonal > DEL > INS, same steps as the generic engine's alignAndEmitWide (dbg_window.hpp); returns the
	// number of steps of the edit script left in alops
	DEV uint32_t alignAndEmitWide(LDSQ uint8_t const * cons, uint32_t const n)
	{
		if constexpr ( CT::wide != 0 )
		{
		uint32_t const m = P.w;
		enum { PW = FastLds<CT>::pw };
		static_assert(PW >= 2,"the A window of a wide tier (string 0, stride PW) has at least two words per pattern mask: w <= 128 uses words 0 and 1");
		LDSQ uint64_t const * PEQ = L.peq();      // string 0 = the A window: word q of symbol c at PW*c + q
		uint64_t const mask1 = (m == 128) ? ~0ull : ((1ull<<(m-64))-1);
		uint64_t Pv0 = ~0ull, Mv0 = 0, Pv1 = mask1, Mv1 = 0; uint32_t score = m;
		L.alpv()[0] = Pv0; L.alpv()[1] = Pv1; L.almv()[0] = Mv0; L.almv()[1] = Mv1; L.albot()[0] = m;
		uint64_t const top = 1ull<<(m-65);
		for ( uint32_t c = 0; c < n; ++c )
		{
			uint32_t const ch = cons[c] & 3u;
			uint64_t const Eq0 = PEQ[PW*ch], Eq1 = PEQ[PW*ch+1];
			uint64_t const Xv0 = Eq0 | Mv0;
			uint64_t const Xh0 = (((Eq0 & Pv0) + Pv0) ^ Pv0) | Eq0;
			uint64_t Ph0 = Mv0 | ~(Xh0 | Pv0);
			uint64_t Mh0 = Pv0 & Xh0;
			uint64_t const phc = Ph0>>63, mhc = Mh0>>63;
			Ph0 = (Ph0<<1) | 1ull; Mh0 <<= 1;
			Pv0 = Mh0 | ~(Xv0 | Ph0);
			Mv0 = Ph0 & Xv0;
			uint64_t const Eq1c = Eq1 | mhc;
			uint64_t const Xv1 = Eq1 | Mv1;
			uint64_t const Xh1 = (((Eq1c & Pv1) + Pv1) ^ Pv1) | Eq1c;
			uint64_t Ph1 = Mv1 | ~(Xh1 | Pv1);
			uint64_t Mh1 = Pv1 & Xh1;
			if ( Ph1 & top ) ++score; else if ( Mh1 & top ) --score;
			Ph1 = (Ph1<<1) | phc; Mh1 = (Mh1<<1) | mhc;
			Pv1 = (Mh1 | ~(Xv1 | Ph1)) & mask1;
			Mv1 = (Ph1 & Xv1) & mask1;
			L.alpv()[2*c+2] = Pv0; L.alpv()[2*c+3] = Pv1; L.almv()[2*c+2] = Mv0; L.almv()[2*c+3] = Mv1; L.albot()[c+1] = score;
		}
		uint32_t i = m, j = n; uint32_t d = score; uint32_t nops = 0;
		while ( i || j )
		{
			uint32_t op = 2; bool done = false;
			if ( i && j )
			{
				uint32_t const sh = i-1;
				uint64_t const p0 = L.alpv()[2*(j-1)], p1 = L.alpv()[2*(j-1)+1], q0 = L.almv()[2*(j-1)], q1 = L.almv()[2*(j-1)+1];
				uint32_t const np_ = sh < 64 ? (dacc_popc64(p0>>sh) + dacc_popc64(p1)) : dacc_popc64(p1>>(sh-64));
				uint32_t const nm_ = sh < 64 ? (dacc_popc64(q0>>sh) + dacc_popc64(q1)) : dacc_popc64(q1>>(sh-64));
				uint32_t const dd = L.albot()[j-1] - np_ + nm_;
				uint32_t const cj = cons[j-1] & 3u;
				uint32_t const neq = ((PEQ[PW*cj + (sh>>6)] >> (sh&63u)) & 1ull) ? 0u : 1u;      // A[i-1] != cons[j-1]
				if ( dd + neq == d ) { op = neq ? 1 : 0; --i; --j; d = dd; done = true; }
			}
			if ( !done && i )
			{
				uint32_t const r = i-1;
				uint64_t const pv = L.alpv()[2*j+(r>>6)];
				if ( (pv >> (r&63u)) & 1ull ) { op = 3; --i; d = d-1; done = true; }
			}
			if ( !done ) { op = 2; --j; d = d-1; }
			L.alops()[nops++] = op;
		}
		return nops;
		}
		else return 0;
	}
	// window record from the edit script alops[0..nops) (traceback order: last step first), all lanes.  Every step emits
	// exactly one symbol (INS / MATCH / MISMATCH: the next consensus symbol, DEL: 'D' = 4), so symbol q belongs to step q
	// in forward order; off[r] = number of symbols before the group of A column r = index behind the (r-1)-th step that
	// consumes an A symbol (HandleContext.hpp:2448-2489)
	DEV void emitRecordWide(LDSQ uint8_t const * cons, uint32_t const nops, uint8_t * rec)
	{
		if constexpr ( CT::wide != 0 )
		{
			uint32_t const m = P.w;
			// wide record (dev_types.hpp): 16 bit group offsets from rec[2] on, symbols behind the m+2 offsets
			uint8_t * const off = rec+2; uint8_t * const sym = rec + 2 + 2*(m+2);
			if ( lane == 0 ) { rec[0] = WREC_FINAL; rec[1] = 0; off[0] = 0; off[1] = 0; off[2*(m+1)] = nops & 0xFFu; off[2*(m+1)+1] = nops >> 8; }
			uint32_t cbase = 0, abase = 0;
			for ( uint32_t c0 = 0; c0 < nops; c0 += WSZ )
			{
				uint32_t const q = c0 + lane;
				bool const act = q < nops;
				uint32_t const op = act ? L.alops()[nops-1-q] : 2u;
				uint32_t ctot, atot;
				uint32_t const cpos = cbase + wv_scan_flag(act && op != 3,ctot);
				uint32_t const arank = abase + wv_scan_flag(act && op != 2,atot);
				if ( act )
				{
					sym[q] = (op == 3) ? 4 : cons[cpos];
					if ( op != 2 ) { off[2*(arank+1)] = (q+1) & 0xFFu; off[2*(arank+1)+1] = (q+1) >> 8; }
				}
				cbase += ctot; abase += atot;
			}
		}
	}
	// pending record of a narrow window (dev_types.hpp: WREC_PENDING), all lanes: one 64 bit word per lane -- the header, the four pattern
	// masks of the A window (string 0: word 0 of every symbol), the consensus.  cons is 8 byte aligned and readable up to the next
	// multiple of 8 behind n (bestL); rec is the window's 256 byte slot
	DEV void storePending(LDSQ uint8_t const * cons, uint32_t const n, uint8_t * rec)
	{
		enum { PW = FastLds<CT>::pw };
		static_assert(MAXCONS <= 96 && (FastLds<CT>::o_bestL & 7) == 0 && PEND_PEQ == 8 && PEND_CONS == 40,"one 64 bit word per lane: header, four masks, twelve words of consensus");
		LDSQ uint64_t const * T8 = reinterpret_cast<LDSQ uint64_t const *>(cons);
		uint64_t * const R8 = reinterpret_cast<uint64_t *>(rec);
		for ( uint32_t q = lane; q < PEND_CONS/8 + (n+7)/8; q += WSZ )
			R8[q] = (q == 0) ? (static_cast<uint64_t>(WREC_PENDING) | (static_cast<uint64_t>(n) << (8*PEND_LEN))) : ((q < PEND_CONS/8) ? L.peq()[(q-1)*PW] : T8[q-PEND_CONS/8]);
	}
};

// returns FW_DONE, FW_NEXT (does not fit this tier's capacities) or FW_GENERIC (shape no LDS tier supports)
enum { FW_DONE = 0, FW_NEXT = 1, FW_GENERIC = 2 };
// Size class of a window (pre-pass of shallow batches): 0 = small (starts in tier 0), 1 = the rest (starts in tier 1).  An
// upper bound of the number of k-mer instances at the smallest k from the window tables: every active overlap counts (the
// window may keep fewer, `maxalign`), so a window classed small can still overflow tier 0 and is then handed on like any other.
DEV uint32_t classifyWindow(WindowBatch const & B, uint64_t const widx, uint32_t const t0inst, uint32_t const t7inst = 0)
{
	// (round 6, measured and dropped: the pile index from a table filled by a pre-pass instead of this search -- no difference, profiles/r06d)
	uint32_t lo = 0, hi = B.npiles;
	while ( hi-lo > 1 ) { uint32_t const mid = (lo+hi)>>1; if ( B.piles[mid].winbase <= widx ) lo = mid; else hi = mid; }
	DevPile const pile = B.piles[lo];
	uint32_t const y = static_cast<uint32_t>(widx - pile.winbase);
	uint32_t astart, aend;
	windowInterval(pile.l,B.P.a,B.P.w,y,astart,aend);
	uint32_t const k = B.P.klow;
	uint32_t nact = 0, inst = B.P.w >= k ? (B.P.w - k + 1) : 0u;
	DevOvl const * ov = B.ovl + pile.first_ovl;
	for ( uint32_t z = 0; z < pile.novl; ++z )
		if ( ov[z].abpos <= static_cast<int32_t>(astart) && ov[z].aepos >= static_cast<int32_t>(aend) )
		{
			uint64_t const row = ov[z].wtoff + (y - ov[z].y0);
			uint32_t const len = B.wt_e[row] - B.wt_b[row];
			++nact; inst += len >= k ? (len - k + 1) : 0u;
		}
	uint64_t const nb = (B.P.maxalign > 0) ? (B.P.maxalign-1) : 0;
	uint32_t const mao = 1 + static_cast<uint32_t>(nact < nb ? nact : nb);
	// 0: tier 0, 1: the rest (tier 1), 2: the middle class (tier 7; only with a threshold for it)
	if ( mao <= FastTier<0>::maxs && inst <= t0inst && B.P.w <= 63 ) return 0u;
	if ( t7inst && mao <= FastTier<7>::maxs && inst <= t7inst && B.P.w <= 63 ) return 2u;
	return 1u;
}

template<typename CT>
DEV int processWindowFast(FastBatch const & FB, uint64_t const widx, LDSQ uint8_t * lds, bool const resume = false)
{
	WindowBatch const & B = FB.W;
	FastEngine<CT> E;
#if defined(DACC_EMUL)
	{ char const * pz = getenv("DACC_EMUL_POISON"); if ( pz ) __builtin_memset(static_cast<void *>(&E),atoi(pz),sizeof(E)); }   // debugging aid: no member may be read before it is set
#endif
	if ( B.pregen && ((B.pregen[widx>>5] >> (widx&31)) & 1) ) return FW_DONE;      // the generic engine has this window (a string longer than 64 bases)
	E.mao = 0; E.k = 0; E.kmask = 0; E.npre = E.nlast = E.nn = E.nmfirst = E.nmlast = 0; E.n0 = E.npool = E.nlinks = E.nwF = E.nwR = 0; E.nF = E.nL = 0;
	E.nsiq = E.ncdh = E.nacc = 0; E.rstop = 0; E.roundT0 = 0; E.cfree = 0; E.pvpath = E.pvrp = E.pvnf = 0; E.pvcl = 0; E.nmid = 0; E.midbase = 0; E.nLmagic = 0;
	E.T = B.T; E.P = B.P; E.nrows = FB.F.nrows; E.nsup = FB.F.nsup; E.vst = FB.dpsq_vst;
	E.gslab = 0; E.gtab = FB.tab32; E.sfresh = true; E.sdirty = false;
	if ( CT::gw )
	{
#if defined(DACC_EMUL)
		E.gslab = FB.gslab;
#else
		E.gslab = FB.gslab + static_cast<uint64_t>(blockIdx.x)*FB.gstride;
#endif
		// (one-slab tier: the weights, the spill image and the instance image follow the layout in the buffer the caller passed as `lds`)
		if constexpr ( FastOneSlab<CT>::value != 0 ) E.gslab = (uint8_t *)(lds) + FastLds<CT>::g_base;
	}
	E.lane = wv_lane(); E.flags = 0; E.prof = B.prof; E.feasneed = FB.feasneed; E.tiefast = FB.tiefast;
#if defined(DACC_EMUL)
	E.feascount = false; E.feasapplied = false; E.nwFall = E.nwRall = 0;
#endif
#if defined(DACC_LEDGER)
	E.ledger = FB.ledger;
#endif
#if defined(DACC_PROFILE) && !defined(DACC_EMUL)
	uint64_t * const prof = E.prof;
#endif
#if defined(DACC_EMUL)
	g_fstats.clear();
#endif
	E.L.base = lds;
	FastLds<CT> const & L = E.L;
	int const lane = E.lane;
	PROF_T0
	// A window that does not fit is handed to the next capacity tier together with the filter frequency of the pass
	// that overflowed: with a single k the passes before it ended without a consensus and left no state behind
	// (minrate, best), so the next tier starts at that pass instead of repeating them.
	int32_t curff = B.P.maxff;
	uint32_t hslot = 0;      // hand-over slot + 1 with the sorted instances of this window (FastBatch::hand), 0: none
	bool const handable = FB.hand != 0 && B.P.klow == B.P.khigh && CT::gw != 0;
	if ( resume && B.P.klow == B.P.khigh )
	{
		WindowOut const prev = B.wout[widx];
		if ( prev.status == WS_RETRY && prev.filterfreq <= B.P.maxff && prev.filterfreq >= B.P.minff )
		{
			curff = prev.filterfreq;
			if ( handable && prev.minrate <= FB.handcap ) hslot = static_cast<uint32_t>(prev.minrate);
		}
	}
	int32_t const startff = curff;
	#define FFAIL(code) { if ( lane == 0 ) { B.wout[widx].status = WS_RETRY; B.wout[widx].flags = ((code)<<24) | (E.flags & 0xFFFFFF); B.wout[widx].filterfreq = curff; B.wout[widx].minrate = hslot; } return ((code) == 1 || (code) == 4) ? FW_GENERIC : FW_NEXT; }

	// (round 6, measured and dropped: the pile index from a table filled by a pre-pass instead of this search -- no difference, profiles/r06d)
	uint32_t lo = 0, hi = B.npiles;
	while ( hi-lo > 1 ) { uint32_t const mid = (lo+hi)>>1; if ( B.piles[mid].winbase <= widx ) lo = mid; else hi = mid; }
	DevPile const pile = B.piles[lo];
	uint32_t const y = static_cast<uint32_t>(widx - pile.winbase);
	uint32_t astart, aend;
	windowInterval(pile.l,B.P.a,B.P.w,y,astart,aend);

	WindowOut out; out.status = WS_INSUFFICIENT; out.mao = 0; out.elength = 0; out.k = 0; out.filterfreq = -1; out.conslen = 0; out.minrate = 0; out.flags = 0;
	uint8_t * rec = B.wrec + widx*(CT::wide ? DACC_WREC_OF(B.P.w) : static_cast<uint32_t>(WREC));
	if ( lane == 0 ) rec[0] = 0;
	if ( B.P.w > (CT::wide ? (FastRows3<CT>::value ? 128u : 127u) : 63u) ) { FFAIL(1) }      // (rows 0 ... w of the model table: 64, 128 or 192 positions per mask)

	DevOvl const * ov = B.ovl + pile.first_ovl;
	uint32_t nact = 0, mao = 0, toolong = 0;
	LEDGER_REPX(E,0)
	{
	nact = 0;
	for ( uint32_t c = 0; c < pile.novl; c += WSZ )
	{
		uint32_t const z = c + lane;
		uint32_t act = 0;
		if ( z < pile.novl ) act = (ov[z].abpos <= static_cast<int32_t>(astart)) && (ov[z].aepos >= static_cast<int32_t>(aend));
		uint32_t tot; uint32_t const pre = wv_scan_excl(act,tot);
		if ( act && nact+pre < CT::precap ) L.pre()[nact+pre] = (static_cast<uint64_t>(ov[z].ekey)<<32) | z;
		nact += tot;
	}
	if ( nact > CT::precap || next_pow2(nact < 2 ? 2 : nact) > CT::precap ) { FFAIL(2) }      // (the padding below needs the next power of two to fit)
	uint32_t const ap2 = next_pow2(nact < 2 ? 2 : nact);
	for ( uint32_t i = nact + lane; i < ap2; i += WSZ ) L.pre()[i] = ~0ull;
	wv_sync();
	wv_sort_keys<CT::precap>(L.pre(),nact);
	mao = 0;
	if ( nact )
	{
		uint64_t const nb = (B.P.maxalign > 0) ? (B.P.maxalign-1) : 0;
		mao = 1 + static_cast<uint32_t>(nact < nb ? nact : nb);
	}
	if ( mao > CT::maxs ) { FFAIL(3) }
	// the deep-window tier runs only what the tiers behind it cannot hold: the others go on as they came (filter frequency and hand-over slot kept)
	if constexpr ( CT::mins != 0 ) { if ( mao <= CT::mins ) { FFAIL(3) } }
	E.mao = mao; out.mao = mao;

	toolong = 0;
	if ( mao )
	{
		// string descriptors, one lane per string (a single round of dependent HBM loads for the whole window):
		// mfirst[j] = first base | read length << 32, mlast[j] = byte offset of the read | inverse << 63
		for ( uint32_t j = lane; j < mao; j += WSZ )
		{
			uint32_t bs, len, rl; uint64_t off; bool inv;
			if ( j == 0 ) { bs = astart; len = B.P.w; off = B.boff[pile.aread]; rl = B.rlen[pile.aread]; inv = false; }
			else
			{
				uint32_t const z = static_cast<uint32_t>(L.pre()[j-1] & 0xFFFFFFFFu);
				DevOvl const & o = ov[z];
				uint64_t const row = o.wtoff + (y - o.y0);
				bs = B.wt_b[row]; len = B.wt_e[row]-bs;
				off = B.boff[o.bread]; rl = B.rlen[o.bread]; inv = o.flags & 1;
			}
			if ( len > FastLds<CT>::maxlen ) { toolong = 1; len = 0; }
			L.slen()[j] = len;
			L.mfirst()[j] = bs | (static_cast<uint64_t>(rl)<<32);
			L.mlast()[j] = off | (static_cast<uint64_t>(inv ? 1 : 0)<<63);
		}
		toolong = wv_any(toolong);
		wv_sync();
		// bases: lane p of string j; four strings per round so that their loads are in flight together
		for ( uint32_t j0 = 0; j0 < mao; j0 += 4 )
			for ( uint32_t p = lane; p < CT::lstr; p += WSZ )
			{
				uint8_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
				bool const a0 = p < L.slen()[j0], a1 = j0+1 < mao && p < L.slen()[j0+1], a2 = j0+2 < mao && p < L.slen()[j0+2], a3 = j0+3 < mao && p < L.slen()[j0+3];
				#define DACC_LB(u) { uint64_t const d0 = L.mfirst()[j0+u], d1 = L.mlast()[j0+u]; v##u = readBase(B.bps,d1 & 0x7FFFFFFFFFFFFFFFull,static_cast<uint32_t>(d0>>32),(d1>>63) != 0,static_cast<uint32_t>(d0)+p); }
				if ( a0 ) DACC_LB(0)
				if ( a1 ) DACC_LB(1)
				if ( a2 ) DACC_LB(2)
				if ( a3 ) DACC_LB(3)
				#undef DACC_LB
				if constexpr ( CT::gw != 0 )
				{
					// pattern masks by ballot: bit p of word c of string j <=> symbol c at position p (positions behind the string: no bit)
					// (words 4*PW*j + PW*symbol + word: PW = 2 holds strings of up to 128 bases, the second round of p fills word 1; PW = 4: four rounds, up to 255)
					enum { PW = FastLds<CT>::pw };
					uint32_t const sh0 = p - static_cast<uint32_t>(lane);      // (a 64-lane wavefront: 0 or 64; the 1-lane test build walks p)
					uint32_t const wq = sh0 >> 6, sh = sh0 & 63u;
					#define DACC_PM(u) if ( j0+u < mao ) { \
						uint64_t const b0 = wv_ballot(a##u && v##u == 0) << sh, b1 = wv_ballot(a##u && v##u == 1) << sh, b2 = wv_ballot(a##u && v##u == 2) << sh, b3 = wv_ballot(a##u && v##u == 3) << sh; \
						if ( lane == 0 ) { LDSQ uint64_t * const q = L.peq() + 4*PW*(j0+u) + wq; if ( sh == 0 ) { q[0] = b0; q[PW] = b1; q[2*PW] = b2; q[3*PW] = b3; } else { q[0] |= b0; q[PW] |= b1; q[2*PW] |= b2; q[3*PW] |= b3; } } }
					DACC_PM(0) DACC_PM(1) DACC_PM(2) DACC_PM(3)
					#undef DACC_PM
				}
				else
				{
				if ( a0 ) L.str()[(j0+0)*CT::lstr+p] = v0;
				if ( a1 ) L.str()[(j0+1)*CT::lstr+p] = v1;
				if ( a2 ) L.str()[(j0+2)*CT::lstr+p] = v2;
				if ( a3 ) L.str()[(j0+3)*CT::lstr+p] = v3;
				}
			}
	}
	wv_sync();
	}
	if ( toolong ) { FFAIL(4) }
	PROF(E,0)

	int32_t elength = 0;
	if ( mao )
	{
		E.buildPeq();
		LEDGER_REPX(E,1) elength = E.estimateLength()+1;
	}
	out.elength = elength;
	PROF(E,1)

	if ( mao >= B.P.minwindowcov )
	{
		bool pathfailed = true;
		uint64_t minrate = B.P.eminrate;
		bool haveMin = false;
		uint32_t bestlen = 0;
		LDSQ uint8_t * best = L.bestL();
		for ( uint32_t k = B.P.klow; k <= B.P.khigh; ++k )
		{
			E.k = k; E.kmask = (1ull<<(2*k))-1;
			bool instvalid = false, instsaved = false, handloaded = false;
			for ( int32_t ff = startff; ff >= B.P.minff; --ff )
			{
				curff = ff;
				PROF_T0
				// the sorted instances of this k are still in place when the pass before ended without a traversal; a pass that
				// traversed has saved them to the slab first (gw tiers)
				if ( !instvalid )
				{
					SITE_T0
					if ( instsaved ) { E.restoreInstances(); SITE(27) }
					else if ( !(hslot && !handloaded && E.loadHand(FB,hslot)) ) { LEDGER_REPX(E,2) E.buildInstances(); SITE(28) }      // handed over by the tier before: no second sort
					else { SITE(30) }
					handloaded = true;
				}
				if ( E.flags ) { FFAIL(7) }     // uniform: set from wave-uniform values only
				PROF(E,2)
				LEDGER_REPX(E,3) E.buildNodes(ff > 1 ? ff : 1);
				E.flags = wv_or(E.flags);
				// the node table does not fit this tier (82 % of tier 1's hand-overs): the instances are sorted and valid, the next tier takes them
				if ( E.flags ) { if ( handable ) hslot = E.saveHand(FB,hslot); FFAIL(7) }
				PROF(E,3)
				// A pass cannot produce a candidate if no node holds position 0 of a string (no first k-mer) or no last k-mer
				// candidate is a node (every reverse enumeration is empty): its three traversals (:2270-2322) are skipped.  The
				// traversal structures then never overwrite the instance array, which the next pass takes over.
				instvalid = false;
				{ bool dead_ = false; LEDGER_REPX(E,16) dead_ = (ff != 0 && E.passIsDead()); if ( dead_ ) { instvalid = true; continue; } }
				if ( CT::gw != 0 && ff > B.P.minff && !instsaved ) { SITE_T0 LEDGER_REPX(E,17) E.saveInstances(); instsaved = true; SITE(29) }
				LEDGER_REPX(E,4) E.buildSuccessors(mao);
				PROF(E,4)
				if ( ff == 0 )
				{
					// gap filling (HandleContext.hpp:2233-2268)
					E.loadTab();
					E.levelSuccessors2();
					E.flags = wv_or(E.flags);
					if ( E.flags ) { FFAIL(6) }
					E.buildNodes(1);
					E.flags = wv_or(E.flags);
					if ( E.flags ) { FFAIL(7) }
					E.buildSuccessors(mao);
					PROF(E,6)
				}
				E.flags = wv_or(E.flags);
				if ( E.flags ) { FFAIL(7) }
				uint32_t mintry = 0; bool lconsok = false;
				while ( true )
				{
					bool const consok = E.traverse(static_cast<int64_t>(elength)-4,static_cast<int64_t>(elength)+4);
					E.flags = wv_or(E.flags);
					if ( E.flags ) { FFAIL(8) }
					if ( consok )
					{
						uint64_t const err = L.accerr()[0];
						if ( err < minrate )
						{
							lconsok = true; minrate = err; haveMin = true;
							bestlen = L.acc()[0].l;
							if ( bestlen > ((CT::wide && B.P.w > 64u) ? FastLds<CT>::consmax : static_cast<uint32_t>(MAXCONS)) ) { FFAIL(9) }
							for ( uint32_t i = lane; i < bestlen; i += WSZ ) best[i] = L.consL()[L.acc()[0].o+i];
							out.k = k; out.filterfreq = ff;
							wv_sync();
						}
						else if ( haveMin ) lconsok = true;
						break;
					}
					else
					{
						if ( ++mintry >= 3 ) break;
					}
					if ( !E.addNextFromHeap() ) break;
				}
				if ( lconsok ) { pathfailed = false; break; }
			}
		}
		if ( !pathfailed )
		{
			out.status = WS_OK; out.conslen = bestlen; out.minrate = minrate;
			PROF_T0
			LEDGER_REPX(E,15)
			{
			bool wide = false;
			if constexpr ( CT::wide != 0 ) wide = DACC_WIDE_W(B.P.w);
			if ( wide )
			{
				uint32_t nops = 0;
				wv_sync();      // the alignment scratch may lie over the candidate buffers the lanes have just read (gw layout)
				if ( lane == 0 ) nops = E.alignAndEmitWide(best,bestlen);
				wv_sync();
				nops = wv_bcast(nops,0);
				E.emitRecordWide(best,nops,rec);
			}
			else
			{
				// narrow record: the alignment is k_emit's (one lane per window, behind all engines)
				E.storePending(best,bestlen,rec);
#if defined(DACC_EMUL)
				// (host emulation: no k_emit; lane 0 converts the record with the same routine right away)
				wv_sync();
				if ( lane == 0 ) emitPendingRecord(rec,B.P.w);
				wv_sync();
#endif
			}
			}
			PROF(E,14)
		}
		else out.status = WS_FAILED;
	}
	if ( lane == 0 ) B.wout[widx] = out;
	wv_sync();
#if defined(DACC_EMUL)
	fstats_dump(static_cast<int>(CT::maxs));
#endif
	return FW_DONE;
	#undef FFAIL
}

#if defined(DACC_EMUL)
#undef over
#endif
}
#endif
