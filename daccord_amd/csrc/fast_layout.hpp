/*
 * Where the working state of one window lives: the layout FastLds<CT> of a capacity tier CT = FastTier<N> (fast_tiers.hpp), the two records
 * it holds arrays of, and fastCapsOf, which turns a tier's compile-time sizes into the run-time record FastCaps (tier_pipeline.hpp) that the
 * planner and the launches work with.  Two layouts: the gw layout of every tier but tier 5, and tier 5's legacy layout.  Nothing of the
 * engine (fast_window.hpp) is needed to read a size from here.
 */
#ifndef DACC_FAST_LAYOUT_HPP
#define DACC_FAST_LAYOUT_HPP
#include "wave.hpp"
#include "dev_types.hpp"
#include "tier_pipeline.hpp"
#include "fast_tiers.hpp"

namespace dacc {

struct FSI { uint64_t w; uint16_t left, right, current, path; };   // ScoreInterval (left/right/current: sorted reverse entries, path: forward pop index)
struct FCC { uint64_t w; uint32_t o, l; };                                       // ConsensusCandidate

HDEV constexpr uint32_t fcpow2(uint32_t v) { uint32_t p = 1; while ( p < v ) p <<= 1; return p; }
HDEV constexpr uint32_t fcmax(uint32_t a, uint32_t b) { return a > b ? a : b; }
template<bool W, typename A, typename B> struct FWideSel { typedef A type; };
template<typename A, typename B> struct FWideSel<false,A,B> { typedef B type; };

/*
 * LDS layout of one wavefront.  FLD(name,type,count,start) declares an array at byte offset `start` (a constant
 * expression), its end offset e_name (8 byte aligned) and an accessor returning an LDS (address space 3) pointer, so
 * that every access compiles to ds_read/ds_write with a constant offset.
 */
#define FLD(name,type,count,start) \
	static constexpr uint32_t o_##name = (start); \
	static constexpr uint32_t e_##name = (o_##name + static_cast<uint32_t>(sizeof(type))*static_cast<uint32_t>(count) + 7u) & ~7u; \
	HDEV LDSQ type * name() const { return reinterpret_cast<LDSQ type *>(base + o_##name); }

template<typename CT, bool GW = (CT::gw != 0)> struct FastLds;

// legacy layout: everything in LDS (tier 5 only: the one row of fast_tiers.hpp with gw = 0)
template<typename CT>
struct FastLds<CT,false>
{
	LDSQ uint8_t * base;
	static constexpr uint32_t keycap = fcpow2(CT::maxs < 2 ? 2 : CT::maxs);
	typedef uint16_t toff_t; static constexpr bool wides = false, xwides = false, ywides = false, hranges = false; static constexpr uint32_t fqmax = 255u, icap = CT::precap;      // (more than 256 strings: gw layout only)
	static_assert(CT::maxs <= 256,"the legacy layout has 8 bit node frequencies and string ids");
	static_assert((CT::precap & (CT::precap-1)) == 0,"precap must be a power of two: the bitonic sorts pad to one");
	static_assert(sizeof(typename CT::id_t) > 1 || (CT::fcap <= 256 && CT::rccap <= 256),"pool slots are recorded as id_t (pout)");
	static_assert(CT::blcap <= (FastRows3<CT>::value ? 192u : 128u) && (CT::blcap & 7) == 0,"base length buckets: two 64 bit occupancy words (three in the tier of w = 128, FastRows3), cleared 8 at a time");
	// ---- live during the whole window ----
	static_assert(CT::lstr == 64 || CT::lstr == 128 || CT::lstr == 256,"string stride: one, two or four 64 bit words per pattern mask");
	static constexpr uint32_t pw = CT::lstr/64;      // words per pattern mask
	static constexpr uint32_t maxlen = CT::lstr < 256u ? static_cast<uint32_t>(CT::lstr) : 255u;      // longest string the layout holds
	static constexpr uint32_t maskrows = 64u, supcap = static_cast<uint32_t>(FSUPCAP);      // one word per position mask, the narrow table copy
	typedef uint8_t sid_t;      // stretch ids are 8 bits in the legacy layout
	static_assert(sizeof(typename CT::sid_t) == 1,"16 bit stretch ids need the gw layout");
	FLD(str,uint8_t,CT::maxs*CT::lstr,0)
	FLD(slen,uint8_t,CT::maxs,e_str)
	FLD(peq,uint64_t,CT::maxs*4*pw,e_slen)      // pattern masks of string j: words 4*pw*j + pw*symbol + word
	FLD(ipos,uint8_t,CT::precap,e_peq)
	FLD(irpos,uint8_t,CT::precap,e_ipos)
	FLD(nv,uint32_t,CT::ncap,e_irpos)
	FLD(nps,uint16_t,CT::ncap+1,e_nv)
	FLD(nfreq,uint8_t,CT::ncap,e_nps)
	FLD(succ0,uint16_t,CT::ncap,e_nfreq)
	FLD(sinfo,uint16_t,CT::ncap,e_succ0)
	FLD(npred,uint8_t,CT::ncap,e_sinfo)
	FLD(nrange,uint32_t,CT::ncap,e_npred)   // feasible position range of a node: pfrom | pto<<8 | cpfrom<<16 | cpto<<24
	FLD(mfirst,uint64_t,keycap,e_nrange)
	FLD(mlast,uint64_t,keycap,e_mfirst)
	FLD(suplo8,uint8_t,FSUPCAP,e_mlast)
	FLD(suphi8,uint8_t,FSUPCAP,e_suplo8)
	// small scratch of the serial code (dynamically indexed, so it must not live in registers)
	FLD(vrem,uint8_t,8,e_suphi8)
	FLD(vadd,uint8_t,8,e_vrem)
	FLD(vapos,uint8_t,8,e_vadd)
	FLD(vfn,uint16_t,8,e_vapos)
	FLD(vln,uint16_t,8,e_vfn)
	FLD(sstack,uint16_t,3*24,e_vln)
	FLD(chain,uint8_t,64,e_sstack)
	FLD(midpar,uint16_t,8,e_chain)          // middle pieces of twice-split stretches: parent stretch, node range [midA,midB]
	FLD(midA,uint8_t,8,e_midpar)
	FLD(midB,uint8_t,8,e_midA)
	static constexpr uint32_t ubase = e_midB;
	// ---- overlay A: build phase ----
	FLD(pre,uint64_t,CT::precap,ubase)
	FLD(lastk,uint64_t,keycap,e_pre)
	static constexpr uint32_t uA = e_lastk;
	// ---- overlay B: traversal phase ----
	FLD(sfirst,uint16_t,CT::scap,ubase)
	FLD(slast,uint16_t,CT::scap,e_sfirst)
	FLD(sslen,uint16_t,CT::scap,e_slast)
	FLD(slink,uint16_t,CT::scap,e_sslen)
	FLD(maskF,uint64_t,CT::scap,e_slink)
	FLD(maskR,uint64_t,CT::scap,e_maskF)
	FLD(woffF,uint16_t,CT::scap,e_maskR)
	FLD(woffR,uint16_t,CT::scap,e_woffF)
	FLD(links,uint16_t,CT::lcap,e_woffR)
	// weights of the feasible (stretch, position) pairs: whole stretch (48 bit), its first node in walking direction and,
	// forward only, its last node (40 bit each), split into 32 bit low words and high parts
	FLD(wF_lo,uint32_t,CT::wcap,e_links)
	FLD(wF1_lo,uint32_t,CT::wcap,e_wF_lo)
	FLD(wFl_lo,uint32_t,CT::wcap,e_wF1_lo)
	FLD(wR_lo,uint32_t,CT::wcap,e_wFl_lo)
	FLD(wR1_lo,uint32_t,CT::wcap,e_wR_lo)
	FLD(wF_hi,uint16_t,CT::wcap,e_wR1_lo)
	FLD(wR_hi,uint16_t,CT::wcap,e_wF_hi)
	FLD(wF1_hi,uint8_t,CT::wcap,e_wR_hi)
	FLD(wFl_hi,uint8_t,CT::wcap,e_wF1_hi)
	FLD(wR1_hi,uint8_t,CT::wcap,e_wFl_hi)
	// lookup of stretches by first / last node: head index per node, base stretches ordered by (last node, id)
	FLD(lhead,uint8_t,CT::ncap,e_wR1_hi)
	FLD(lord,uint32_t,CT::scap,e_lhead)
	FLD(ppos,uint8_t,CT::scap,e_lord)      // pieces: number of base stretches sorting before them
	FLD(fkmer,uint32_t,CT::fnc,e_ppos)
	FLD(lkmer,uint32_t,CT::fnc,e_fkmer)
	FLD(fnode,uint16_t,CT::fnc,e_lkmer)
	FLD(lnode,uint16_t,CT::fnc,e_fnode)
	FLD(parF,uint8_t,CT::fnc,e_lnode)
	FLD(posF,uint8_t,CT::fnc,e_parF)
	FLD(parL,uint8_t,CT::fnc,e_posF)
	FLD(posL,uint8_t,CT::fnc,e_parL)
	FLD(pieF,uint8_t,CT::fnc,e_posL)      // first piece id of candidate i (second = +1), FNOPAR if none
	FLD(pieL,uint8_t,CT::fnc,e_pieF)
	static constexpr uint32_t consmax = MAXCONS;
	static_assert(CT::wide == 0,"the wide tier needs the gw layout");
	FLD(bestL,uint8_t,MAXCONS,e_pieL)      // best consensus so far (survives the tries)
	FLD(cdh,FCC,16,e_bestL)
	static_assert(uA <= o_cdh,"the model table copy (from o_cdh on) is loaded for gap filling while the instance array is live");
	FLD(cseq,uint8_t,18*CT::seqcap,e_cdh)      // stretch sequences of the kept candidates (16 slots) + current + previous
	// dead until the kept candidates are decoded: shared with the lane scratch of the enumerations (lscr: per lane a
	// heap of 32 path ids / of 12 path ids / of PSIQ score intervals; all of it for an enumeration on lane 0 alone)
	FLD(ch,FCC,16,e_cseq)
	FLD(acc,FCC,16,e_ch)
	FLD(accerr,uint32_t,16,e_acc)
	FLD(canderr,uint8_t,16*CT::maxs,e_accerr)
	FLD(consL,uint8_t,16*CT::consrow,e_canderr)   // decoded candidates
	static constexpr uint32_t lscrbytes = static_cast<uint32_t>(CT::lscrids)*static_cast<uint32_t>(sizeof(typename CT::id_t));
	FLD(lscr,uint8_t,lscrbytes,e_cseq)
	FLD(siq,FSI,CT::siqcap,e_cseq)          // score intervals of a pair combined on lane 0
	static_assert(sizeof(FSI)*CT::siqcap <= lscrbytes,"the serial score interval heap shares the lane scratch");
	static constexpr uint32_t pbase = fcmax(e_consL,e_lscr);
	// reverse pool: paths by pool id
	FLD(rc_w,uint64_t,CT::rccap,pbase)
	FLD(rc_parent,typename CT::id_t,CT::rccap,e_rc_w)
	FLD(rc_stretch,uint8_t,CT::rccap,e_rc_parent)
	FLD(rc_pos,uint8_t,CT::rccap,e_rc_stretch)
	FLD(rc_len,uint8_t,CT::rccap,e_rc_pos)
	FLD(rc_baselen,uint8_t,CT::rccap,e_rc_len)
	FLD(rc_acc,typename CT::id_t,CT::rccap,e_rc_baselen)     // accepted paths of an enumeration, in its own slots
	// sorted blocks of the reverse enumerations
	FLD(rc_ord,typename CT::id_t,CT::rccap,e_rc_acc)
	FLD(rc_arw,typename CT::id_t,CT::rccap,e_rc_ord)
	FLD(rc_sbl,uint8_t,CT::rccap,e_rc_arw)         // base length of the i-th entry in sorted order
	FLD(rc_front,uint32_t,CT::rccap,e_rc_sbl)      // front k-mer of the i-th entry in sorted order
	FLD(rbase,uint16_t,CT::fnc+1,e_rc_front)
	FLD(rn,uint16_t,CT::fnc+1,e_rbase)
	FLD(rmaxw,uint64_t,CT::fnc+1,e_rn)
	FLD(rtmask,uint64_t,CT::fnc+1,e_rmaxw)
	FLD(rfmask,uint64_t,CT::fnc+1,e_rtmask)    // one bit per front k-mer (value mod 64) of the accepted reverse paths
	// forward pool: paths by pool id
	FLD(f_w,uint64_t,CT::fcap,e_rfmask)
	FLD(f_parent,typename CT::id_t,CT::fcap,e_f_w)
	FLD(f_stretch,uint8_t,CT::fcap,e_f_parent)
	FLD(f_pos,uint8_t,CT::fcap,e_f_stretch)
	FLD(f_baselen,uint8_t,CT::fcap,e_f_pos)
	FLD(f_len,uint8_t,CT::fcap,e_f_baselen)
	// popped paths of a tree (pop order, in the tree's own slots): path, candidate length, k-mer of its last node, weight
	// minus the junction node
	FLD(fp_id,typename CT::id_t,CT::fcap,e_f_len)
	FLD(fp_cl,uint8_t,CT::fcap,e_fp_id)
	FLD(fp_front,uint32_t,CT::fcap,e_fp_cl)
	FLD(fp_adj,uint64_t,CT::fcap,e_fp_front)
	// per first k-mer candidate: chunk list of its tree, popped paths, junction k-mer bits, scan target bits, heaviest path
	FLD(fchb,uint8_t,8*CT::fnw*(CT::fnc+1),e_fp_adj)   // chunk ids of the forward trees: 8*fnw per first k-mer candidate (+ one exact tree)
	FLD(fnp,uint16_t,CT::fnc+1,e_fchb)
	FLD(ffm,uint64_t,CT::fnc+1,e_fnp)
	FLD(ftm,uint64_t,CT::fnc+1,e_ffm)
	FLD(fmx,uint64_t,CT::fnc+1,e_ftm)
	// recorded (path, entry) sequences of the pairs of a round
	FLD(pout,typename CT::id_t,32*32,e_fmx)
	FLD(poutn,uint8_t,64,e_pout)
	FLD(ctr,uint32_t,4,e_poutn)
	FLD(rchx,uint8_t,32,e_ctr)              // chunk ids of a reverse enumeration on lane 0 alone
	static constexpr uint32_t upool = e_rchx;
	// chunk ids of the reverse enumerations of all last k-mers (32 per lane, lanes < min(fnc,64)): over the per first k-mer tables, which are
	// written after those enumerations have been copied to their blocks
	FLD(rchb,uint8_t,(CT::fnc < 64 ? CT::fnc : 64u)*32,o_fchb)
	static_assert(e_rchb <= o_pout,"reverse chunk lists must fit the per first k-mer tables");
	// raw stretches (overlay of the caches)
	FLD(tfirst,uint16_t,CT::scap,pbase)
	FLD(tlast,uint16_t,CT::scap,e_tfirst)
	FLD(tslen,uint16_t,CT::scap,e_tlast)
	FLD(tlink,uint16_t,CT::scap,e_tslen)
	FLD(skey,uint64_t,fcpow2(CT::scap),e_tlink)
	static constexpr uint32_t uraw = e_skey;
	// final alignment (overlay of the caches)
	FLD(alpv,uint64_t,MAXCONS+1,pbase)
	FLD(almv,uint64_t,MAXCONS+1,e_alpv)
	FLD(albot,uint16_t,MAXCONS+1,e_almv)
	FLD(alops,uint8_t,2*MAXCONS+2*64+8,e_albot)
	static constexpr uint32_t ualn = e_alops;
	static constexpr uint32_t uend = fcmax(fcmax(uA,uraw),fcmax(upool,ualn));
	// scratch behind the build overlay (gap filling)
	FLD(gfbuf,uint64_t,(pbase-uA)/8,uA)
	static constexpr uint32_t gfcap = (pbase-uA)/8;
	// fixed-point model table [pos][row], row stride nrows+1.  It shares the bytes of the enumeration pools: it is
	// (re)loaded from HBM/L2 for gap filling and for the stretch feasibility of a traverse call, both of which are over
	// before the pools are used.
	// feasibility tasks (with the table, dead before the pools are used): first task, first and end start position of
	// every (stretch, direction)
	static constexpr uint32_t taskbytes = ((2*CT::scap+2)*2 + 2*(2*CT::scap) + 15u) & ~15u;
	FLD(toff,uint16_t,2*CT::scap+2,upool-taskbytes)
	FLD(ulo,uint8_t,2*CT::scap,e_toff)
	FLD(uhi,uint8_t,2*CT::scap,e_ulo)
	FLD(tab,uint32_t,(upool-taskbytes-o_cdh)/4,o_cdh)   // also over the candidate buffers, which are dead at that time
	static constexpr uint32_t tabcap = (upool-taskbytes-o_cdh)/4;
	HDEV static uint32_t bytes(uint32_t const, uint32_t const) { return (uend + 15u) & ~15u; }
	// scratch of the stretch construction, the candidate search and the reachability test: borrowed from the weight arrays,
	// which are written after them.  Walk slots (wtmp) of 64 node ids each in front, the walking table behind them.
	static_assert(6u*CT::ncap + 16u <= e_wR1_hi - o_wF_lo,"scratch tables of the stretch walk must fit the weight arrays");
	static_assert(CT::wcap*4 >= CT::ncap*2,"interior node table must fit the weight array it borrows");
	static_assert(2u*CT::ncap + CT::scap + 8u <= 4u*CT::wcap,"reachability scratch must fit the first weight array");
	HDEV LDSQ uint32_t * xcnt32() const { return reinterpret_cast<LDSQ uint32_t *>(base + o_wF_lo); }
	HDEV LDSQ uint16_t * xstep() const { return reinterpret_cast<LDSQ uint16_t *>(base + ((e_wR1_hi - 2u*CT::ncap) & ~7u)); }
	HDEV LDSQ uint16_t * xwtmp() const { return reinterpret_cast<LDSQ uint16_t *>(base + o_wF_lo); }
	static constexpr uint32_t xnslot = (((e_wR1_hi - 2u*CT::ncap) & ~7u) - o_wF_lo) / 128u;
	HDEV LDSQ uint16_t * xsid() const { return reinterpret_cast<LDSQ uint16_t *>(base + o_wR_lo); }
	HDEV LDSQ uint8_t * xspos() const { return reinterpret_cast<LDSQ uint8_t *>(base + o_wR1_lo); }
	HDEV LDSQ uint8_t * xreach() const { return reinterpret_cast<LDSQ uint8_t *>(base + o_wF_lo); }
};

/*
 * gw layout (tier 1 since round 3).  Three regions:
 *   P  live during the whole window: string lengths, support bounds, serial scratch, node keys, fhead, best consensus;
 *   S  results of the build phase that the first phases of a traversal (stretches, candidates, feasibility) and its last
 *      ones (candidate errors, next activation state) need, but not the enumerations and the pairs in between: the
 *      enumeration pools are laid over S, whose bytes are spilled to the workgroup's global slab before the
 *      enumerations and restored after the pairs (two bulk copies of 12 KB per traversal);
 *   X  overlay A (sorted instances, build phase) / overlay B (stretches, candidates, candidate heap, lane scratch).
 * The weights of the feasible (stretch, position) pairs (16 of the 54 KB of the legacy tier 1) live in the global slab,
 * the model table is read from its padded 32 bit copy in global memory (both stay in L1/L2).  The scratch tables of the
 * stretch construction sit in parts of overlay B that are written later (pattern masks: raw stretches; candidate heap,
 * sequences and lane scratch: predecessor counts, walking table, interior nodes, reachability, feasibility tasks).
 */
template<typename CT>
struct FastLds<CT,true>
{
	LDSQ uint8_t * base;
	static constexpr uint32_t keycap = fcpow2(CT::maxs < 2 ? 2 : CT::maxs);
	// (precap need not be a power of two in this layout: the sorts touch only the n keys there are; the padding of the overlap
	// sort at the start of a window is checked against it)
	static_assert(sizeof(typename CT::id_t) > 1 || (CT::fcap <= 256 && CT::rccap <= 256),"pool slots are recorded as id_t (pout)");
	static_assert(CT::blcap <= (FastRows3<CT>::value ? 192u : 128u) && (CT::blcap & 7) == 0,"base length buckets: two 64 bit occupancy words (three in the tier of w = 128, FastRows3), cleared 8 at a time");
	static_assert(CT::lstr == 64 || CT::lstr == 128 || CT::lstr == 256,"the gw layout holds strings of up to 64 bases in one word per pattern mask, of up to 128 in two (round 6), of up to 255 in four (tier 17)");
	static constexpr uint32_t pw = CT::lstr/64;
	static constexpr uint32_t maxlen = CT::lstr < 256u ? static_cast<uint32_t>(CT::lstr) : 255u;      // longest string the layout holds: its length is a byte
	static constexpr bool oneslab = FastOneSlab<CT>::value != 0;      // FastTier<17> / <20>: layout and slab in one buffer, the layout first
	// FastTier<20>, w = 128: three 64 bit words per position mask (model tables of up to 192 rows; w = 128 has 129), rows of 192 symbols for candidates and consensus
	static constexpr bool rows3 = FastRows3<CT>::value != 0;
	static_assert(!rows3 || CT::wide != 0,"three-word position masks extend the two words of a wide tier");
	static constexpr uint32_t maskrows = CT::wide ? (rows3 ? 192u : 128u) : 64u;      // rows of the model table the position masks of a stretch can name
	typedef typename CT::sid_t sid_t;      // stretch ids: 8 bits (at most 250 stretches) or 16 bits
	// more than 256 strings (tier 15): 16 bit node frequencies capped at fqmax, 32 bit first-instance offsets, a 32 byte forward weight record
	static constexpr bool wides = CT::maxs > 256;
	// more than 1024 strings (tier 16): node frequencies up to 4095, 64 instance ranges, 32 bit task offsets
	static constexpr bool xwides = CT::maxs > 1024;
	// more than 2048 strings (tier 18): 256 instance ranges, 15 bit node fields in the stretch sort key
	static constexpr bool ywides = CT::maxs > 2048;
	static constexpr uint32_t fqmax = xwides ? 4095u : (wides ? 1023u : 255u);
	// k-mer instances the layout holds: precap, the capacity of one instance sort -- with more than 256 strings four such ranges, with more than
	// 1024 strings 64 ranges that share eight times precap, with more than 2048 strings 256 ranges that share sixteen times precap (buildInstances).
	// hranges: the ranges are counted by a histogram pass.  The wide tier of more than 256 strings as well: its strings are up to twice as long, and
	// 792 strings of 100 bases have more than precap instances in each of four ranges
	static constexpr bool hranges = xwides || (wides && CT::wide != 0);
	static constexpr uint32_t icap = ywides ? 16u*CT::precap : (hranges ? 8u*CT::precap : (wides ? 4u*CT::precap : CT::precap));
	// (the wide tier of more than 256 strings as well: a traversal of 1300 stretches has 2 x 1300 x up to 128 (stretch, direction, position) tasks)
	static constexpr bool toff32 = xwides || (wides && CT::wide != 0);
	typedef typename FWideSel<toff32,uint32_t,uint16_t>::type toff_t;
	typedef typename FWideSel<wides,uint16_t,uint8_t>::type nfreq_t;
	typedef typename FWideSel<wides,uint32_t,uint16_t>::type nps_t;
	static_assert(fqmax <= (1u << (8u*sizeof(nfreq_t))) - 1u,"a node frequency holds fqmax");
	static_assert(icap <= (sizeof(nps_t) == 2 ? 65535u : 0xFFFFFFFFu),"nps[nn] = npre <= icap must fit a first-instance offset");
	// ---- P ----
	FLD(slen,uint8_t,CT::maxs,0)
	static_assert(maxlen <= 255u,"slen: a string's length is a byte");
	static constexpr uint32_t supcap = CT::wide ? static_cast<uint32_t>(FSUPCAPW) : static_cast<uint32_t>(FSUPCAP);
	FLD(suplo8,uint8_t,supcap,e_slen)
	FLD(suphi8,uint8_t,supcap,e_suplo8)
	FLD(vrem,uint8_t,8,e_suphi8)
	FLD(vadd,uint8_t,8,e_vrem)
	FLD(vapos,uint8_t,8,e_vadd)
	FLD(vfn,uint16_t,8,e_vapos)
	FLD(vln,uint16_t,8,e_vfn)
	FLD(sstack,uint16_t,3*24,e_vln)
	FLD(chain,uint8_t,64,e_sstack)
	FLD(midpar,uint16_t,8,e_chain)          // middle pieces of twice-split stretches: parent stretch, node range [midA,midB]
	FLD(midA,uint8_t,8,e_midpar)
	FLD(midB,uint8_t,8,e_midA)
	FLD(nv,uint32_t,CT::ncap,e_midB)
	FLD(npred,sid_t,CT::ncap,e_nv)
	// longest consensus / candidate of this tier: MAXCONS, 128 in the wide tier (consensus of a window of up to 127 bases), 192 in the tier of w = 128
	static constexpr uint32_t consmax = CT::wide ? (rows3 ? 192u : 128u) : static_cast<uint32_t>(MAXCONS);
	static_assert(!rows3 || 2u + 2u*(DACC_WMAX+2u) + DACC_WMAX + consmax <= static_cast<uint32_t>(WRECW),"the wide record holds the group offsets and the symbols of a window of 128 bases: one symbol per A position and at most consmax consensus symbols");
	static constexpr uint32_t alw = CT::wide ? 2u : 1u;      // 64 bit words per column of the consensus -> A alignment
	FLD(bestL,uint8_t,consmax,e_npred)
	static constexpr uint32_t sbase = (e_bestL + 15u) & ~15u;
	// ---- S (spilled while the pools are live) ----
	// (round 5: no string array -- the pattern masks ARE the strings: symbol c at position p of string j <=> bit p of peq[4*j+c]; they are
	// built by ballots while the bases are gathered and the k-mers are cut from them; the 64 bytes per string went into the node tables)
	FLD(peq,uint64_t,CT::maxs*4*pw,sbase)
	FLD(ipos,uint8_t,icap,e_peq)
	FLD(irpos,uint8_t,icap,e_ipos)
	static_assert(supcap <= 255u && maxlen <= 255u,"ipos / irpos: the position of a k-mer in its string, from either end, is stored as min(position,nsup) <= supcap in a byte");
	FLD(nps,nps_t,CT::ncap+1,e_irpos)
	FLD(nfreq,nfreq_t,CT::ncap,e_nps)
	FLD(succ0,uint16_t,CT::ncap,e_nfreq)
	FLD(sinfo,uint16_t,CT::ncap,e_succ0)
	FLD(nrange,uint32_t,CT::ncap,e_sinfo)
	FLD(mfirst,uint64_t,keycap,e_nrange)
	FLD(mlast,uint64_t,keycap,e_mfirst)
	static constexpr uint32_t send = (e_mlast + 15u) & ~15u;
	static constexpr uint32_t sbytes = send - sbase;
	// ---- enumeration pools: overlay of S ----
	FLD(rc_w,uint64_t,CT::rccap,sbase)
	FLD(rc_parent,typename CT::id_t,CT::rccap,e_rc_w)
	FLD(rc_stretch,sid_t,CT::rccap,e_rc_parent)
	FLD(rc_pos,uint8_t,CT::rccap,e_rc_stretch)
	FLD(rc_len,uint8_t,CT::rccap,e_rc_pos)
	FLD(rc_baselen,uint8_t,CT::rccap,e_rc_len)
	FLD(rc_acc,typename CT::id_t,CT::rccap,e_rc_baselen)
	FLD(rc_ord,typename CT::id_t,CT::rccap,e_rc_acc)
	FLD(rc_arw,typename CT::id_t,CT::rccap,e_rc_ord)
	FLD(rc_sbl,uint8_t,CT::rccap,e_rc_arw)
	FLD(rc_front,uint32_t,CT::rccap,e_rc_sbl)
	FLD(rbase,uint16_t,CT::fnc+1,e_rc_front)
	FLD(rn,uint16_t,CT::fnc+1,e_rbase)
	FLD(rmaxw,uint64_t,CT::fnc+1,e_rn)
	FLD(rtmask,uint64_t,CT::fnc+1,e_rmaxw)
	FLD(rfmask,uint64_t,CT::fnc+1,e_rtmask)
	FLD(f_w,uint64_t,CT::fcap,e_rfmask)
	FLD(f_parent,typename CT::id_t,CT::fcap,e_f_w)
	FLD(f_stretch,sid_t,CT::fcap,e_f_parent)
	FLD(f_pos,uint8_t,CT::fcap,e_f_stretch)
	FLD(f_baselen,uint8_t,CT::fcap,e_f_pos)
	FLD(f_len,uint8_t,CT::fcap,e_f_baselen)
	FLD(fp_id,typename CT::id_t,CT::fcap,e_f_len)
	FLD(fp_cl,uint8_t,CT::fcap,e_fp_id)
	FLD(fp_front,uint32_t,CT::fcap,e_fp_cl)
	FLD(fp_adj,uint64_t,CT::fcap,e_fp_front)
	FLD(fchb,uint8_t,8*CT::fnw*(CT::fnc+1),e_fp_adj)
	FLD(fnp,uint16_t,CT::fnc+1,e_fchb)
	FLD(ffm,uint64_t,CT::fnc+1,e_fnp)
	FLD(ftm,uint64_t,CT::fnc+1,e_ffm)
	FLD(fmx,uint64_t,CT::fnc+1,e_ftm)
	FLD(pout,typename CT::id_t,32*32,e_fmx)
	FLD(poutn,uint8_t,64,e_pout)
	FLD(ctr,uint32_t,4,e_poutn)
	FLD(rchx,uint8_t,32,e_ctr)
	static constexpr uint32_t upool = e_rchx;
	// (pools larger than the build-phase arrays run on into a gap in front of the overlays: tier 3, whose reverse pool is sized
	// for the 72 last k-mer candidates of a 54x pile -- 256 chunks of 8 paths, the most an 8 bit chunk id can name)
	FLD(rchb,uint8_t,(CT::fnc < 64 ? CT::fnc : 64u)*32,o_fchb)
	static_assert(e_rchb <= o_pout,"reverse chunk lists must fit the per first k-mer tables");
	static constexpr uint32_t ubase = fcmax(send,(upool + 15u) & ~15u);
	// ---- overlay A: build phase ----
	FLD(pre,uint64_t,icap,ubase)
	FLD(lastk,uint64_t,keycap,e_pre)
	static constexpr uint32_t uA = e_lastk;
	// ---- overlay B: traversal ----
	FLD(sfirst,uint16_t,CT::scap,ubase)
	FLD(slast,uint16_t,CT::scap,e_sfirst)
	FLD(sslen,uint16_t,CT::scap,e_slast)
	FLD(slink,uint16_t,CT::scap,e_sslen)
	FLD(maskF,uint64_t,CT::scap,e_slink)
	FLD(maskR,uint64_t,CT::scap,e_maskF)
	FLD(maskFh,uint64_t,(CT::wide ? CT::scap : 0u),e_maskR)      // wide tier: start positions 64 ... 127
	FLD(maskRh,uint64_t,(CT::wide ? CT::scap : 0u),e_maskFh)
	FLD(maskFx,uint64_t,(rows3 ? CT::scap : 0u),e_maskRh)      // tier of w = 128: start positions 128 ... 191 (the table of w = 128 has row 128)
	FLD(maskRx,uint64_t,(rows3 ? CT::scap : 0u),e_maskFx)
	FLD(woffF,toff_t,CT::scap,e_maskRx)      // (toff_t: 16 bits, wcap <= 65535; more than 1024 strings: 32 bits)
	FLD(woffR,toff_t,CT::scap,e_woffF)
	static_assert(sizeof(toff_t) == 4 || CT::wcap <= 65535u,"weight offsets of 16 bits");
	FLD(links,uint16_t,CT::lcap,e_woffR)
	FLD(lhead,sid_t,CT::ncap,e_links)
	FLD(lord,uint32_t,CT::scap,e_lhead)
	FLD(ppos,sid_t,CT::scap,e_lord)
	FLD(fkmer,uint32_t,CT::fnc,e_ppos)
	FLD(lkmer,uint32_t,CT::fnc,e_fkmer)
	FLD(fnode,uint16_t,CT::fnc,e_lkmer)
	FLD(lnode,uint16_t,CT::fnc,e_fnode)
	FLD(parF,sid_t,CT::fnc,e_lnode)
	FLD(posF,uint8_t,CT::fnc,e_parF)
	FLD(parL,sid_t,CT::fnc,e_posF)
	FLD(posL,uint8_t,CT::fnc,e_parL)
	FLD(pieF,sid_t,CT::fnc,e_posL)
	FLD(pieL,sid_t,CT::fnc,e_pieF)
	static constexpr uint32_t xbase = (e_pieL + 15u) & ~15u;
	FLD(cdh,FCC,16,xbase)
	FLD(cseq,sid_t,18*CT::seqcap,e_cdh)
	FLD(ch,FCC,16,e_cseq)
	FLD(acc,FCC,16,e_ch)
	FLD(accerr,uint32_t,16,e_acc)
	FLD(canderr,uint8_t,16*CT::maxs,e_accerr)
	static_assert(fcmax(maxlen,CT::consrow) <= 255u,"canderr: the error of a candidate against one string is at most max(string,candidate), a byte");
	FLD(consL,uint8_t,16*CT::consrow,e_canderr)
	static constexpr uint32_t lscrbytes = static_cast<uint32_t>(CT::lscrids)*static_cast<uint32_t>(sizeof(typename CT::id_t));
	FLD(lscr,uint8_t,lscrbytes,e_cseq)
	FLD(siq,FSI,CT::siqcap,e_cseq)
	static_assert(sizeof(FSI)*CT::siqcap <= lscrbytes,"the serial score interval heap shares the lane scratch");
	// (the scratch tables of the stretch construction need 3 bytes per node: the region is at least that long)
	static constexpr uint32_t alnbytes = 2u*8u*alw*(consmax+1u) + 2u*(consmax+1u) + 8u + (2u*consmax + 2u*64u + 8u) + 16u;      // alpv, almv, albot, alops
	static constexpr uint32_t uB = fcmax(fcmax(fcmax(fcmax(e_consL,e_lscr),xbase + 3u*CT::ncap + 16u),xbase + (2u*CT::scap+2u)*static_cast<uint32_t>(sizeof(toff_t)) + 8u + 8u*CT::scap + 16u),CT::wide ? xbase + alnbytes : 0u);
	static constexpr uint32_t xbytes = uB - xbase;
	// raw stretches: over the pattern masks and weight offsets, which the feasibility writes later
	FLD(tfirst,uint16_t,CT::scap,o_maskF)
	FLD(tlast,uint16_t,CT::scap,e_tfirst)
	FLD(tslen,uint16_t,CT::scap,e_tlast)
	FLD(tlink,uint16_t,CT::scap,e_tslen)
	FLD(skey,uint64_t,fcpow2(CT::scap),e_tlink)
	static_assert(e_skey <= o_links,"raw stretches must fit the mask / offset arrays they borrow");
	// scratch over [xbase,uB): candidate heap, sequences and lane scratch are written by the enumerations only
	FLD(alpv,uint64_t,alw*(consmax+1),xbase)
	FLD(almv,uint64_t,alw*(consmax+1),e_alpv)
	FLD(albot,uint16_t,consmax+1,e_almv)
	FLD(alops,uint8_t,2*consmax+2*64+8,e_albot)
	static_assert(e_alops <= uB,"final alignment scratch");
	FLD(toff,toff_t,2*CT::scap+2,xbase)
	FLD(urec,uint32_t,2*CT::scap,e_toff)      // unit at position q of the processing order: lo | unit << 7
	static_assert(e_urec <= uB,"feasibility tasks");
	static_assert(3u*CT::ncap + 16u <= xbytes,"predecessor counts (a byte per node) and walking table must fit the scratch");
	static_assert(3u*CT::ncap + 16u <= xbytes && 2u*CT::ncap + CT::scap + 8u <= xbytes,"interior node table / reachability scratch");
	HDEV LDSQ uint32_t * xcnt32() const { return reinterpret_cast<LDSQ uint32_t *>(base + xbase); }
	HDEV LDSQ uint16_t * xstep() const { return reinterpret_cast<LDSQ uint16_t *>(base + xbase + ((CT::ncap + 3u) & ~3u) + 8u); }
	HDEV LDSQ uint16_t * xsid() const { return reinterpret_cast<LDSQ uint16_t *>(base + xbase); }
	HDEV LDSQ uint8_t * xspos() const { return reinterpret_cast<LDSQ uint8_t *>(base + xbase + 2u*CT::ncap + 8u); }
	HDEV LDSQ uint8_t * xreach() const { return reinterpret_cast<LDSQ uint8_t *>(base + xbase); }
	// (more than 256 strings: the instances as they are generated, before they are split into the four sorted ranges of `pre`; behind both overlays)
	FLD(pregen,uint64_t,(wides ? icap : 0u),((fcmax(uA,uB) + 15u) & ~15u))
	// scratch behind the build overlay (gap filling): small in this layout, a window that needs more goes to the next tier
	// (one-slab tier: nothing comes behind it but the generic engine, and the windows of noisy sequence that carry its long strings reach filter frequency 0
	// more often than others -- a region of its own behind both overlays, 16384 records and as many candidates; where the build overlay is the longer
	// one, as in tiers 14 and 17, the shared scratch has no room at all)
	static constexpr uint32_t gfown = (oneslab && !wides) ? 32768u : 0u;
	FLD(gfbuf,uint64_t,(gfown ? gfown : (uB > uA ? (uB-uA)/8 : 0u)),(gfown ? ((fcmax(uA,uB) + 15u) & ~15u) : uA))
	static constexpr uint32_t gfcap = gfown ? gfown : (uB > uA ? (uB-uA)/8 : 0u);
	static constexpr uint32_t uend = wides ? e_pregen : (gfown ? e_gfbuf : fcmax(uA,uB));
	static constexpr uint32_t tabcap = 0x7FFFFFFFu;      // no LDS copy of the model table
	HDEV static uint32_t bytes(uint32_t const, uint32_t const) { return (uend + 15u) & ~15u; }
	// the global slab of a workgroup: forward weights, reverse weights (16 bytes per entry), spill of S; the walk slots of
	// the stretch construction borrow the weight part
	// (round 4) behind the spill image: the sorted k-mer instances and last k-mers of the current k, saved before the first
	// traversal of a pass overwrites overlay A, so that the next filter frequency pass reloads them instead of sorting again
	// (wides: the forward record is 32 bytes -- three 64 bit weights --, the reverse record stays 16)
	static constexpr uint32_t recFbytes = wides ? 32u : 16u;
	static constexpr uint32_t g_wF = 0, g_wR = recFbytes*CT::wcapg, g_spill = (recFbytes+16u)*CT::wcapg, g_inst = ((g_spill + sbytes + 255u) & ~255u),
		g_bytes = g_inst + (((icap + keycap)*8u + 255u) & ~255u);
	static_assert((o_pre & 15u) == 0 && (icap & 1u) == 0 && (keycap & 1u) == 0,"instance arrays are saved 16 bytes at a time");
	static constexpr uint32_t xnslot = g_spill / 128u;
	// device-memory tiers (CT::gmem): this layout itself sits behind the instance image, g_total bytes per workgroup in all
	static constexpr uint32_t g_layout = g_bytes, g_total = CT::gmem ? g_bytes + ((((uend + 15u) & ~15u) + 255u) & ~255u) : g_bytes;
	// one-slab tiers (FastTier<17>::oneslab): the layout comes FIRST -- base is the first byte of the workgroup's buffer -- and the g_* part follows it at g_base
	// (processWindowFast: E.gslab = base + g_base); the buffer has the same g_total bytes
	static constexpr uint32_t g_base = oneslab ? ((((uend + 15u) & ~15u) + 255u) & ~255u) : 0u;
	static_assert(!oneslab || CT::gmem != 0,"a one-slab tier is a device-memory tier");
};
#undef FLD

template<typename CT>
HDEV FastCaps fastCapsOf(uint32_t const nrows, uint32_t const nsup)
{
	FastCaps C;
	C.maxs = CT::maxs; C.precap = FastLds<CT>::icap; C.ncap = CT::ncap; C.scap = CT::scap; C.lcap = CT::lcap; C.wcap = CT::wcap; C.rccap = CT::rccap;
	C.fcap = CT::fcap; C.siqcap = CT::siqcap; C.blcap = CT::blcap;
	C.nrows = nrows; C.nsup = nsup;
	C.ldsbytes = FastLds<CT>::bytes(nrows,nsup);
	C.tabcap = FastLds<CT>::tabcap;
	if constexpr ( CT::gw != 0 ) C.gbytes = FastLds<CT>::g_total; else C.gbytes = 0;
	if constexpr ( FastOneSlab<CT>::value != 0 ) C.ldsbytes = C.gbytes;      // one buffer: layout, then weights, spill image, instance image
	C.gmem = CT::gmem;
	static_assert(CT::gmem == 0 || CT::gw != 0,"a layout in device memory is the gw layout");
	return C;
}
}
#endif
