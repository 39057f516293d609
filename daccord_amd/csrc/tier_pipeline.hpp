/*
 * The pipeline of LDS capacity tiers of the window stage, once and as data (host only, plain C++17: the planner, the launches
 * of capi.hip and the CPU emulation of the tests all read it from here).
 *
 * Every window runs through a chain of tiers (FastTier<N>, fast_tiers.hpp); which tiers, in which order, depends on the batch:
 *
 *   shallow batches   slot 0: 0 -> 7 -> 1     slot 1: 6     slot 2: 10 -> 12 -> 3
 *   deep batches      slot 0: 4               slot 1: 2     slot 2: 11 -> 12 -> 3
 *   wide batches                              slot 1: 8     slot 2: 9
 *   shallow and deep  tier 5 on the second stream (k_window_long), in front of the generic engine there
 *   wide batches      the LONG STRING stage on the second stream: tier 17 (strings of 129 ... 255 bases, layout in device memory), in front of the generic engine there
 *   w = 128           ONE stage, tier 20 (three words per position mask: the model table has 129 rows; strings of up to 255 bases, layout in device memory), over every window
 *                     of the batch, in front of the generic engine; no slot, no trailing stage and no second stream run there
 *   every other batch the TRAILING stages, each once, behind the slots and in front of the generic engine: tier 13 (shallow, deep) / tier 14 (wide), then in
 *                     shallow and deep batches tier 15, tier 16 and tier 18 and in wide batches tier 19, each only in a batch with a window deep enough for it
 *
 * (TIER_CHAIN below: one row per stage, one column per batch shape.)
 *
 * A slot is one entry of dacc_timing.tier_ms[3] / tier_out[3].  Its MAIN tier takes what the slot in front handed on (slot 0: all
 * windows) and hands on to the next slot, the last one to the generic engine.  FRONT tiers run before the main tier of their slot
 * with more wavefronts per CU: each hands on to the next stage of its slot.  Tiers 0 and 7 are fed by the size-class pre-pass
 * (k_classify), tiers 10 / 11 by the list of the slot in front, tier 12 (windows of 97 ... 250 strings; it passes the others on) by what they hand on.
 *
 * A TRAILING stage (ROLE_LAST) is no slot: its tier keeps the layout FastLds<CT> in a slab of device memory per workgroup instead of LDS (FastCaps::gmem),
 * with tables no CU's LDS could hold.  It reads the list the nearest stage in front of it that ran handed on -- a trailing stage, else the last enabled
 * slot -- and hands on to the next one, the last to the generic engine (k_window), which recomputes both enumerations for every (first, last) k-mer
 * pair and is two to three orders of magnitude slower per window.  It does not run when no slot runs.  Its row of TIER_CHAIN names its two switches and
 * its threshold: DACC_*_TIER=0 removes it (the chain as it was before the stage); its slab is allocated and its kernel launched only in a batch whose
 * deepest window has more strings than the threshold (resolveTiers: maxstrings), so every other batch runs the launches it ran before the stage existed;
 * DACC_*_AS_SLOT2=1 (tests, A/B timing) makes its tier the main tier of the third slot instead, with the slot's front tiers still in front of it, and
 * switches the stage off: the planner, the launches and the emulation harness then run the device-memory tier as an ordinary slot.  Each of these names
 * the third slot's main tier, so more than one of them is an error (TierSwitches::conflict).
 *
 *   stage      tier                        its windows                                        =0 removes it     =1: the third slot's main tier            threshold
 *   ID_LAST    13 (shallow, deep) / 14     what overflowed a table of the slots, up to 250    DACC_LAST_TIER    DACC_LAST_AS_SLOT2 (13 for 3, 14 for 9)   0: every batch
 *              (wide)                      strings
 *   ID_VDEEP   15 (shallow, deep)          251 ... 1000 strings, which every tier in front    DACC_VDEEP_TIER   DACC_VDEEP_AS_SLOT2 (a wide batch keeps   VDEEP_MINS = 250
 *                                          refuses at its string count; others passed on                        tier 9)
 *   ID_XDEEP   16 (shallow, deep)          1001 ... 2000 strings, and those of 251 ... 1000   DACC_XDEEP_TIER   DACC_XDEEP_AS_SLOT2 (a wide batch keeps   XDEEP_MINS = 1000
 *                                          that overflowed a table of tier 15; those of at                      tier 9)
 *                                          most 250 passed on
 *   ID_FDEEP   18 (shallow, deep)          2001 ... 5001 strings (the deepest window of a     DACC_FDEEP_TIER   DACC_FDEEP_AS_SLOT2 (a wide batch keeps   FDEEP_MINS = 2000
 *                                          default run), and those of 251 ... 2000 that                             tier 9)
 *                                          overflowed a table of tier 16; those of at most
 *                                          250 passed on
 *   ID_WDEEP   19 (wide)                   251 ... 1000 strings of a wide batch, which tiers  DACC_WDEEP_TIER   DACC_WDEEP_AS_SLOT2 (19 for 9; a shallow  VDEEP_MINS = 250
 *                                          8, 9 and 14 refuse at their string count; those                      or deep batch keeps tier 3)
 *                                          of at most 250 passed on
 *
 * The stage of w = 128 (ID_W128, ROLE_ALONE) runs tier 20 -- tier 17 with three words per position mask, rows of 192 symbols and tier 19's reverse pool -- over every window of a batch
 * with a window of 128 bases, with a kernel of its own, k_window_fast<20>, a hand-on list and a slab of its own (optional like a trailing stage's), and k_window runs what it hands on:
 * more than 250 strings, a string of more than 255 bases, a table that overflowed.  DACC_W128_TIER=0 removes it: such a batch is the generic engine alone, as before the stage.
 * DACC_W128_AS_SLOT2=1 (tests) makes tier 20 the third slot's main tier and the second stream's tier of such a batch instead and switches the stage off: a harness that walks the
 * three slots and ROLE_LONG then runs every window in the tier, those with a string of more than 128 bases through the second stream's path.  It counts in TierSwitches::conflict.
 *
 * The LONG STRING stage (ID_LONG in a wide batch, ROLE_LONG) runs tier 17 -- tier 14 with four words per pattern mask, strings of up to 255 bases -- over the
 * two lists of the second stream (the pre-scan's: a B string of more than 128 bases; the first tier's generic-only windows) with a kernel of its own,
 * k_window_fast<17>, in front of k_window_long, which then runs the generic engine alone over what the tier handed on (a string of more than 255 bases,
 * a table that overflowed).  Its slab is allocated and its kernel launched only for a list that is not empty.  DACC_LONGSTR_TIER=0 removes it: a wide
 * batch's second stream is then the generic engine alone, as before the stage.  Shallow and deep batches keep tier 5 inside k_window_long.
 */
#ifndef DACC_TIER_PIPELINE_HPP
#define DACC_TIER_PIPELINE_HPP
#include <cstdint>
#include <cstdlib>
#include <algorithm>

namespace dacc {

// run time description of a capacity tier (host planning, launch parameters)
struct FastCaps
{
	uint32_t maxs, precap, ncap, scap, lcap, wcap, rccap, fcap, siqcap, blcap;
	uint32_t tabcap;             // 32-bit words the table overlay of this tier can hold
	uint32_t nrows, nsup;        // dimensions of the fixed-point table copy held in LDS
	uint32_t ldsbytes;
	uint32_t gbytes;             // gw tiers: bytes of global scratch per workgroup (0: none); with gmem: the layout (ldsbytes, at gbytes - its rounded size) included
	uint32_t gmem;               // 1: the layout lives in the workgroup's slab in device memory -- no LDS requested, no 160 KiB gate; ldsbytes stays the layout's size
};
enum { FSUPCAP = 128, FSUPCAPW = 192 };      // max width (read offsets) of the model table copy in LDS (W: the wide tiers -- the table of w = 127 covers 165 read offsets)
enum : uint32_t { T0INST_DEFAULT = 576, T7INST_DEFAULT = 704 };      // a window with more k-mer instances (upper bound of the pre-pass) starts in tier 7 / tier 1; run-time
                                               // arguments of the pre-pass (DACC_T0INST / DACC_T7INST override them for sweeps)

// The tiers.  KERNEL: those with a kernel of their own (k_window_fast<N>, window_kernels.hpp); tier 5 runs inside k_window_long.
#define DACC_KERNEL_TIERS(X) X(0) X(1) X(2) X(3) X(4) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19)
#define DACC_ALL_TIERS(X) DACC_KERNEL_TIERS(X) X(5)
// (the two lists above are the tiers whose layout sizes are recorded, tests/golden/fast_layout_sizes.txt: one line per tier of DACC_ALL_TIERS.  A tier added since has a
// kernel of its own like those of DACC_KERNEL_TIERS and stands in a list of its own, with its own recorded line -- tier 20: tests/golden/w128_layout_sizes.txt.  Whatever
// walks every kernel tier walks DACC_EVERY_KERNEL_TIER, whatever walks every tier DACC_EVERY_TIER)
#define DACC_W128_TIERS(X) X(20)
#define DACC_EVERY_KERNEL_TIER(X) DACC_KERNEL_TIERS(X) DACC_W128_TIERS(X)
#define DACC_EVERY_TIER(X) DACC_ALL_TIERS(X) DACC_W128_TIERS(X)

// From a run-time tier number to its compile-time capacities: f is called with a TierTag<N>, whose `type` is FastTier<N>
template<int TIER> struct FastTier;
template<int TIER> struct TierTag { typedef FastTier<TIER> type; };
template<typename F> static inline auto withTier(uint32_t const tier, F && f) -> decltype(f(TierTag<0>()))
{
#define DACC_TIER_CASE(N) case N: return f(TierTag<N>());
	switch ( tier ) { DACC_EVERY_TIER(DACC_TIER_CASE) }
#undef DACC_TIER_CASE
	std::abort();
}

enum TierRole { ROLE_FRONT, ROLE_MAIN, ROLE_LONG, ROLE_LAST, ROLE_ALONE };      // front tier of a slot, the slot's main tier, tier 5 / tier 17 on the second stream, the device-memory tier behind the slots, the one stage of a batch no slot runs in (w = 128)
// What switches a stage off, beside its bit of DACC_TIERS, its LDS size (at most the 160 KiB of a CU) and a batch shape it has no tier
// for (TIER_NONE: "not in a wide batch", "not in a deep batch").  A front tier also needs the main tier of its slot.
enum : uint32_t
{
	GATE_TABFIT = 1,      // the tier's table overlay must hold the model table: (nrows+1)*(nsup+1) <= tabcap
	GATE_PREV_FRONT = 2,  // needs the front tier before it (tier 7 needs tier 0)
	GATE_T7_ABOVE_T0 = 4, // only with DACC_T7INST > DACC_T0INST (else the middle size class is empty)
	GATE_DENSE = 8,       // DACC_DENSE_TIER=0 switches it off
	GATE_PREV_SLOT = 16,  // needs the main tier of the slot in front as well (the dense tiers need slots 1 and 2)
	GATE_DEEP = 128,      // DACC_DEEP_TIER=0 switches it off (windows of more than 96 strings run in the generic engine, as before the deep-window tier)
	GATE_TRAILING = 256,  // a trailing stage: its row's DACC_*_TIER=0 or DACC_*_AS_SLOT2=1 switches it off; needs a slot that ran and a window of more strings than its row's minstrings in the batch
	GATE_ALONE = 512,     // the stage of a w = 128 batch: its row's DACC_*_TIER=0 or DACC_*_AS_SLOT2=1 switches it off; needs no slot (none runs there)
	GATE_LONGSTR = 2048,  // DACC_LONGSTR_TIER=0 switches it off in a wide batch (the second stream of a wide batch is then the generic engine alone); no gate in the other shapes
	STAGE_PREPASS = 32,   // (no gate) fed by the size-class pre-pass instead of the list in front of it
	STAGE_ADAPTIVE = 64   // (no gate) switches itself off for the rest of a context when it hands on too much (DACC_T7_ADAPT)
};
// counters of d_work (32 bit words): eight per-XCD work counters for every kernel that pulls its windows (window_kernels.hpp: next_window)
enum : uint32_t { WORK_SLOT0 = 0, WORK_SLOT1 = 8, WORK_SLOT2 = 16, WORK_DENSE = 24, WORK_GENERIC = 32, WORK_T0 = 40, WORK_T7 = 48,
	WORK_PRE_MID = 56, WORK_PRE_BIG = 57,      // what the pre-pass itself put on the middle and the big list (for dacc_timing)
	WORK_TRACE = 60, WORK_DEEP = 64,
	WORK_DEEP_COUNT = 72,      // two words: windows of more than FastTier<12>::mins strings the deep-window tier read / handed on (for dacc_timing)
	WORK_LAST = 80, WORK_VDEEP = 88,
	WORK_VDEEP_COUNT = 96,     // two words: windows of more than VDEEP_MINS strings the very deep stage read / handed on (for dacc_timing)
	WORK_XDEEP = 104,
	WORK_XDEEP_COUNT = 112,    // two words: windows of more than VDEEP_MINS strings the deepest stage read / handed on (for dacc_timing)
	WORK_FDEEP = 120,
	WORK_FDEEP_COUNT = 128,    // two words: windows of more than VDEEP_MINS strings the full-depth stage read / handed on (for dacc_timing)
	WORK_WDEEP = 136,
	WORK_WDEEP_COUNT = 144,    // two words: windows of more than VDEEP_MINS strings the wide deep stage read / handed on (for dacc_timing)
	// (everything above is the first stream's and cleared at the start of every pass; the second stream clears what follows in front of its launches)
	WORK_LONGSTR = 152,        // the long string stage's launch over the pre-scan list, WORK_LONGSTR + 8: its launch over the first tier's generic-only list
	WORK_W128 = 168,           // the stage of a w = 128 batch (no slot, no second stream there: cleared with the whole array in front of its launch)
	WORK_WORDS = 176 };

// The stages, in the order they run (ID_FDEEP runs behind ID_XDEEP and ID_WDEEP behind that: the trailing stages run in the order of their rows, and no row between them is one; in a
// wide batch ID_WDEEP stands directly behind ID_LAST, the rows between them have no wide tier); their
// place in this table is their place in BatchPlan::stageCaps, TierPipeline and dacc_ctx::st.  TIER_NSTAGES counts the rows up to ID_LONG, which is what a caller
// that holds one capacity record per stage in an array of TIER_NSTAGES walks (the emulation harness, tests/tiers/tier_resolution.cpp and its recording of one
// column per stage); the rows added since stand behind it, TIER_NROWS counts all, and resolveTiers resolves them for a caller that says it holds them (`rows`).
enum TierId { ID_T0, ID_T7, ID_SLOT0, ID_SLOT1, ID_DENSE, ID_DEEP, ID_SLOT2, ID_LAST, ID_VDEEP, ID_XDEEP, ID_LONG, TIER_NSTAGES, ID_FDEEP = TIER_NSTAGES, ID_WDEEP, ID_W128, TIER_NROWS };
enum { TIER_NSLOTS = 3, TIER_NONE = 255, TIER_SHALLOW_FIRST = 1 };      // (the first slot's main tier of shallow batches: a batch whose windows mostly overflow its strings / instances is deep)
enum : uint32_t { VDEEP_MINS = 250 };      // the very deep stage takes the windows with more strings than this (= FastTier<15>::mins = FastTier<13>::maxs; fast_tiers.hpp asserts this and the two below)
enum : uint32_t { XDEEP_MINS = 1000 };     // the deepest stage is resolved for a batch with a window of more strings than this (= FastTier<15>::maxs); its tier takes what has more than VDEEP_MINS
enum : uint32_t { FDEEP_MINS = 2000 };     // the full-depth stage is resolved for a batch with a window of more strings than this (= FastTier<16>::maxs); its tier takes what has more than VDEEP_MINS
enum : uint64_t { TIER_GMEM_SLAB = 256ull << 20 };      // device memory the slabs of a device-memory tier's workgroups take together (tierGridGmem below)
// The wide deep stage's budget: tier 19's slab is 8 884 992 B per workgroup, 24 workgroups in 256 MiB -- measured on an MI355X, 24 wavefronts are slower than the wavefront per
// window k_window gives the same windows (profiles/wdeep_measurements.md).  2 GiB hold 240 workgroups, about one per CU; a batch that has such windows is one whose generic
// engine asks for arenas of 200 MB per wavefront.  The slab is allocated for the grid, a workgroup per window of the batch up to that, and is optional like the others.
enum : uint64_t { WDEEP_GMEM_SLAB = 2048ull << 20 };
struct TierStage
{
	uint8_t tier[3] /* in a shallow, deep, wide batch */, slot, role; int8_t tiersbit /* bit of DACC_TIERS */; uint32_t flags, work;
	// a trailing stage (ROLE_LAST) only
	char const * offswitch = nullptr;      // DACC_*_TIER: 0 removes the stage
	char const * slot2switch = nullptr;    // DACC_*_AS_SLOT2: 1 makes its tier the main tier of the third slot and switches the stage off
	uint32_t minstrings = 0;               // resolved only for a batch whose deepest window has more strings than this (0: every batch)
	bool slot2wide = false;                // does its AS_SLOT2 switch apply to a wide batch (else that keeps tier 9)
	bool slot2narrow = true;               // does it apply to a shallow or deep batch (else that keeps tier 3)
	uint64_t slab = 0;                     // bytes of device memory its workgroups' slabs may take together (0: TIER_GMEM_SLAB)
	uint32_t onlyw = 0;                    // the row (its stage and its AS_SLOT2 switch) is for batches of this window size alone (0: any)
};
#if !defined(DACC_W128_SLAB_MB)
#define DACC_W128_SLAB_MB 1024
#endif
// The budget of the stage of w = 128: tier 20's slab is 1 788 416 B per workgroup, 144 workgroups in the common 256 MiB -- and the stage runs EVERY window of its batch:
// measured on an MI355X, 300 reads of 10 kb (92 988 windows) take 14.4 s with 144 workgroups and 3.8 s with the 600 of 1 GiB (profiles/w128_measurements.md).  The slab is
// allocated for the grid, a workgroup per window of the batch up to that, and is optional like the others
enum : uint64_t { W128_GMEM_SLAB = static_cast<uint64_t>(DACC_W128_SLAB_MB) << 20 };
enum : uint32_t { W128 = 128 };      // the window size whose model table has 129 rows: three words per position mask (FastTier<20>)
// an environment switch: set to 0 (a default that is on), set to 1 (a default that is off), a number
static inline bool envOff(char const * const name) { char const * const e = getenv(name); return e && e[0] == '0'; }
static inline bool envOn(char const * const name) { char const * const e = getenv(name); return e && e[0] == '1'; }
static inline uint32_t envNum(char const * const name, uint32_t const dflt) { char const * const e = getenv(name); return e ? static_cast<uint32_t>(atoi(e)) : dflt; }
static TierStage const TIER_CHAIN[TIER_NROWS] = {
	{ { 0, TIER_NONE, TIER_NONE }, 0, ROLE_FRONT, 3, STAGE_PREPASS, WORK_T0 },
	{ { 7, TIER_NONE, TIER_NONE }, 0, ROLE_FRONT, 4, STAGE_PREPASS|STAGE_ADAPTIVE|GATE_PREV_FRONT|GATE_T7_ABOVE_T0, WORK_T7 },
	{ { 1, 4, TIER_NONE }, 0, ROLE_MAIN, 0, GATE_TABFIT, WORK_SLOT0 },
	{ { 6, 2, 8 }, 1, ROLE_MAIN, 1, GATE_TABFIT, WORK_SLOT1 },
	{ { 10, 11, TIER_NONE }, 2, ROLE_FRONT, -1, GATE_TABFIT|GATE_DENSE|GATE_PREV_SLOT, WORK_DENSE },
	{ { 12, 12, TIER_NONE }, 2, ROLE_FRONT, -1, GATE_TABFIT|GATE_DEEP|GATE_PREV_SLOT, WORK_DEEP },
	{ { 3, 3, 9 }, 2, ROLE_MAIN, 2, GATE_TABFIT, WORK_SLOT2 },
	{ { 13, 13, 14 }, 2, ROLE_LAST, -1, GATE_TABFIT|GATE_TRAILING, WORK_LAST, "DACC_LAST_TIER", "DACC_LAST_AS_SLOT2", 0, true },
	{ { 15, 15, TIER_NONE }, 2, ROLE_LAST, -1, GATE_TABFIT|GATE_TRAILING, WORK_VDEEP, "DACC_VDEEP_TIER", "DACC_VDEEP_AS_SLOT2", VDEEP_MINS, false },
	{ { 16, 16, TIER_NONE }, 2, ROLE_LAST, -1, GATE_TABFIT|GATE_TRAILING, WORK_XDEEP, "DACC_XDEEP_TIER", "DACC_XDEEP_AS_SLOT2", XDEEP_MINS, false },
	// (tier 5 holds no wide window and no string of more than 128 bases: a wide batch's second stream runs tier 17, a kernel of its own over a slab in device
	// memory, and the generic engine behind it)
	{ { 5, 5, 17 }, 0, ROLE_LONG, 2, GATE_TABFIT|GATE_LONGSTR, WORK_LONGSTR },
	// (behind TIER_NSTAGES; it runs behind ID_XDEEP)
	{ { 18, 18, TIER_NONE }, 2, ROLE_LAST, -1, GATE_TABFIT|GATE_TRAILING, WORK_FDEEP, "DACC_FDEEP_TIER", "DACC_FDEEP_AS_SLOT2", FDEEP_MINS, false },
	// (the wide batches' very deep stage: behind ID_LAST's tier 14 there.  The wide column of ID_VDEEP stays empty: a caller that walks TIER_NSTAGES rows resolves what it resolved)
	{ { TIER_NONE, TIER_NONE, 19 }, 2, ROLE_LAST, -1, GATE_TABFIT|GATE_TRAILING, WORK_WDEEP, "DACC_WDEEP_TIER", "DACC_WDEEP_AS_SLOT2", VDEEP_MINS, true, false, WDEEP_GMEM_SLAB },
	// (a batch of w = 128: no slot, no trailing stage and no second stream run there -- the stage takes every window of the batch and hands on to the generic engine.
	// DACC_W128_AS_SLOT2=1 makes its tier the third slot's main tier AND the second stream's tier of such a batch instead: resolveTiers)
	{ { TIER_NONE, TIER_NONE, 20 }, 2, ROLE_ALONE, -1, GATE_TABFIT|GATE_ALONE, WORK_W128, "DACC_W128_TIER", "DACC_W128_AS_SLOT2", 0, true, false, W128_GMEM_SLAB, W128 } };
static TierId const TIER_MAIN[TIER_NSLOTS] = { ID_SLOT0, ID_SLOT1, ID_SLOT2 };
// does the stage run in a batch of this shape, and the tier whose capacities the plan holds for it (a stage that does not run keeps
// those of the nearest shape: the first slot of a wide batch has tier 1's or tier 4's)
static inline bool stageRuns(TierStage const & st, bool const deep, bool const wide) { return st.tier[wide ? 2 : deep] != TIER_NONE; }
// DACC_*_AS_SLOT2=1 of a trailing stage's row: the third slot's main tier is that stage's tier (read by the planner and by resolveTiers alike, so once per call)
static inline bool stageAsSlot2(TierStage const & st) { return st.slot2switch && envOn(st.slot2switch); }
// (w: the batch's window size, for the rows that are for one size alone (TierStage::onlyw); a caller that leaves it out sees none of them.  Such a row's AS_SLOT2 switch
// names the second stream's tier as well: the long string stage of that batch is its tier)
static inline uint32_t stageTier(TierStage const & st, bool const deep, bool const wide, uint32_t const w = 0)
{
	TierStage const * t = &st;
	if ( &st == &TIER_CHAIN[ID_SLOT2] || &st == &TIER_CHAIN[ID_LONG] )
		for ( TierStage const & r : TIER_CHAIN )
			if ( (r.onlyw ? (r.onlyw == w) : (&st == &TIER_CHAIN[ID_SLOT2])) && stageAsSlot2(r) && (wide ? r.slot2wide : r.slot2narrow) ) { t = &r; break; }
	// (a row with a wide tier only -- ID_WDEEP -- keeps that tier's capacities in the other shapes, where it does not run)
	return (wide && t->tier[2] != TIER_NONE) ? t->tier[2] : (t->tier[deep] != TIER_NONE ? t->tier[deep] : (t->tier[0] != TIER_NONE ? t->tier[0] : t->tier[2]));
}

// the environment switches of the chain, read once per context
struct TierSwitches
{
	bool nofast;              // DACC_NOFAST=1: generic engine only
	uint32_t tiers;           // DACC_TIERS: bit t enables the main tier of slot t (bit 2: tier 5 as well), bit 3 tier 0 (size classes), bit 4 tier 7 (the middle class)
	bool widetier;            // DACC_WIDE_TIER=0: wide batches run in the generic engine only, as in rounds 4-5
	bool dense;               // DACC_DENSE_TIER=0: the second slot hands on to tier 3 directly (before round 6's dense tiers)
	bool deepwin;             // DACC_DEEP_TIER=0: no deep-window tier (tier 12) in front of tier 3
	bool off[TIER_NROWS];        // a trailing stage's DACC_*_TIER=0: the chain as it was before that stage (its windows run in what stands behind it)
	bool as_slot2[TIER_NROWS];   // a trailing stage's DACC_*_AS_SLOT2=1: its tier as the third slot's main tier, no such stage
	bool longstr;             // DACC_LONGSTR_TIER=0: no long string stage (tier 17) on the second stream of a wide batch, the generic engine alone as before that stage
	bool conflict() const { int n = 0; for ( bool const b : as_slot2 ) n += b; return n > 1; }      // more than one wants the third slot: dacc_create refuses
	bool long128;             // DACC_LONG128=0: windows with a string of 65 ... 128 bases run in tier 5 on the second stream (rounds 3-5)
	bool hand;                // DACC_HAND=0: no hand-over buffer, every hand-over restarts from the strings
	uint32_t t0inst, t7inst;  // DACC_T0INST / DACC_T7INST: size-class thresholds (k-mer instances) of tiers 0 and 7
	uint32_t lds_t1, lds_t0;  // DACC_LDS_T1 / DACC_LDS_T0, measurement only: LDS bytes requested for the first slot's main tier / for tier 0 (more than it needs = fewer wavefronts per CU)
};
static inline TierSwitches readTierSwitches()
{
	TierSwitches S;
	S.nofast = envOn("DACC_NOFAST");
	S.tiers = envNum("DACC_TIERS",31);
	S.widetier = !envOff("DACC_WIDE_TIER"); S.dense = !envOff("DACC_DENSE_TIER"); S.deepwin = !envOff("DACC_DEEP_TIER"); S.longstr = !envOff("DACC_LONGSTR_TIER"); S.long128 = !envOff("DACC_LONG128"); S.hand = !envOff("DACC_HAND");
	for ( uint32_t i = 0; i < TIER_NROWS; ++i ) { TierStage const & st = TIER_CHAIN[i]; S.off[i] = st.offswitch && envOff(st.offswitch); S.as_slot2[i] = stageAsSlot2(st); }
	S.t0inst = envNum("DACC_T0INST",T0INST_DEFAULT); S.t7inst = envNum("DACC_T7INST",T7INST_DEFAULT);
	S.lds_t1 = envNum("DACC_LDS_T1",0); S.lds_t0 = envNum("DACC_LDS_T0",0);
	return S;
}

enum : uint32_t { TIER_LDS_CU = 160*1024 };
// launch geometry of a tier: floor(160 KiB / ldsbytes) wavefronts per CU, 1 ... 8, and a workgroup per window up to 256 CUs' worth
// (a device-memory tier is launched with tierGridGmem below)
static inline uint32_t tierGrid(uint32_t const ldsbytes, uint64_t const nwindows)
{
	uint64_t const percu = std::min<uint64_t>(8,std::max<uint64_t>(1,TIER_LDS_CU / (ldsbytes ? ldsbytes : 1)));
	return static_cast<uint32_t>(std::min<uint64_t>(256*percu,std::max<uint64_t>(8,((nwindows+7)/8)*8)));
}

// Launch geometry of a device-memory tier (FastCaps::gmem): no LDS and 512 registers, so up to four workgroups per CU would fit; what bounds the
// grid is the slab, gbytes per workgroup (tier 13: 1 059 840 B, tier 14: 1 125 632 B, tiers 15, 16, 18 and 19: see DESIGN 3.2), kept to TIER_GMEM_SLAB = 256 MiB per context:
// 256 MiB / 1 059 840 B = 253 -> 248 workgroups (a multiple of 8, one share per XCD), 232 for tier 14 -- about one per CU, whose working sets
// (1 MB each) then share the L2 of their XCD with no more than 31 others.  The stage sees a few windows per batch, hundreds on high-error data;
// a small batch gets a workgroup per window and a slab to match.
// (a row of TIER_CHAIN may name a budget of its own, TierStage::slab: the wide deep stage's 2 GiB, see WDEEP_GMEM_SLAB)
static inline uint32_t tierGridGmem(uint32_t const gbytes, uint64_t const nwindows, uint64_t const slab = TIER_GMEM_SLAB)
{
	uint64_t g = std::min<uint64_t>(1024,std::max<uint64_t>(8,((nwindows+7)/8)*8));
	uint64_t const fit = ((slab ? slab : static_cast<uint64_t>(TIER_GMEM_SLAB)) / (gbytes ? gbytes : 1)) & ~7ull;
	return static_cast<uint32_t>(std::max<uint64_t>(8,std::min<uint64_t>(g,fit)));
}

// The chain of one batch with every gate resolved, by TierId.
struct TierPipeline
{
	bool usefast = false;                 // the LDS tiers may run at all
	bool widetier = false;                // wide windows (w = 64 ... 127) in tiers 8 and 9
	bool ok[TIER_NROWS] = {};
	uint32_t tier[TIER_NROWS] = {};     // the tier of the stage in this batch
	bool late_long = false;               // slots 1 and 2 skip only the windows the second stream has (a string of more than 128 bases), not all with more than 64
	bool slot1_long = false;              // the pre-scan puts the windows with a string of 65 ... 128 bases on the first slot's hand-over list
	bool handover = false;                // hand-over slots pay: a wide batch has nothing to hand the sorted instances to
	uint32_t handwords = 0;               // 64 bit words of a hand-over slot: header + the instance capacity of the tiers that hand on + their last k-mer lists
	bool slotok(uint32_t const s) const { return ok[TIER_MAIN[s]]; }
	bool anytier() const { return slotok(0) || slotok(1) || slotok(2); }
};

// fastpath: the caller's own conditions (not switched off, a model table that fits 32 bit fixed point).  capsOf(id): the plan's capacities
// of a stage (BatchPlan::stageCaps); the measurement switches DACC_LDS_T1 / DACC_LDS_T0 raise the LDS sizes in them.
// maxstrings: strings of the deepest window of the batch (BatchPlan::maxstrings); a trailing stage with a threshold (TierStage::minstrings) is resolved only for a batch that has a
// window for it -- a caller that walks the slots only (the emulation harness) leaves it out and sees no such stage.
// rows: the rows of TIER_CHAIN the caller holds capacities for (capsOf is asked for no other): TIER_NSTAGES, or TIER_NROWS with the stages behind ID_LONG.
template<typename C>
static inline TierPipeline resolveTiers(TierSwitches const & S, bool const fastpath, bool const deep, bool const wide, uint32_t const nrows, uint32_t const nsup, uint32_t const w, C && capsOf,
	uint32_t const maxstrings = 0, uint32_t const rows = TIER_NSTAGES)
{
	TierPipeline R;
	// wide windows, w = 64 ... 127 (model table of up to 128 rows: two words per position mask): DACC_WIDE_TIER=0 leaves them to the generic engine.
	// w = 128 (BatchPlan::wide covers it; 129 rows, 0 ... w: three words per position mask, up to 192 rows) is a batch of its own: none of the wide tiers holds its
	// table, so no slot, no trailing stage and no second stream run -- its stage (ID_W128, tier 20) alone, or, with DACC_W128_AS_SLOT2=1, that tier as the third slot's
	// main tier and the second stream's tier
	bool const w128 = wide && w == W128;
	bool const w128slot = w128 && S.as_slot2[ID_W128];
	R.widetier = wide && S.widetier && nrows <= (w128 ? 192u : 128u) && nsup <= FSUPCAPW;
	R.usefast = fastpath && (R.widetier || (nrows <= 64 && nsup <= FSUPCAP && w <= 63));
	R.handover = S.hand && !R.widetier;
	R.handwords = (deep ? 2048u + 128u : 1024u + 64u) + 4u;
	auto const gated = [&](uint32_t const i) -> bool
	{
		TierStage const & st = TIER_CHAIN[i]; FastCaps const & F = capsOf(i);
		return R.usefast && stageRuns(st,deep,wide) && (st.onlyw ? st.onlyw == w : (!w128 || (w128slot && (i == ID_SLOT2 || i == ID_LONG)))) && (F.gmem || F.ldsbytes <= TIER_LDS_CU) && (st.tiersbit < 0 || ((S.tiers >> st.tiersbit) & 1))
			&& (!(st.flags & GATE_TABFIT) || static_cast<uint64_t>(nrows+1)*(nsup+1) <= F.tabcap)
			&& (!(st.flags & GATE_T7_ABOVE_T0) || S.t7inst > S.t0inst) && (!(st.flags & GATE_DENSE) || S.dense) && (!(st.flags & GATE_DEEP) || S.deepwin)
			&& (!(st.flags & GATE_TRAILING) || (!S.off[i] && !S.as_slot2[i] && (!st.minstrings || maxstrings > st.minstrings)))
			&& (!(st.flags & GATE_ALONE) || (!S.off[i] && !S.as_slot2[i]))
			&& (!(st.flags & GATE_LONGSTR) || !wide || S.longstr);
	};
	{ FastCaps & F = capsOf(ID_SLOT0); if ( S.lds_t1 > F.ldsbytes && S.lds_t1 <= TIER_LDS_CU ) F.ldsbytes = S.lds_t1; }
	{ FastCaps & F = capsOf(ID_T0); if ( S.lds_t0 > F.ldsbytes && S.lds_t0 <= TIER_LDS_CU ) F.ldsbytes = S.lds_t0; }
	for ( uint32_t i = 0; i < rows; ++i ) { R.tier[i] = stageTier(TIER_CHAIN[i],deep,wide,w); if ( TIER_CHAIN[i].role != ROLE_FRONT ) R.ok[i] = gated(i); }
	// a trailing stage reads what a slot handed on: no slot, no such stage (generic-only configurations stay generic-only)
	for ( uint32_t i = 0; i < rows; ++i ) if ( TIER_CHAIN[i].role == ROLE_LAST ) R.ok[i] = R.ok[i] && R.anytier();
	// the front tiers, in chain order (a front tier stands before the main tier of its slot)
	for ( uint32_t i = 0; i < rows; ++i )
	{
		TierStage const & st = TIER_CHAIN[i];
		if ( st.role == ROLE_FRONT )
			R.ok[i] = gated(i) && R.slotok(st.slot) && (!(st.flags & GATE_PREV_FRONT) || R.ok[i-1]) && (!(st.flags & GATE_PREV_SLOT) || R.slotok(st.slot-1));
	}
	R.late_long = R.slotok(0) && S.long128;
	R.slot1_long = R.late_long && (R.slotok(1) || R.slotok(2));
	return R;
}

}
#endif
