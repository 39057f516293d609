/*
 * The launch arithmetic of a batch's setup (capi.hip: dacc_submit_piles_body), host only and plain C++17: how many words, lanes, LDS bytes and workgroups
 * the trace kernels get, the generic engine's grids, the capacity of the hand-over buffer, how much of dacc_timing a caller's record size takes.  No device
 * and no environment: what a switch overrides comes in as an argument.  tests/tiers/launch_geometry.cpp pins every threshold; the CPU emulation of the
 * tests chooses its trace kernel here as well.
 */
#ifndef DACC_LAUNCH_GEOMETRY_HPP
#define DACC_LAUNCH_GEOMETRY_HPP
#include <cstdint>
#include <cstddef>
#include "../../include/daccord_hip.h"

// (the sizing helpers are read by the trace kernels too)
#if defined(__HIP__)
#define DACC_GEOM_HDEV __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define DACC_GEOM_HDEV inline
#endif

namespace dacc {

// ---- column stores of the trace kernels (trace_kernel.hpp: what the constants trade against each other)
enum { TRS = 16 };      // wide kernels (k_trace_wide): checkpoints and segment in LDS
// two word kernel: T2C columns between checkpoints (global slab), T2S columns per segment (LDS)
#if !defined(DACC_T2C)
#define DACC_T2C 8
#endif
#if !defined(DACC_T2S)
#define DACC_T2S 4
#endif
enum { T2C = DACC_T2C, T2S = DACC_T2S };
static_assert(T2C % T2S == 0 && T2C <= 16,"segments tile the checkpoint groups; a group's B symbols are kept packed in 32 bits");
DACC_GEOM_HDEV uint32_t traceSlots(uint32_t const maxcols) { return maxcols/TRS + 1 + TRS; }     // wide kernels: checkpoints 0,TRS,2*TRS,.. + one segment
DACC_GEOM_HDEV uint32_t traceCheckpoints(uint32_t const maxcols) { return maxcols/T2C + 1; }     // two word kernel: checkpoints per lane (global slab)
DACC_GEOM_HDEV uint32_t traceSlabWords(uint32_t const maxcols) { return traceCheckpoints(maxcols)*4u*64u; }      // 64 bit words per workgroup
enum : uint32_t { TRACE2_LDS = T2S*64*32 };      // LDS bytes of a wavefront of k_trace
template<int NW> DACC_GEOM_HDEV uint32_t traceWideBytesPerLane(uint32_t const maxcols) { return traceSlots(maxcols)*(16u*NW+2u); }

// ---- trace kernels: one wavefront per workgroup, as many workgroups per CU as their LDS column stores allow, a few rounds of blocks per workgroup
struct TraceGeometry
{
	uint32_t words = 0;      // 64 bit words per column vector: 2 (k_trace), 4 or 8 (k_trace_wide<words>)
	uint32_t lanes = 0;      // lanes of a wavefront that take blocks
	uint32_t lds = 0;        // dynamic LDS bytes of a workgroup
	bool fits = false;       // lds <= 160 KiB; else the batch is DACC_ENOTSUP and what follows is not set
	uint64_t percu = 0;      // resident workgroups per CU
	uint32_t grid = 0;
};
// two word columns for tspace <= 128 while every lane's column store fits (blocks of up to 928 B bases: always with one byte trace values); a batch with a
// longer block runs the four word kernel, which sizes its lanes to the LDS
static inline uint32_t traceWords(int32_t const tspace, uint32_t const maxcols) { return (tspace <= 128 && maxcols <= 928) ? 2 : (tspace <= 256 ? 4 : 8); }
// k_trace draws its rounds of 64 blocks from a 32 bit counter (DACC_TRACE_DYN): only while no workgroup's last draw can wrap it
static inline bool traceCounterHolds(uint64_t const nblocks) { return nblocks < 0xFFFFFF00ull; }
// percu_override: DACC_TR_PERCU (1 ... 32; anything else, 0 included: none)
static inline TraceGeometry traceGeometry(int32_t const tspace, uint32_t const maxcols, uint64_t const nblocks, uint64_t const percu_override)
{
	TraceGeometry G;
	G.words = traceWords(tspace,maxcols);
	G.lanes = 64;
	if ( G.words == 2 ) G.lds = TRACE2_LDS;
	else
	{
		// wide blocks: as many lanes per wavefront as have room for their column checkpoints
		uint32_t const perlane = G.words == 4 ? traceWideBytesPerLane<4>(maxcols) : traceWideBytesPerLane<8>(maxcols);
		while ( G.lanes > 8 && static_cast<uint64_t>(G.lanes)*perlane > 160*1024 ) G.lanes >>= 1;
		G.lds = G.lanes*perlane;
	}
	G.fits = !(G.lds > 160*1024);
	if ( !G.fits ) return G;
	// resident workgroups per CU: LDS is handed out in granules of 1280 bytes (measured, round 5); k_trace holds 92 registers = 5 wavefronts per SIMD
	uint64_t percu = (160*1024) / ((((G.lds ? G.lds : 1) + 1279u)/1280u)*1280u); if ( percu > (G.words == 2 ? 20u : 8u) ) percu = (G.words == 2 ? 20u : 8u); if ( percu < 1 ) percu = 1;
	if ( percu_override >= 1 && percu_override <= 32 ) percu = percu_override;
	// two word kernel: exactly the resident workgroups (grid stride over the blocks), so that the checkpoint slabs
	// (53 KB per workgroup at a B span of 160) stay in the L2 / Infinity Cache
	uint64_t g = (nblocks+G.lanes-1)/G.lanes, gmax = 256*percu*(G.words == 2 ? 1 : 4);
	if ( g > gmax ) g = gmax;
	if ( g < 1 ) g = 1;
	if ( G.words == 2 )
	{
		// the checkpoint slabs of the resident workgroups are meant to stay in the Infinity Cache (256 MB): one block with a
		// long B span makes every workgroup's slab large (300 KB at the 928 columns this kernel takes), so the grid gives way
		// before the slabs outgrow 192 MB, down to one workgroup per CU
		uint64_t const slabbytes = static_cast<uint64_t>(traceSlabWords(maxcols))*sizeof(uint64_t);
		while ( g > 256 && g*slabbytes > (192ull<<20) ) g -= 256;
	}
	G.percu = percu; G.grid = static_cast<uint32_t>(g);
	return G;
}

// ---- the generic engine (k_window)
// Its per-wavefront arena grows with the deepest pile of the batch (7 MB at depth 32, 200 MB at 1000, 800 MB at the default -D of 5000): the number of
// wavefronts is bounded so that one batch's arenas stay below 32 GB instead of failing the batch for want of 400 GB.
static inline uint32_t boundByArena(uint64_t grid, uint64_t const bytes, uint64_t const mingrid)
{
	uint64_t const budget = 32ull << 30;
	while ( grid > mingrid && grid*bytes > budget ) grid >>= 1;
	return static_cast<uint32_t>(grid < 1 ? 1 : grid);
}
struct GenericGeometry { uint32_t retry_grid, win_grid, early_grid; };      // behind the chain; over all windows; on the second stream (0: none runs there)
// chain: slots and a second stream run in front of it (else: the generic engine alone, or with the stage of w = 128 in front)
static inline GenericGeometry genericGeometry(uint64_t const nwindows, uint64_t const arenabytes, bool const chain)
{
	uint64_t wg = ((nwindows+7)/8)*8;
	uint64_t const maxwg = 256*8;
	if ( wg > maxwg ) wg = maxwg;
	if ( wg < 8 ) wg = 8;
	GenericGeometry G;
	if ( !chain ) { G.win_grid = boundByArena(wg,arenabytes,8); G.retry_grid = G.win_grid; G.early_grid = 0; return G; }
	G.retry_grid = boundByArena(wg < 512 ? wg : 512,arenabytes,8);
	G.win_grid = G.retry_grid;
	// generic engine on the second stream (windows with a string of more than 64 bases): a wavefront per window as far as the arenas stay below 8 GB (the
	// handful of such windows of config 2 took the generic engine up to 6.6 s each next to the 8.2 s of the LDS tiers; tier 5 takes them now)
	G.early_grid = G.retry_grid < 256 ? G.retry_grid : 256;
	while ( G.early_grid > 16 && static_cast<uint64_t>(G.early_grid)*arenabytes > (8ull<<30) ) G.early_grid >>= 1;
	return G;
}

// ---- hand-over slots (sorted instances of a window that overflowed a tier's node table, picked up by the next tier): as many as a third of the windows,
// within 16 GB (config 2: 1.6 M hand-overs of 10 M windows); handwords: 64 bit words of a slot (TierPipeline::handwords)
static inline uint64_t handOverCapacity(uint64_t const nwindows, uint32_t const handwords, bool const krange, bool const nohand, bool const handover)
{
	uint64_t cap = nwindows/3 + 4096; uint64_t const maxcap = (16ull<<30) / (static_cast<uint64_t>(handwords)*8ull);
	if ( cap > maxcap ) cap = maxcap;
	if ( krange ) cap = 0;        // klow != khigh
	if ( nohand ) cap = 0;        // a retry after an allocation failure: no optional buffer (dacc_drop_hand)
	if ( !handover ) cap = 0;     // DACC_HAND=0, or a wide batch: nothing to hand the sorted instances to
	return cap;
}

// ---- dacc_last_timing2(size): the record grew by 16 bytes per stage, and a caller gets the largest record it has room for in full -- one built with an
// earlier record that passes a larger size (its record inside a larger buffer) gets the bytes it knows.  A size below the first of them copies `size` bytes
static size_t const TIMING_SIZES[] = { DACC_TIMING_SIZE_V2, DACC_TIMING_SIZE_V3, DACC_TIMING_SIZE_V4, DACC_TIMING_SIZE_V5, sizeof(dacc_timing) };
static inline size_t timingCopySize(size_t const size)
{
	size_t n = size < TIMING_SIZES[0] ? size : TIMING_SIZES[0];
	for ( size_t const s : TIMING_SIZES ) if ( s <= size ) n = s;
	return n;
}

}
#endif
