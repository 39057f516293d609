/*
 * The capacity tiers of the window fast path (fast_window.hpp), as compile-time data: one row FastTier<N> per tier of DACC_EVERY_TIER
 * (tier_pipeline.hpp).  Plain C++17, no device code: the planner, the launches, the emulation and the engine all read the rows from here.
 * The engine is instantiated once per row; the layout FastLds<CT> (fast_layout.hpp) is a compile time constant, so every LDS access has
 * an immediate offset.  Which of the tiers a batch runs, in which order and behind which switches, is written down once, in tier_pipeline.hpp.
 *
 *   tier  role                                                        layout  path/stretch ids  wavefronts per CU
 *      0  front of slot 0, shallow: the small size class              gw       8 /  8 bit       8
 *      7  front of slot 0, shallow: the middle size class             gw       8 /  8 bit       7
 *      1  slot 0 of shallow batches                                   gw       8 /  8 bit       6
 *      4  slot 0 of deep batches (many strings, small graph)          gw       8 /  8 bit       5
 *      6  slot 1 of shallow batches (strings of up to 128 bases)      gw       8 /  8 bit       4
 *      2  slot 1 of deep batches                                      gw       8 /  8 bit       3
 *     10  front of slot 2, shallow: dense graphs                      gw      16 /  8 bit       2
 *     11  front of slot 2, deep: many instances                       gw      16 /  8 bit       2
 *     12  front of slot 2, shallow and deep: 97 ... 250 strings       gw      16 / 16 bit       1
 *      3  slot 2 of shallow and deep batches                          gw      16 / 16 bit       1
 *      8  slot 1 of wide batches (w = 64 ... 127)                     gw      16 /  8 bit       2
 *      9  slot 2 of wide batches                                      gw      16 / 16 bit       1
 *      5  second stream (k_window_long): strings of up to 128 bases   legacy  16 /  8 bit       1
 *     13  last stage, shallow and deep (layout in device memory)      gw      16 / 16 bit       no LDS
 *     14  last stage, wide batches (layout in device memory)          gw      16 / 16 bit       no LDS
 *     15  very deep stage, shallow and deep: 251 ... 1000 strings     gw      16 / 16 bit       no LDS
 *     16  deepest stage, shallow and deep: 1001 ... 2000 strings      gw      16 / 16 bit       no LDS
 *     17  second stream, wide batches: strings of 129 ... 255 bases   gw      16 / 16 bit       no LDS
 *     18  full-depth stage, shallow and deep: 2001 ... 5001 strings   gw      16 / 16 bit       no LDS
 *     19  wide deep stage, wide batches: 251 ... 1000 strings         gw      16 / 16 bit       no LDS
 *     20  w = 128: every window of such a batch, strings up to 255     gw      16 / 16 bit       no LDS
 *
 * A window that does not fit its tier leaves it through processWindowFast (fast_window.hpp), which returns
 * FW_NEXT when a window overflows a tier (flags say what overflowed: 1 instances, 2 nodes, 8 candidates, 16 walk,
 * 32 stretches, 64 links, 128 weights, 512 pools (0x4000 reverse cache, 0x8000 path ids, 0x10000 forward pool,
 * 0x20000 popped paths, 0x40000 score intervals), 1024 introsort's depth limit reached in the replayed std::sort (the tiers
 * stop there; the generic engine finishes such a range with libstdc++'s heapsort fallback), 2048 base length, 4096 candidate
 * length / sequence, 8192 gap filling) and FW_GENERIC for shapes the tier does not support (a window wider than it holds, a string
 * longer than its string stride lstr: 64 or 128 bases, tiers 17 and 20: longer than 255); those go to tier 5 / tier 17 / the generic engine (dbg_window.hpp).
 */
#ifndef DACC_FAST_TIERS_HPP
#define DACC_FAST_TIERS_HPP
#include <cstdint>
#include "tier_pipeline.hpp"

namespace dacc {

// compile time capacities of the tiers: every LDS offset below is an instruction immediate
template<int TIER> struct FastTier;
// gw: the weights of the feasible (stretch, position) pairs and the model table live in global memory (a scratch slab per
// workgroup / the padded 32 bit table), the build-phase arrays are overlaid by the enumeration pools (spilled to the slab
// while the enumerations run): layout FastLds<CT,true>.  Round 3 measured that a second wavefront per SIMD hides the LDS
// round trips of the first almost completely (profiles/r03a_occupancy_experiment.md), so LDS bytes per window decide the
// throughput: tier 1 is 26.3 KB = 6 wavefronts per CU with (almost) the capacities it had at 53.8 KB = 3 per CU.
// (round 6) reverse pool of tiers 0 and 1 in chunks of TWO paths: a lane takes pool entries a chunk at a time, and with one lane per last
// k-mer candidate (9 on average, up to 24) most chunks of four were half empty -- the reverse pool had become what sent tier 0's windows on
// (82 % of its hand-overs, each after the whole build phase and the feasibility; emulation, 8 piles of config 2: 261 of 5251 windows -> 14)
#if !defined(DACC_RCH01)
#define DACC_RCH01 2
#endif
template<> struct FastTier<1> { typedef uint8_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 1024, rch = DACC_RCH01, fch = 4, fnw = 2, fnc = 40, idmax = 250, rpstcap = 256, lstr = 64, maxs = 32, precap = 1024, ncap = 776, scap = 112, lcap = 960, wcap = 1024, rccap = 144, fcap = 192, siqcap = 56, blcap = 96, seqcap = 32, psiq = 8, consrow = 64, lscrids = 2048, wide = 0, mins = 0, gmem = 0 }; };
// tier 0 (size classes): the windows a pre-pass (classifyWindow, k_classify) finds small -- few strings, at most T0INST k-mer
// instances -- in 20 KB = 8 wavefronts per CU (two on every SIMD).  What overflows it joins the other windows in tier 1.
template<> struct FastTier<0> { typedef uint8_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 768, rch = DACC_RCH01, fch = 4, fnw = 2, fnc = 32, idmax = 250, rpstcap = 256, lstr = 64, maxs = 28, precap = 576, ncap = 524, scap = 88, lcap = 640, wcap = 768, rccap = 96, fcap = 128, siqcap = 56, blcap = 96, seqcap = 32, psiq = 8, consrow = 64, lscrids = 2048, wide = 0, mins = 0, gmem = 0 }; };
// tier 7 (round 6, the MIDDLE size class of shallow batches): 22.9 KB = 7 wavefronts per CU.  Four fifths of the windows tier 1 (6 per CU)
// used to run have at most 28 strings, 704 k-mer instances, 640 nodes and 800 links (emulation, 16 piles of config 2: 4244 of 5295); the
// pre-pass sends them here, what overflows joins tier 1's list like tier 0's hand-overs join this one.
template<> struct FastTier<7> { typedef uint8_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 896, rch = DACC_RCH01, fch = 4, fnw = 2, fnc = 32, idmax = 250, rpstcap = 256, lstr = 64, maxs = 28, precap = 704, ncap = 640, scap = 104, lcap = 800, wcap = 896, rccap = 112, fcap = 148, siqcap = 56, blcap = 96, seqcap = 32, psiq = 8, consrow = 64, lscrids = 2048, wide = 0, mins = 0, gmem = 0 }; };
// (the size-class thresholds of the pre-pass, T0INST_DEFAULT / T7INST_DEFAULT = the instance capacities of tiers 0 and 7: tier_pipeline.hpp)
// tier 2: gw layout as well since round 3 (43 KB: 3 wavefronts per CU; the legacy layout was 80.5 KB: 2 per CU)
// (round 4: 76 KB = 2 wavefronts per CU instead of 46.5 KB = 3, with tier 3's node capacity: at 54x more than half of what the deep tier
// hands on has more than 1024 nodes at filter frequency 1 and used to go through this tier only to be handed on again to tier 3, which
// runs one wavefront per CU)
// (round 6: 53 744 B = 42 LDS granules = THREE wavefronts per CU instead of 63.9 KB = two, with 1536 nodes and 2032 links instead of 2048 / 2304:
// of the 65 903 windows the deep tier hands on in 1000 piles of the 54x shape 3045 went on to tier 3 before and 3329 do now, and the tier's
// time falls from 96 to 66 ms -- 27.4 -> 30.1 Mbase/s, profiles/r06s; the node tables are 20 of its bytes per node)
#if !defined(DACC_T2_NCAP)
#define DACC_T2_NCAP 1536
#endif
#if !defined(DACC_T2_LCAP)
#define DACC_T2_LCAP 2032
#endif
template<> struct FastTier<2> { typedef uint8_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 3072, rch = 4, fch = 4, fnw = 4, fnc = 64, idmax = 250, rpstcap = 256, lstr = 64, maxs = 96, precap = 2048, ncap = DACC_T2_NCAP, scap = 232, lcap = DACC_T2_LCAP, wcap = 3072, rccap = 256, fcap = 192, siqcap = 96, blcap = 96, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 0, gmem = 0 }; };
// tier 6 (second slot of SHALLOW batches since round 3, gw layout, 36 KB = 4 wavefronts per CU): what tier 1 hands on at 20x
// are windows with more than its 608 nodes (82 % of the hand-overs) or fuller pools, not more strings or instances, so this
// tier keeps tier 1's string / instance capacities and spends its LDS on nodes, stretches and pools.  Deep batches keep
// tier 2 (64 strings, 2048 instances) behind the deep tier.
// (round 6: the tier sat at 34 720 B, 6 KB below what four wavefronts per CU allow (40 960 B): the bytes went to what sends its windows on to
// tier 3 -- ONE wavefront per CU -- on the ONT mix at small k (emulation, 6 piles of config 5 at k = 10 / 12: reverse pool 73 / 130, weights 53 / 1,
// forward pool 45 / 7 of about 200 hand-overs): reverse pool 192 -> 256 paths in chunks of two, 248 stretches, 2048 weight records)
template<> struct FastTier<6> { typedef uint8_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 2048, rch = 2, fch = 8, fnw = 3, fnc = 40, idmax = 250, rpstcap = 256, lstr = 128, maxs = 40, precap = 1024, ncap = 1024, scap = 248, lcap = 1280, wcap = 2048, rccap = 256, fcap = 256, siqcap = 96, blcap = 96, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 0, gmem = 0 }; };

// tier 3 (one wavefront per CU): 16 bit path ids, so that an enumeration may hold more than 250 paths; sized for deep piles
// too (BASELINE config 4, 54x: up to 96 strings with 4096 k-mer instances, 72 first / last k-mer candidates)
// gw layout and 16 bit STRETCH ids since round 3: what the legacy tier 3 handed to the generic engine at 54x were windows with
// more than 250 stretches (13 of 19 per 60 000 windows) or more than 2112 feasible weights (5 of 19), and each of them cost the
// generic engine seconds (685 such windows were 92 % of a 2000-pile 54x batch, profiles/r03c_bench_54x_2000piles.log)
template<> struct FastTier<3> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 1000, gw = 1, wcapg = 8192, rch = 8, fch = 16, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 96, precap = 4096, ncap = 2048, scap = 1024, lcap = 4096, wcap = 8192, rccap = 2048, fcap = 512, siqcap = 256, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 0, gmem = 0 }; };

// tier 4 (three wavefronts per CU, takes the place of tier 1 in batches of deep piles): many strings and k-mer instances,
// small graph.  At 54x (BASELINE config 4) 96 % of the windows find their consensus at filter frequency 2, where the graph
// has about a hundred nodes, while the 55 strings of a window carry 1500 k-mer instances.
template<> struct FastTier<4> { typedef uint8_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 608, rch = 4, fch = 4, fnw = 2, fnc = 40, idmax = 250, rpstcap = 256, lstr = 64, maxs = 96, precap = 2048, ncap = 256, scap = 48, lcap = 256, wcap = 608, rccap = 128, fcap = 96, siqcap = 56, blcap = 96, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 0, gmem = 0 }; };

// tier 5 (one wavefront per CU, only for the windows the pre-scan found): B strings of up to 128 bases (string stride 128,
// two words per pattern mask); everything else as tier 3 with 64 strings.  Window strings of more than 64 bases are rare
// at the default window (a few per ten million windows of config 2) but each of them costs the generic engine seconds.
template<> struct FastTier<5> { typedef uint16_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 0, wcapg = 0, rch = 8, fch = 16, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 64, precap = 4096, ncap = 1792, scap = 250, lcap = 2048, wcap = 2040, rccap = 512, fcap = 512, siqcap = 256, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 0, gmem = 0 }; };

// tier 8 (round 6, two wavefronts per CU): WIDE windows, -w 64 ... 127 (the reference takes any -w, daccord.cpp:1282-1305; rounds 4-5 ran them in the generic
// engine, two orders of magnitude slower per window).  What a wide window needs beyond tier 6's two-word pattern masks: feasible start positions
// of a stretch up to nrows = w+1 <= 128 (two words per position mask: maskF / maskFh), candidates and a consensus of up to 128 symbols, the
// two-word consensus -> A alignment and the wide window record (dev_types.hpp: WRECW).  A batch with w > 63 runs this tier alone in front of the
// generic engine (BatchPlan::wide); sized for 20x piles at w = 64 ... 96 (20 strings of 83 k-mers at w = 96, k = 14).
template<> struct FastTier<8> { typedef uint16_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 6144, rch = 4, fch = 8, fnw = 4, fnc = 64, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 40, precap = 3072, ncap = 2304, scap = 248, lcap = 3072, wcap = 6144, rccap = 640, fcap = 512, siqcap = 96, blcap = 128, seqcap = 96, psiq = 10, consrow = 128, lscrids = 2560, wide = 1, mins = 0, gmem = 0 }; };

// tier 9 (round 6, one wavefront per CU): what overflows tier 8 -- its reverse pool (512 paths), forward pool, score intervals -- before the generic
// engine, which recomputes both enumerations for every (first, last) k-mer pair and takes seconds for such a window (30 of 37 000 windows at
// w = 64 were 6.2 of a step's 6.7 s, profiles/r06v).  Tier 3's pools with the wide tier's masks, alignment and record.
template<> struct FastTier<9> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 500, gw = 1, wcapg = 8192, rch = 16, fch = 16, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 64, precap = 4096, ncap = 3072, scap = 512, lcap = 4096, wcap = 8192, rccap = 2048, fcap = 1024, siqcap = 256, blcap = 128, seqcap = 96, psiq = 10, consrow = 128, lscrids = 2560, wide = 1, mins = 0, gmem = 0 }; };

// tier 10 (round 6, two wavefronts per CU): the DENSE-graph tier of shallow batches, between tier 6 (four per CU, 8 bit path ids: 256 reverse
// paths) and tier 3 (ONE per CU).  On the ONT error mix at k = 10 tier 6 hands 1.4 % of the windows on -- reverse pools of more than 256 paths,
// forward pools, more than 1024 k-mer instances -- and tier 3 needs 17 % of the step for them (profiles/r06k/bench_ont_k10.log; VERDICT r05 task 4:
// "more than 1 % in tier 3: add a dense-graph tier").  Tier 8's pools and 16 bit ids without its wide parts.
template<> struct FastTier<10> { typedef uint16_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 6144, rch = 4, fch = 8, fnw = 4, fnc = 64, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 64, precap = 2560, ncap = 2048, scap = 248, lcap = 3072, wcap = 6144, rccap = 896, fcap = 512, siqcap = 128, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 0, gmem = 0 }; };

// tier 11 (round 6, two wavefronts per CU): tier 10's place in batches of DEEP piles, between tier 2 (three per CU, 2048 k-mer instances) and tier 3 (one per CU).
// At 54x what tier 2 hands on are windows of more than 2048 k-mer instances (75 strings and more: 186 of 208 hand-overs in 12 piles of config 4), a few node
// tables and pools; tier 3 needs 6.8 % of the step for them (profiles/r06zz/bench_54x_2000piles.log).  Tier 3's string / instance capacities with tier 10's pools.
template<> struct FastTier<11> { typedef uint16_t id_t; typedef uint8_t sid_t; enum : uint32_t { smax = 250, gw = 1, wcapg = 4096, rch = 4, fch = 8, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 96, precap = 4096, ncap = 1536, scap = 248, lcap = 2048, wcap = 4096, rccap = 640, fcap = 384, siqcap = 128, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 0, gmem = 0 }; };

// tier 12 (one wavefront per CU): the DEEP-WINDOW tier, windows of 97 ... 250 strings (repeat piles: the rRNA operons of a bacterial genome at 20x
// are about 140 deep, a low-copy repeat at 54x 100 ... 220), which every other tier refuses at its string count and which used to run in the
// generic engine at a few dozen wavefronts (its scratch arenas grow with the deepest pile of the batch).  Tier 3's graph and pools with 250 strings
// and 8192 k-mer instances, 157 856 B of LDS.  Such a window finds its consensus at filter frequency 2, but its graph is not small: with tier 4's
// graph capacities (256 nodes, 101 088 B) 977 of 997 windows of a 150x pile overflow the node table, with tier 11's (1536 nodes, 129 568 B) 644 of
// 997 at k = 8; only tier 3's held every window, so a lighter variant with more than one wavefront per CU does not pay.
// mins: the tier takes only the windows with MORE strings than that and passes the others on untouched (tier 3 runs what it ran before).
// String ids stay 8 bits in the compact string list of the instance generation (maxs <= 256); a k-mer seen more than 255 times does not fit
// the node frequency byte and sends the window on (buildNodes: overflow bit 2), nothing wraps.
template<> struct FastTier<12> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 1000, gw = 1, wcapg = 8192, rch = 8, fch = 16, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 250, precap = 8192, ncap = 2048, scap = 1024, lcap = 4096, wcap = 8192, rccap = 2048, fcap = 512, siqcap = 256, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 2560, wide = 0, mins = 96, gmem = 0 }; };

// tiers 13 and 14: the LAST stage, behind the slots and in front of the generic engine (tier_pipeline.hpp: ID_LAST).  gmem: the whole layout FastLds<CT>
// lives in the workgroup's slab in device memory instead of LDS (k_fast_13.hip / k_fast_14.hip compile this header with LDSQ = the global address
// space; nothing else changes -- the emulation has always run the tiers over a plain buffer).  A dependent load that hits L2 costs 180 ... 225 cycles
// against about 50 for ds_read, so a window costs a few times what it costs in tier 3 -- and not the seconds of the generic engine, which recomputes
// stretches, feasibility and both enumerations for every (first, last) k-mer pair.  Without the 160 KiB of a CU as a bound every table is at least
// as large as the largest of tiers 3, 6, 9, 10, 11 and 12, and the tables that have sent windows to the generic engine are twice tier 3's (tier 9's
// in the wide tier 14): nodes, stretches, links, weights, both pools, score intervals; 16384 k-mer instances.
//  - reverse pool: 4096 paths in 256 chunks of 16 (8 bit chunk ids kept: tier 3 has 256 chunks of 8, so an enumeration needs at most as many chunks here);
//  - 16 bit weight offsets and task offsets kept: 16384 weight records per direction, at most 65535 (stretch, direction, position) tasks per traversal;
//  - more than 4094 nodes: the stretch sort key takes 13 bit node fields and a 12 bit stretch number (FastEngine: KF, QB).
// Windows of more than 250 strings go on to tiers 15, 16 and 18; wider than 127 bases or with a string of more than 128 bases they still go to the generic engine.
template<> struct FastTier<13> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 2000, gw = 1, wcapg = 16384, rch = 16, fch = 16, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 250, precap = 16384, ncap = 4096, scap = 2048, lcap = 8192, wcap = 16384, rccap = 4096, fcap = 1024, siqcap = 512, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 4096, wide = 0, mins = 0, gmem = 1 }; };
template<> struct FastTier<14> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 1000, gw = 1, wcapg = 16384, rch = 16, fch = 16, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 250, precap = 16384, ncap = 6144, scap = 1024, lcap = 8192, wcap = 16384, rccap = 4096, fcap = 2048, siqcap = 512, blcap = 128, seqcap = 96, psiq = 10, consrow = 128, lscrids = 4096, wide = 1, mins = 0, gmem = 1 }; };
// tier 15: the VERY DEEP stage, behind the last stage and in front of the generic engine (tier_pipeline.hpp: ID_VDEEP): windows of 251 ... 1000 strings
// (a repeat pile of several hundred overlaps), which every other tier refuses at its string count and the generic engine runs at a handful of
// wavefronts (its arena is 200 MB per wavefront at depth 1000).  Tier 13's graph, pool, weight and interval capacities with 1000 strings and 65536
// k-mer instances (FastLds<CT>::icap = 4 x precap: the instances are split by their first symbol into four ranges, each sorted on its own with the sort
// of 16384 keys that tier 13 has -- precap stays the capacity of one sort); mins = 250: what tier 13 could have held is passed on as it came.  What a string count above 256 widens (FastLds<CT>::wides, all
// other tiers keep their fields bit for bit):
//  - compact string list of the instance generation: 10 bit string id | 16 bit first slot (4 x 1000 bytes <= the 65536 bytes of irpos);
//  - node frequency: 16 bits, capped at fqmax = 1023 -- a k-mer seen more often sets overflow bit 2 and the window goes on, nothing wraps;
//  - node weight: at most 1023 table words of < 2^32, so < 2^42 (10 bit high part); a feasible stretch has at most nrows <= 64 nodes, so < 2^48
//    (16 bit high part, as before): the reverse record packs 16 + 10 bits into its third word, the forward record (16 + 10 + 10 = 36 bits) becomes
//    32 bytes of three 64 bit words; path weights (rc_w, f_w, score intervals, candidates) are 64 bit sums of at most FSEQCAP stretches, < 2^54;
//  - first instance of a node (nps): 32 bits, 1000 strings carry up to 65536 instances;
//  - the 16 chunks of 64 strings of the instance generation are walked twice (count, then place) instead of being kept in 48 registers;
//  - key tables (mfirst, mlast, lastk) of 1024 entries, 16000 candidate error bytes.
// One capacity is not tier 13's: 32768 weight records per direction instead of 16384 (the 16 bit weight offsets hold that).  At k = 8 a window of
// 700 strings has a graph of 2100 nodes in 1200 stretches at filter frequency 2, and 24 of the 197 windows of such a pile have more than 16384
// feasible (stretch, position) pairs in one direction (emulation, tests/vdeep_cases.py shape D); the slab is device memory, the records cost 1.5 MB.
template<> struct FastTier<15> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 2000, gw = 1, wcapg = 32768, rch = 16, fch = 16, fnw = 4, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 128, maxs = 1000, precap = 16384, ncap = 4096, scap = 2048, lcap = 8192, wcap = 32768, rccap = 4096, fcap = 1024, siqcap = 512, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 4096, wide = 0, mins = 250, gmem = 1 }; };

static_assert(uint32_t(FastTier<15>::mins) == VDEEP_MINS && uint32_t(FastTier<13>::maxs) == VDEEP_MINS,"the very deep stage takes what the last stage refuses at its string count");
// tier 16: the DEEPEST stage, behind the very deep stage and in front of the generic engine (tier_pipeline.hpp: ID_XDEEP): windows of 1001 ... 2000 strings
// and the windows of 251 ... 1000 strings that overflowed one of tier 15's tables (mins = 250: everything else is passed on as it came).  Tier 15's code
// with twice its graph: 8190 nodes (the most the 13 bit node fields of the stretch sort key name), 4096 stretches (its 12 bit stretch number), 16384
// links, 4000 pool stretches.  What a string count above 1024 widens (FastLds<CT>::xwides, all other tiers keep their fields bit for bit):
//  - compact string list: 11 bit string id | 17 bit first slot;
//  - node frequency capped at fqmax = 4095: node weight < 2^44 (12 bit high part), stretch weight < 2^50 (18 bit high part), the reverse record's third
//    word holds 18 + 12 bits; the forward record is the three 64 bit words of tier 15;
//  - 131072 k-mer instances (icap = 8 x precap) as 64 ranges by the first three symbols of the k-mer: a histogram pass counts them, every range is sorted
//    with the sort of precap = 16384 keys (a uniform window of 2000 strings has 5200 in its largest range); a range of more than precap hands the window on;
//  - 32 bit task offsets and weight offsets (FastLds<CT>::toff_t): a traversal of 3400 stretches at k = 8 has more than 65535 (stretch, direction,
//    position) tasks and up to 45324 feasible ones in a direction, so 65536 weight records per direction (with tier 15's 32768, 19 of the 37 windows of
//    tests/xdeep_cases.py shape P overflow at k = 8; with 65536 none).
// Pools, intervals and the lane scratch are tier 15's: the pending-path heap of a reverse enumeration that outgrows its lane's 32 ids is run again on the
// whole scratch (lscrids = 4096 ids), which holds every path of the pool (rccap = 4096), so it never sends a window on by itself.
template<> struct FastTier<16> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 4000, gw = 1, wcapg = 65536, rch = 16, fch = 16, fnw = 4, fnc = 72, idmax = 8000, rpstcap = 768, lstr = 128, maxs = 2000, precap = 16384, ncap = 8190, scap = 4096, lcap = 16384, wcap = 65536, rccap = 4096, fcap = 1024, siqcap = 512, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 4096, wide = 0, mins = 250, gmem = 1 }; };
static_assert(uint32_t(FastTier<16>::mins) == VDEEP_MINS && uint32_t(FastTier<15>::maxs) == XDEEP_MINS,"the deepest stage takes what the very deep stage hands on with more than 250 strings");
// tier 18: the FULL-DEPTH stage, behind the deepest stage and in front of the generic engine (tier_pipeline.hpp: ID_FDEEP): windows of 2001 ... 5001 strings
// -- 5001 is the deepest window a default run submits (-D 5000 overlaps and the A read) -- and the windows of 251 ... 2000 strings that overflowed one of
// tier 16's tables (mins = 250).  Tier 16's code with twice its node table and capacities sized on the emulation (tests/fdeep_cases.py): 16384 nodes,
// 12288 stretches, 49152 links, 12000 pool stretches, 131072 weight records per direction -- at k = 8 the deepest pile of a default run needs 9005 stretches
// and 121390 forward records.  What a string
// count above 2048 widens (FastLds<CT>::ywides, all other tiers keep their fields bit for bit):
//  - compact string list: 13 bit string id | 18 bit first slot;
//  - 262144 k-mer instances (icap = 16 x precap) as 256 ranges by the first FOUR symbols of the k-mer (k >= 4; a window at k = 3 is handed on), every range
//    sorted with the sort of precap = 16384 keys;
//  - stretch sort key: 15 bit node fields (FastEngine: KF).  The base sort orders (first, ext) and the stretch number alone -- two stretches that share
//    (first, ext) send the window on, so length and last node never decide an order that is kept --: 15 + 15 + 14 bits.  The pool key keeps its four
//    fields, 60 bits, and carries no stretch number;
//  - key tables (mfirst, mlast, lastk) of 8192 entries, 80016 candidate error bytes, 79 chunks of 64 strings in the instance generation.
//  - the four words per (stretch, direction) unit of the stretch feasibility live in device memory (the bytes of pregen), not in 4 x 384 registers.
// Node frequencies stay capped at fqmax = 4095, so the weight widths are tier 16's.  Node ids, stretch ids and link offsets stay 16 bit words: 16384 nodes,
// 12288 stretches and 49152 links are below 65535 (0xFFFF stays "none").
template<> struct FastTier<18> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 12000, gw = 1, wcapg = 131072, rch = 16, fch = 16, fnw = 4, fnc = 72, idmax = 24000, rpstcap = 768, lstr = 128, maxs = 5001, precap = 16384, ncap = 16384, scap = 12288, lcap = 49152, wcap = 131072, rccap = 4096, fcap = 1024, siqcap = 512, blcap = 128, seqcap = 48, psiq = 10, consrow = 96, lscrids = 4096, wide = 0, mins = 250, gmem = 1 }; };
static_assert(uint32_t(FastTier<18>::mins) == VDEEP_MINS && uint32_t(FastTier<16>::maxs) == FDEEP_MINS,"the full-depth stage takes what the deepest stage hands on with more than 250 strings");
// tier 17: the LONG STRING stage of wide batches, on the second stream in front of the generic engine there (tier_pipeline.hpp: ID_LONG): the windows the
// pre-scan set aside because a B string has more than 128 bases.  Tier 14 with a string stride of 256: FOUR 64 bit words per pattern mask (FastLds<CT>::pw),
// strings of up to 255 bases -- the lengths and positions of a string are bytes (slen, ipos, irpos, canderr) --, a longer one is FFAIL(4) = FW_GENERIC and
// goes on to the generic engine.  Tables, pools and the wide fields (two words per position mask, 128 symbol consensus, base lengths up to 191) are tier
// 14's: what a long string can make longer than those hold -- a forward base length, a candidate, a consensus -- is refused by the checks that refuse it in
// tier 14 (extendPath: over(2048), buildSeq: over(4096), FFAIL(9)) and the window goes on, nothing wraps (DESIGN 3.5 lists the audit).
// oneslab: the whole working set of a workgroup is ONE buffer whose first byte is the layout's (L.base); the weights, the spill image and the instance
// image follow the layout (FastLds<CT>::g_base) instead of preceding it, so a caller that has one buffer of FastCaps::ldsbytes for a stage and no slab
// (the emulation's ROLE_LONG stage) runs the tier as it is.  Tiers 13 ... 16 keep their addressing.
// tier 19: the WIDE DEEP stage of wide batches, behind the last stage (tier 14) and in front of the generic engine (tier_pipeline.hpp: ID_WDEEP): the windows of
// 251 ... 1000 strings at w = 64 ... 127, which tiers 8, 9 and 14 refuse at their string count (mins = 250: what tier 14 could have held is passed on as it came).
// Tier 14's code -- two words per position mask, 128 symbol consensus, the consensus -> A alignment inside the kernel -- under tier 15's compile-time widths
// (FastLds<CT>::wides: 10 bit string ids, 16 bit node frequencies capped at 1023, 32 bit nps, the 32 byte forward record, the two-pass instance generation, key
// tables of 1024 entries).  What the combination widens: a feasible stretch has up to 128 nodes here, 128 x 1023 table words < 2^49, so the high part of a stretch
// weight has 17 bits (FastEngine: SROWS, SWHB) and the reverse record's third word 17 + 10; path weights are sums of at most seqcap = 96 stretches, < 2^56, and
// live in whole 64 bit words.  What else the wide windows of several hundred strings need, sized on the emulation (tests/wdeep_cases.py):
//  - 131072 k-mer instances (FastLds<CT>::hranges: icap = 8 x precap in tier 16's 64 ranges by the first three symbols, each sorted with the sort of
//    precap = 16384 keys that tiers 13 ... 18 have; 17 bit first slots in the compact string list): 1000 strings of 100 bases carry 73800 at k = 10;
//  - 32 bit task and weight offsets (FastLds<CT>::toff32): 3000 stretches with up to 128 start positions are far more than 65535 tasks; 98304 weight records per direction;
//  - 8190 nodes, 4096 stretches (the 13 bit node fields and the 12 bit stretch number of the stretch sort key), 16384 links;
//  - reverse pool of 16384 paths in 256 chunks of rch = 64: an enumeration's 32 chunk ids then name 2048 paths, where 512 sent 71 of 77 windows of a pile on;
//    lscrids = 16384, so that the retry of a pending-path heap on the whole scratch holds every path of the pool;
//  - the per-unit words of the stretch feasibility in device memory, as in tier 18 (128 chunks would be 512 registers).
template<> struct FastTier<19> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 4000, gw = 1, wcapg = 98304, rch = 64, fch = 16, fnw = 4, fnc = 72, idmax = 8000, rpstcap = 768, lstr = 128, maxs = 1000, precap = 16384, ncap = 8190, scap = 4096, lcap = 16384, wcap = 98304, rccap = 16384, fcap = 2048, siqcap = 512, blcap = 128, seqcap = 96, psiq = 10, consrow = 128, lscrids = 16384, wide = 1, mins = 250, gmem = 1 }; };
static_assert(uint32_t(FastTier<19>::mins) == VDEEP_MINS && uint32_t(FastTier<14>::maxs) == VDEEP_MINS && uint32_t(FastTier<19>::maxs) == FastTier<15>::maxs,"the wide deep stage takes what the last stage of a wide batch refuses at its string count");
template<> struct FastTier<17> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 1000, gw = 1, wcapg = 16384, rch = 16, fch = 16, fnw = 8, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 256, maxs = 250, precap = 16384, ncap = 6144, scap = 1024, lcap = 8192, wcap = 16384, rccap = 4096, fcap = 4096, siqcap = 512, blcap = 128, seqcap = 96, psiq = 10, consrow = 128, lscrids = 4096, wide = 1, mins = 0, gmem = 1, oneslab = 1 }; };
// tier 20: the stage of a batch with w = 128 (tier_pipeline.hpp: ID_W128), in front of the generic engine, which used to run every window of such a batch.  Tier 17's row -- four
// words per pattern mask, strings of up to 255 bases, one slab, its gap filling region and forward pool -- with the three widths that w = 128 needs and no tier below it has
// (rows3: FastRows3<CT>, every other tier keeps its fields and its instruction stream):
//  - position masks of THREE 64 bit words (maskF / maskFh / maskFx): the model table of w = 128 has w + 1 = 129 rows, a stretch's feasible start positions are rows 0 ... w;
//    three words hold tables of up to 192 rows;
//  - candidates and a consensus of up to 192 symbols (consrow, FastLds<CT>::consmax): on deletion-rich reads the consensus of a window of 128 bases is longer than
//    128 symbols more often than not (123 ... 133 seen); the wide record holds 2 + 2 x 130 + 128 + 192 = 582 of its 640 bytes;
//  - blcap = 192 base lengths (three occupancy words, as the forward base lengths FBLMAX = 191 have had).
// One table is not tier 17's: the reverse pool.  With tier 17's 4096 paths in chunks of 16 -- an enumeration's 32 chunk ids name 512 paths -- 76 of 364 windows of the
// even error mix at k = 10 and 15 of 364 of the deletion-rich mix overflow it (flags 0x4200; emulation, tests/w128_cases.py shapes E and D): a window of 128 bases has
// reverse paths of twice the stretches.  Tier 19's pool instead: 16384 paths in 256 chunks of rch = 64, 2048 paths per enumeration, and lscrids = 16384, so that the retry
// of a pending-path heap on the whole scratch holds every path of the pool.
// A feasible stretch has up to 129 nodes of frequency at most 255: its weight stays below 2^48, the 16 bit high part (FastEngine: SROWS).
// Strings of more than 255 bases are FFAIL(4) = FW_GENERIC, more than 250 strings and table overflows FW_NEXT: the generic engine runs them.
template<> struct FastTier<20> { typedef uint16_t id_t; typedef uint16_t sid_t; enum : uint32_t { smax = 1000, gw = 1, wcapg = 16384, rch = 64, fch = 16, fnw = 8, fnc = 72, idmax = 4000, rpstcap = 768, lstr = 256, maxs = 250, precap = 16384, ncap = 6144, scap = 1024, lcap = 8192, wcap = 16384, rccap = 16384, fcap = 4096, siqcap = 512, blcap = 192, seqcap = 96, psiq = 10, consrow = 192, lscrids = 16384, wide = 1, mins = 0, gmem = 1, oneslab = 1, rows3 = 1 }; };
// (only tiers 17 and 20 name the enumerator: for every other tier FastOneSlab<CT>::value is 0)
template<typename CT, typename = void> struct FastOneSlab { enum : uint32_t { value = 0 }; };
template<typename CT> struct FastOneSlab<CT,decltype(void(CT::oneslab))> { enum : uint32_t { value = (CT::oneslab != 0) ? 1u : 0u }; };
// (only tier 20 names this one: three words per position mask, 192 symbol rows, 192 base lengths)
template<typename CT, typename = void> struct FastRows3 { enum : uint32_t { value = 0 }; };
template<typename CT> struct FastRows3<CT,decltype(void(CT::rows3))> { enum : uint32_t { value = (CT::rows3 != 0) ? 1u : 0u }; };

}
#endif
