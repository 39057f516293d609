/*
 * TEST HARNESS ONLY: the launch arithmetic of the batch setup (daccord_amd/csrc/launch_geometry.hpp) against values worked out by hand from the expressions
 * dacc_submit_piles_body held inline before the header existed (T2C = 8, T2S = 4, TRS = 16, TRACE2_LDS = 4*64*32 = 8192).  Every expected value carries its
 * arithmetic; every threshold has both neighbours.  Prints one line per failed check; exit status 1 if there is one.
 */
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "launch_geometry.hpp"

using namespace dacc;

static int nfail = 0, nchecks = 0;
static void eq(char const * const what, uint64_t const got, uint64_t const want)
{
	++nchecks;
	if ( got != want ) { std::printf("FAIL %s: got %llu, want %llu\n",what,static_cast<unsigned long long>(got),static_cast<unsigned long long>(want)); ++nfail; }
}
// a trace geometry that fits: words, lanes, LDS bytes, workgroups per CU, grid
static void trace(char const * const what, int32_t const tspace, uint32_t const maxcols, uint64_t const nblocks, uint64_t const ovr,
	uint32_t const words, uint32_t const lanes, uint32_t const lds, uint64_t const percu, uint32_t const grid)
{
	TraceGeometry const G = traceGeometry(tspace,maxcols,nblocks,ovr);
	std::printf("%s: words %u lanes %u lds %u fits %d percu %llu grid %u\n",what,G.words,G.lanes,G.lds,int(G.fits),static_cast<unsigned long long>(G.percu),G.grid);
	eq(what,G.fits,1); eq(what,G.words,words); eq(what,G.lanes,lanes); eq(what,G.lds,lds); eq(what,G.percu,percu); eq(what,G.grid,grid);
}

int main()
{
	static_assert(T2C == 8 && T2S == 4 && TRS == 16 && TRACE2_LDS == 8192,"the constants the values below are worked out with");
	// ---- sizing helpers
	eq("traceCheckpoints(160)",traceCheckpoints(160),21);               // 160/8 + 1
	eq("traceSlabWords(160)",traceSlabWords(160),5376);                 // 21 * 4 * 64
	eq("traceCheckpoints(928)",traceCheckpoints(928),117);              // 928/8 + 1
	eq("traceSlabWords(928)",traceSlabWords(928),29952);                // 117 * 256
	eq("traceSlots(929)",traceSlots(929),75);                           // 929/16 + 1 + 16 = 58 + 17
	eq("traceWideBytesPerLane<4>(929)",traceWideBytesPerLane<4>(929),4950);       // 75 * (16*4 + 2) = 75 * 66
	eq("traceWideBytesPerLane<8>(4096)",traceWideBytesPerLane<8>(4096),35490);    // (256 + 17) * (16*8 + 2) = 273 * 130
	eq("traceWideBytesPerLane<8>(2048)",traceWideBytesPerLane<8>(2048),18850);    // (128 + 17) * 130 = 145 * 130

	// ---- the choice of kernel: two words for tspace <= 128 and maxcols <= 928, four up to tspace 256, else eight
	eq("words 128/928",traceWords(128,928),2); eq("words 128/929",traceWords(128,929),4); eq("words 129/928",traceWords(129,928),4); eq("words 1/0",traceWords(1,0),2);
	eq("words 256/160",traceWords(256,160),4); eq("words 257/160",traceWords(257,160),8); eq("words 512/160",traceWords(512,160),8); eq("words 256/929",traceWords(256,929),4);

	// ---- two word kernel, one byte trace: LDS 8192 -> 7 granules of 1280 = 8960 B, 163840/8960 = 18 per CU (below the cap of 20); 1 000 000 blocks = 15625 rounds
	// of 64 lanes, more than 256*18 = 4608; slab (160/8+1) * 256 words * 8 = 43008 B per workgroup, 4608 * 43008 = 198 180 864 <= 192 MiB = 201 326 592: no step-down
	trace("two words, maxcols 160",100,160,1000000,0, 2,64,8192,18,4608);
	trace("two words, tspace 128",128,160,1000000,0, 2,64,8192,18,4608);
	// the longest block it takes: slab 117 * 256 * 8 = 239616 B; from 4608 down by 256 while above the bound: 1024 * 239616 = 245 366 784 (above), 768 * 239616 = 184 025 088 (below)
	trace("two words, maxcols 928",100,928,1000000,0, 2,64,8192,18,768);
	// the step-down ends at one workgroup per CU whatever the slab: 300 blocks = 5 rounds stay 5
	trace("two words, maxcols 928, 300 blocks",100,928,300,0, 2,64,8192,18,5);
	// blocks -> rounds of 64, at least one workgroup
	trace("two words, 0 blocks",100,160,0,0, 2,64,8192,18,1);
	trace("two words, 1 block",100,160,1,0, 2,64,8192,18,1);
	trace("two words, 64 blocks",100,160,64,0, 2,64,8192,18,1);
	trace("two words, 65 blocks",100,160,65,0, 2,64,8192,18,2);
	trace("two words, 4608 rounds",100,160,4608*64,0, 2,64,8192,18,4608);
	trace("two words, 4607 rounds + 1",100,160,4606*64+1,0, 2,64,8192,18,4607);
	// the override, 1 ... 32 (slab of maxcols 7: one checkpoint, 2048 B, never binds): 1 -> 256 workgroups, 32 -> 8192, 33 and 0 are no override
	trace("two words, percu 1",100,7,1000000,1, 2,64,8192,1,256);
	trace("two words, percu 32",100,7,1000000,32, 2,64,8192,32,8192);
	trace("two words, percu 33",100,7,1000000,33, 2,64,8192,18,4608);
	trace("two words, percu 0",100,7,1000000,0, 2,64,8192,18,4608);
	// the override and the slab bound together: 8192 * 43008 is above 192 MiB; 4864 * 43008 = 209 190 912 still is, 4608 * 43008 = 198 180 864 is not
	trace("two words, percu 32, maxcols 160",100,160,1000000,32, 2,64,8192,32,4608);

	// ---- four word kernel at tspace <= 128: 4950 B per lane, 64 lanes = 316800 > 163840, 32 lanes = 158400 fit; 124 granules = 158720 B, one workgroup per CU;
	// grid = min(ceil(nblocks/32), 256 * 1 * 4)
	trace("four words, maxcols 929",100,929,1000000,0, 4,32,158400,1,1024);
	trace("four words, maxcols 929, 1000 blocks",100,929,1000,0, 4,32,158400,1,32);      // ceil(1000/32)
	trace("four words, maxcols 929, 0 blocks",100,929,0,0, 4,32,158400,1,1);
	trace("four words, percu 32",100,929,1000000,32, 4,32,158400,32,31250);               // 256*32*4 = 32768 > ceil(1 000 000/32) = 31250
	trace("four words, percu 33",100,929,1000000,33, 4,32,158400,1,1024);
	// tspace 129: (160/16 + 17) * 66 = 1782 B per lane, 64 lanes = 114048 fit; 90 granules = 115200, 163840/115200 = 1
	trace("four words, tspace 129",129,160,1000000,0, 4,64,114048,1,1024);
	trace("four words, tspace 256",256,160,100,0, 4,64,114048,1,2);                       // ceil(100/64)
	// a short block: (0/16 + 17) * 66 = 1122 B per lane, 64 lanes = 71808; 57 granules = 72960, 163840/72960 = 2 per CU (the cap of 8 is out of reach: it never binds)
	trace("four words, maxcols 0",200,0,1000000,0, 4,64,71808,2,2048);
	// ---- eight word kernel: tspace 257, 27 * 130 = 3510 B per lane, 64 lanes = 224640 do not fit, 32 lanes = 112320 do; 88 granules = 112640, one per CU
	trace("eight words, tspace 257",257,160,1000000,0, 8,32,112320,1,1024);
	// tspace 300, maxcols 2048: 18850 B per lane, 16 lanes = 301600 do not fit, 8 lanes = 150800 do; 118 granules = 151040, one per CU; grid min(ceil(nblocks/8), 1024)
	trace("eight words, maxcols 2048",300,2048,1000000,0, 8,8,150800,1,1024);
	trace("eight words, maxcols 2048, 20 blocks",300,2048,20,0, 8,8,150800,1,3);
	// the largest that fits: 8 lanes * 130 * slots <= 163840 <=> slots <= 157 <=> maxcols/16 <= 140: maxcols 2255 (8 * 157 * 130 = 163280; 128 granules = 163840 exactly, one per CU)
	trace("eight words, maxcols 2255",300,2255,1000000,0, 8,8,163280,1,1024);
	// ---- too large for the trace kernels: never fewer than 8 lanes; maxcols 2256: 8 * 158 * 130 = 164320 > 163840; maxcols 4096: 8 * 35490 = 283920
	{ TraceGeometry const G = traceGeometry(300,2256,1000000,0); eq("2256: words",G.words,8); eq("2256: lanes",G.lanes,8); eq("2256: lds",G.lds,164320); eq("2256: fits",G.fits,0); }
	{ TraceGeometry const G = traceGeometry(300,4096,1000000,0); eq("4096: words",G.words,8); eq("4096: lanes",G.lanes,8); eq("4096: lds",G.lds,283920); eq("4096: fits",G.fits,0); }

	// ---- the 32 bit counter k_trace draws its rounds from
	eq("counter, 0xFFFFFEFF blocks",traceCounterHolds(0xFFFFFEFFull),1); eq("counter, 0xFFFFFF00 blocks",traceCounterHolds(0xFFFFFF00ull),0); eq("counter, 0 blocks",traceCounterHolds(0),1);

	// ---- boundByArena: halve while above mingrid and grid * bytes above 32 GiB = 34 359 738 368
	eq("bound 512 x 200 MB",boundByArena(512,200000000ull,8),128);      // 512: 1.024e11, 256: 5.12e10 (above); 128: 2.56e10 (below)
	eq("bound at mingrid",boundByArena(8,10000000000ull,8),8);           // 8e10 is above, but the grid is at its minimum
	eq("bound to mingrid",boundByArena(64,10000000000ull,8),8);          // 64, 32, 16 (1.6e11) above; stops at 8
	eq("bound, no arena",boundByArena(512,0,8),512);
	eq("bound, exactly 32 GiB",boundByArena(32,1ull<<30,8),32);          // 32 * 2^30 = 2^35: not above
	eq("bound, one byte more",boundByArena(32,(1ull<<30)+1,8),16);
	eq("bound, no grid",boundByArena(0,1,0),1);                          // never 0

	// ---- the generic engine behind a chain: wg = nwindows rounded up to 8, within 8 ... 2048; retry_grid = win_grid = bound(min(wg,512)); early_grid = min(retry_grid,256),
	// halved while above 16 and early_grid * bytes above 8 GiB = 8 589 934 592
	{ GenericGeometry const G = genericGeometry(1000000,7000000,true); eq("chain 7 MB: retry",G.retry_grid,512); eq("chain 7 MB: win",G.win_grid,512); eq("chain 7 MB: early",G.early_grid,256); }      // 512 * 7e6 = 3.6e9; 256 * 7e6 = 1.8e9
	{ GenericGeometry const G = genericGeometry(1000000,1ull<<25,true); eq("chain 2^25: retry",G.retry_grid,512); eq("chain 2^25: early",G.early_grid,256); }        // 256 * 2^25 = 8 GiB exactly: not above; 512 * 2^25 = 16 GiB
	{ GenericGeometry const G = genericGeometry(1000000,(1ull<<25)+1,true); eq("chain 2^25+1: retry",G.retry_grid,512); eq("chain 2^25+1: early",G.early_grid,128); }  // 256 * (2^25+1) is above, 128 * (2^25+1) = 2^32 + 128 is not
	// the default -D: 800 MB per wavefront: 512 ... 64 (5.12e10) above 32 GiB, 32 (2.56e10) below; early: 32 * 8e8 is above 8 GiB, 16 is the floor (1.28e10 is still above)
	{ GenericGeometry const G = genericGeometry(1000000,800000000ull,true); eq("chain 800 MB: retry",G.retry_grid,32); eq("chain 800 MB: win",G.win_grid,32); eq("chain 800 MB: early",G.early_grid,16); }
	{ GenericGeometry const G = genericGeometry(5,7000000,true); eq("chain, 5 windows: retry",G.retry_grid,8); eq("chain, 5 windows: early",G.early_grid,8); }
	{ GenericGeometry const G = genericGeometry(0,7000000,true); eq("chain, 0 windows: retry",G.retry_grid,8); eq("chain, 0 windows: early",G.early_grid,8); }
	{ GenericGeometry const G = genericGeometry(300,7000000,true); eq("chain, 300 windows: retry",G.retry_grid,304); eq("chain, 300 windows: early",G.early_grid,256); }     // 300 -> 304
	{ GenericGeometry const G = genericGeometry(513,7000000,true); eq("chain, 513 windows: retry",G.retry_grid,512); }      // 520, within 512
	// alone: win_grid = retry_grid = bound(wg), nothing on the second stream
	{ GenericGeometry const G = genericGeometry(1000000,7000000,false); eq("alone 7 MB: win",G.win_grid,2048); eq("alone 7 MB: retry",G.retry_grid,2048); eq("alone 7 MB: early",G.early_grid,0); }     // 2048 * 7e6 = 1.4e10
	{ GenericGeometry const G = genericGeometry(1000000,200000000ull,false); eq("alone 200 MB: win",G.win_grid,128); eq("alone 200 MB: retry",G.retry_grid,128); }      // 2048 ... 256 above, 128 * 2e8 = 2.56e10 below
	{ GenericGeometry const G = genericGeometry(37,7000000,false); eq("alone, 37 windows",G.win_grid,40); }
	{ GenericGeometry const G = genericGeometry(2041,7000000,false); eq("alone, 2041 windows",G.win_grid,2048); }
	{ GenericGeometry const G = genericGeometry(2049,7000000,false); eq("alone, 2049 windows",G.win_grid,2048); }      // 2056, within 2048

	// ---- hand-over capacity: nwindows/3 + 4096 slots, within 16 GiB / (handwords * 8): shallow 2^34 / 8736 = 1 966 560, deep 2^34 / 17440 = 985 084
	eq("hand, 1 M windows",handOverCapacity(1000000,1092,false,false,true),337429);           // 333333 + 4096
	eq("hand, 0 windows",handOverCapacity(0,1092,false,false,true),4096);
	eq("hand, shallow, at the cap",handOverCapacity(5887392,1092,false,false,true),1966560);  // 1962464 + 4096 = the cap itself
	eq("hand, shallow, below the cap",handOverCapacity(5887391,1092,false,false,true),1966559);
	eq("hand, shallow, capped",handOverCapacity(5887395,1092,false,false,true),1966560);      // 1962465 + 4096 = 1966561
	eq("hand, shallow, 10 M windows",handOverCapacity(10000000,1092,false,false,true),1966560);
	eq("hand, deep, at the cap",handOverCapacity(2942964,2180,false,false,true),985084);      // 980988 + 4096
	eq("hand, deep, capped",handOverCapacity(2942967,2180,false,false,true),985084);          // 980989 + 4096 = 985085
	eq("hand, deep, 10 M windows",handOverCapacity(10000000,2180,false,false,true),985084);
	// zero: a k range, a context that gave the buffer up, DACC_HAND=0, a wide batch (the last two are TierPipeline::handover); and every combination of them
	for ( int m = 1; m < 8; ++m ) eq("hand, switched off",handOverCapacity(10000000,1092,m&1,m&2,!(m&4)),0);

	// ---- dacc_last_timing2(size): below 176 the size itself, then the largest of 176, 192, 208, 224, 240 not above it
	for ( size_t size = 0; size <= 260; ++size )
	{
		size_t const want = size < 176 ? size : size < 192 ? 176 : size < 208 ? 192 : size < 224 ? 208 : size < 240 ? 224 : 240;
		eq("timing copy size",timingCopySize(size),want);
	}
	eq("timing copy size, large",timingCopySize(1u<<20),240);

	std::printf("%d checks, %d failed\n",nchecks,nfail);
	return nfail ? 1 : 0;
}
