// TEST HARNESS: how resolveTiers (daccord_amd/csrc/tier_pipeline.hpp) resolves a batch of w = 128 with all rows of TIER_CHAIN (rows = TIER_NROWS, as the
// library calls it), under the switches of the environment it is started with.  tests/test_w128_tier.py builds this stand-alone program with g++ under
// AddressSanitizer and UndefinedBehaviorSanitizer and reads its one line:
//   conflict usefast widetier anytier | ok and tier of ID_W128, ID_SLOT2, ID_LONG | number of other rows that are ok | the same for a wide batch of w = 100
// argv[1], argv[2]: rows and read offsets of the model table of w = 128 (default 129 x 170)
#define DACC_EMUL 1
#include <wave.hpp>
#include <batch_plan.hpp>
#include <cstdio>
#include <cstdlib>
using namespace dacc;

static void line(uint32_t const w, uint32_t const nrows, uint32_t const nsup)
{
	TierSwitches const S = readTierSwitches();
	bool const wide = w > 63 && w <= W128;      // BatchPlan::wide
	FastCaps caps[TIER_NROWS];
	for ( uint32_t i = 0; i < TIER_NROWS; ++i ) caps[i] = tierCaps(stageTier(TIER_CHAIN[i],false,wide,w),nrows,nsup);
	TierPipeline const R = resolveTiers(S,!S.nofast,false,wide,nrows,nsup,w,[&](uint32_t const id) -> FastCaps & { return caps[id]; },0,TIER_NROWS);
	unsigned others = 0;
	for ( uint32_t i = 0; i < TIER_NROWS; ++i ) if ( i != ID_W128 && i != ID_SLOT2 && i != ID_LONG && R.ok[i] ) ++others;
	std::printf("%d %d %d %d | %d %u %d %u %d %u | %u",int(S.conflict()),int(R.usefast),int(R.widetier),int(R.anytier()),int(R.ok[ID_W128]),R.tier[ID_W128],
		int(R.ok[ID_SLOT2]),R.tier[ID_SLOT2],int(R.ok[ID_LONG]),R.tier[ID_LONG],others);
}

int main(int argc, char ** argv)
{
	uint32_t const nrows = argc > 1 ? static_cast<uint32_t>(atoi(argv[1])) : 129u, nsup = argc > 2 ? static_cast<uint32_t>(atoi(argv[2])) : 170u;
	line(128,nrows,nsup);
	std::printf(" || ");
	line(100,101,133);
	std::printf("\n");
	return 0;
}
