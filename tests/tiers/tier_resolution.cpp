// TEST HARNESS: the tier chain as resolveTiers sees it (daccord_amd/csrc/tier_pipeline.hpp), one line per combination of batch shape, deepest window,
// model table and environment.  tests/test_tier_resolution.py builds this stand-alone program with g++ under AddressSanitizer and
// UndefinedBehaviorSanitizer (the project's headers as system headers: -isystem daccord_amd/csrc) and compares its output byte for byte with
// tests/golden/tier_resolution.txt.  It uses only what every version of the header keeps: readTierSwitches, TierSwitches::conflict / nofast,
// resolveTiers, stageTier, tierGrid, tierGridGmem, TIER_CHAIN, the TierId values, TierPipeline's members and tierCaps.
#define DACC_EMUL 1
#include <wave.hpp>
#include <batch_plan.hpp>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>
using namespace dacc;

typedef std::vector< std::pair<char const *,char const *> > Env;
static char const * const VARS[] = { "DACC_LAST_TIER","DACC_VDEEP_TIER","DACC_XDEEP_TIER","DACC_DEEP_TIER","DACC_DENSE_TIER","DACC_LONGSTR_TIER","DACC_WIDE_TIER",
	"DACC_LONG128","DACC_HAND","DACC_LAST_AS_SLOT2","DACC_VDEEP_AS_SLOT2","DACC_XDEEP_AS_SLOT2","DACC_TIERS","DACC_T7INST","DACC_T0INST","DACC_NOFAST","DACC_LDS_T1","DACC_LDS_T0" };

int main()
{
	std::vector<Env> envs;
	envs.push_back(Env());
	for ( char const * v : { "DACC_LAST_TIER","DACC_VDEEP_TIER","DACC_XDEEP_TIER","DACC_DEEP_TIER","DACC_DENSE_TIER","DACC_LONGSTR_TIER","DACC_WIDE_TIER","DACC_LONG128","DACC_HAND" } )
		envs.push_back(Env{ { v,"0" } });
	char const * const as2[3] = { "DACC_LAST_AS_SLOT2","DACC_VDEEP_AS_SLOT2","DACC_XDEEP_AS_SLOT2" };
	for ( unsigned m = 1; m < 8; ++m ) { Env e; for ( unsigned b = 0; b < 3; ++b ) if ( (m >> b) & 1 ) e.push_back({ as2[b],"1" }); envs.push_back(e); }
	for ( char const * t : { "0","4","25","29","31" } ) envs.push_back(Env{ { "DACC_TIERS",t } });
	envs.push_back(Env{ { "DACC_T7INST","576" },{ "DACC_T0INST","576" } });
	envs.push_back(Env{ { "DACC_NOFAST","1" } });
	// model tables (rows x read offsets): the default error profile (p_i = 0.12, p_d = 0.02) at w = 40 and at w = 100, and one whose (nrows+1)*(nsup+1)
	// exceeds every tabcap, that of the device-memory tiers (2^31-1) included
	struct { char const * name; uint32_t nrows, nsup; } const tabs[] = { { "w40",41,60 },{ "w100",101,133 },{ "huge",65535,65535 } };
	struct { char const * name; bool deep, wide; uint32_t w; } const shapes[] = { { "shallow",false,false,40 },{ "deep",true,false,40 },{ "wide",false,true,100 } };
	uint32_t const maxstrings[] = { 0,250,251,1000,1001,2001 };
	uint64_t const nwin = 37;      // (one window count keeps the recorded output small; the grids of 1 and 5000 windows add nothing the resolution decides)
	std::printf("# environment (DACC_ left out), batch shape, model table, strings of the deepest window | conflict usefast widetier handover late_long slot1_long | handwords | per stage in chain order: ok, tier, grid of %u windows\n",unsigned(nwin));
	for ( Env const & env : envs )
	{
		for ( char const * v : VARS ) unsetenv(v);
		std::string ename;
		for ( auto const & kv : env ) { setenv(kv.first,kv.second,1); ename += std::string(ename.size() ? "," : "") + (kv.first+5) + "=" + kv.second; }
		if ( !ename.size() ) ename = "default";
		for ( auto const & sh : shapes ) for ( auto const & tb : tabs ) for ( uint32_t const ms : maxstrings )
		{
			TierSwitches const S = readTierSwitches();
			FastCaps caps[TIER_NSTAGES];
			for ( uint32_t i = 0; i < TIER_NSTAGES; ++i ) caps[i] = tierCaps(stageTier(TIER_CHAIN[i],sh.deep,sh.wide),tb.nrows,tb.nsup);
			TierPipeline const R = resolveTiers(S,!S.nofast,sh.deep,sh.wide,tb.nrows,tb.nsup,sh.w,[&](uint32_t const id) -> FastCaps & { return caps[id]; },ms);
			std::printf("%s %s %s %u | %d%d%d%d%d%d | %u | ",ename.c_str(),sh.name,tb.name,ms,int(S.conflict()),int(R.usefast),int(R.widetier),int(R.handover),int(R.late_long),int(R.slot1_long),R.handwords);
			for ( uint32_t i = 0; i < TIER_NSTAGES; ++i ) std::printf("%d",int(R.ok[i]));
			for ( uint32_t i = 0; i < TIER_NSTAGES; ++i ) std::printf("%c%u",i ? ',' : ' ',R.tier[i]);
			for ( uint32_t i = 0; i < TIER_NSTAGES; ++i ) std::printf("%c%u",i ? ',' : ' ',caps[i].gmem ? tierGridGmem(caps[i].gbytes,nwin) : tierGrid(caps[i].ldsbytes,nwin));
			std::printf("\n");
		}
	}
	return 0;
}
