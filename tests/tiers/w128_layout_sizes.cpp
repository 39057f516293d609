// TEST HARNESS: the sizes of the layout FastLds<FastTier<N>> of the tiers of DACC_W128_TIERS (tier 20, the tier of w = 128), in the form of
// tests/tiers/fast_layout_sizes.cpp, whose list (DACC_ALL_TIERS) and recording they are not part of.  tests/test_w128_tier.py builds this stand-alone
// program and compares its output byte for byte with tests/golden/w128_layout_sizes.txt.  It includes nothing of the engine.
#define DACC_EMUL 1
#include <wave.hpp>
#include <fast_layout.hpp>
#include <cstdio>
using namespace dacc;

template<int N> static void row()
{
	typedef FastTier<N> CT; typedef FastLds<CT> L;
	static_assert(L::o_bestL < L::uend && L::uA <= L::uend && L::upool <= L::uend && L::gfcap*8u <= L::uend,"the layout's size covers its regions");
	static_assert(L::rows3 && L::consmax == 192u && L::maskrows == 192u && L::e_maskRx - L::o_maskFx == 2u*8u*CT::scap,"the widths of the tier of w = 128");
	std::printf("tier %d bytes %u o_bestL %u ubase %u upool %u uA %u gfcap %u",N,unsigned(L::bytes(0,0)),unsigned(L::o_bestL),unsigned(L::ubase),unsigned(L::upool),unsigned(L::uA),unsigned(L::gfcap));
	std::printf(" sbytes %u g_total %u",unsigned(L::sbytes),unsigned(L::g_total));
	FastCaps const C = fastCapsOf<CT>(0,0);
	std::printf(" caps %u %u %u %u\n",C.precap,C.ldsbytes,C.gbytes,C.gmem);
}

int main()
{
#define DACC_ROW(N) row<N>();
	DACC_W128_TIERS(DACC_ROW)
#undef DACC_ROW
	return 0;
}
