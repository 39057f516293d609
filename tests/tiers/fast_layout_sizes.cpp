// TEST HARNESS: the sizes of the layout FastLds<FastTier<N>> (daccord_amd/csrc/fast_layout.hpp over the rows of fast_tiers.hpp), one line per tier of
// DACC_ALL_TIERS.  tests/test_fast_headers.py builds this stand-alone program with g++ the way tests/test_tier_resolution.py builds its own (1-lane host
// build of the device headers, wave.hpp first, the project's headers as system headers) and compares its output byte for byte with
// tests/golden/fast_layout_sizes.txt, recorded before the tier table and the layout left fast_window.hpp: a row or a field that was dropped, changed or
// put elsewhere on the way moves one of these numbers.  It includes nothing of the engine.
#define DACC_EMUL 1
#include <wave.hpp>
#include <fast_layout.hpp>
#include <cstdio>
using namespace dacc;

template<int N> static void row()
{
	typedef FastTier<N> CT; typedef FastLds<CT> L;
	// a layout is a set of constants (bytes() itself is an ordinary function of them)
	static_assert(L::o_bestL < L::uend && L::uA <= L::uend && L::upool <= L::uend && L::gfcap*8u <= L::uend,"the layout's size covers its regions");
	std::printf("tier %d bytes %u o_bestL %u ubase %u upool %u uA %u gfcap %u",N,unsigned(L::bytes(0,0)),unsigned(L::o_bestL),unsigned(L::ubase),unsigned(L::upool),unsigned(L::uA),unsigned(L::gfcap));
	if constexpr ( CT::gw != 0 ) std::printf(" sbytes %u g_total %u",unsigned(L::sbytes),unsigned(L::g_total));
	FastCaps const C = fastCapsOf<CT>(0,0);
	std::printf(" caps %u %u %u %u\n",C.precap,C.ldsbytes,C.gbytes,C.gmem);
}

int main()
{
#define DACC_ROW(N) row<N>();
	DACC_ALL_TIERS(DACC_ROW)
#undef DACC_ROW
	return 0;
}
