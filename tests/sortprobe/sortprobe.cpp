/*
 * TEST HARNESS ONLY (libsortprobe.so, g++ on demand; with -DSORTPROBE_MAIN a stand-alone program): the three replays of libstdc++'s std::sort
 * on the reverse paths of a window -- WindowEngine::arpSort of the generic engine (dbg_window.hpp) and FastEngine::arpSort / arpSortK of the
 * tiers (fast_window.hpp) -- run on caller-supplied (front, baselen) keys, one call at a time, as the 1-lane host build of the device headers.
 * The expected permutation is std::sort itself over an array of structs with the same comparator, compiled in here.
 *
 * Whether the generic engine took the heapsort fallback of introsort is learnt through DACC_ARP_FALLBACK_NOTE, a hook of dbg_window.hpp that is
 * empty in every other build; the tiers do not reproduce the fallback and report flag 1024 instead.
 */
#define DACC_EMUL 1
#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
static int sortprobe_fallbacks = 0;
#define DACC_ARP_FALLBACK_NOTE() (++::sortprobe_fallbacks)
#include "../../daccord_amd/csrc/batch_plan.hpp"
#include "../../daccord_amd/csrc/window_main.hpp"
#include "../../daccord_amd/csrc/fast_window.hpp"

using namespace dacc;

namespace {

struct Key { uint32_t front; uint16_t baselen; int32_t idx; };
struct KeyLess { bool operator()(Key const & a, Key const & b) const { if ( a.front != b.front ) return a.front < b.front; return a.baselen < b.baselen; } };

// the tier copies: ids 0 .. n-1 in the reverse cache of a tier, every path on a stretch of its own front k-mer
template<typename CT>
int tierSort(bool const keyed, uint32_t const * front, uint16_t const * baselen, uint32_t const n, int32_t * perm, uint32_t * flags)
{
	typedef FastLds<CT> LT; typedef typename CT::id_t id_t;
	if ( n > CT::rccap || (n && n-1 > static_cast<uint32_t>(static_cast<id_t>(~static_cast<id_t>(0)))) ) return 2;
	for ( uint32_t i = 0; i < n; ++i ) if ( baselen[i] > 255 ) return 3;
	std::vector<uint32_t> D(front,front+n); std::sort(D.begin(),D.end()); D.erase(std::unique(D.begin(),D.end()),D.end());
	uint32_t const stretchmax = std::min<uint32_t>(std::min<uint32_t>(CT::scap,CT::ncap),sizeof(typename LT::sid_t) == 1 ? 255u : 65535u);
	if ( D.size() > stretchmax ) return 4;
	uint32_t const bytes = std::max(std::max(LT::e_rc_front,LT::e_sstack),std::max(LT::e_sfirst,LT::e_nv)) + 64;
	std::vector<uint64_t> lds((bytes+7)/8,0);
	static FastEngine<CT> F; std::memset(&F,0,sizeof(F));
	F.L.base = reinterpret_cast<uint8_t *>(lds.data());
	for ( uint32_t j = 0; j < D.size(); ++j ) { F.L.sfirst()[j] = j; F.L.nv()[j] = D[j]; }
	std::vector<id_t> ord(n+1); std::vector<uint64_t> keys(n+1);
	for ( uint32_t i = 0; i < n; ++i )
	{
		F.L.rc_len()[i] = 1; F.L.rc_stretch()[i] = std::lower_bound(D.begin(),D.end(),front[i]) - D.begin(); F.L.rc_baselen()[i] = baselen[i];
		ord[i] = i; keys[i] = (static_cast<uint64_t>(front[i]) << 8) | baselen[i];
	}
	if ( keyed ) F.arpSortK(ord.data(),keys.data(),static_cast<int32_t>(n));
	else F.arpSort(ord.data(),ord.data()+n,0);
	for ( uint32_t i = 0; i < n; ++i ) perm[i] = ord[i];
	*flags = F.flags;
	return 0;
}

}

extern "C" {

enum { SP_GENERIC = 0, SP_TIER3 = 1, SP_TIER3_KEYED = 2, SP_TIER1 = 3, SP_TIER1_KEYED = 4 };

// largest n an engine takes: the generic engine's path pool after its three scratch retries, a tier's reverse cache
uint32_t sp_capacity(int engine)
{
	if ( engine == SP_GENERIC ) { ArenaCaps c; std::memset(&c,0,sizeof(c)); c.poolcap = 8192; for ( int i = 0; i < 3; ++i ) growArenaCaps(c); return c.poolcap; }
	if ( engine == SP_TIER3 || engine == SP_TIER3_KEYED ) return FastTier<3>::rccap;
	if ( engine == SP_TIER1 || engine == SP_TIER1_KEYED ) return FastTier<1>::rccap;
	return 0;
}

// perm: the sorted order as indices into the input; flags: the engine's overflow flags (1024: refused); fallback: heapsort fallbacks taken (generic engine)
int sp_sort(int engine, uint32_t const * front, uint16_t const * baselen, uint32_t n, int32_t * perm, uint32_t * flags, int32_t * fallback)
{
	*flags = 0; *fallback = 0;
	if ( engine == SP_GENERIC )
	{
		if ( n > sp_capacity(SP_GENERIC) ) return 2;
		std::vector<uint32_t> fr(front,front+n); std::vector<uint16_t> bl(baselen,baselen+n);
		static WindowEngine E; std::memset(&E,0,sizeof(E));
		E.A.rp_front = fr.data(); E.A.rp_baselen = bl.data();
		for ( uint32_t i = 0; i < n; ++i ) perm[i] = i;
		sortprobe_fallbacks = 0;
		E.arpSort(perm,perm+n);
		*flags = E.flags; *fallback = sortprobe_fallbacks;
		return 0;
	}
	if ( engine == SP_TIER3 || engine == SP_TIER3_KEYED ) return tierSort< FastTier<3> >(engine == SP_TIER3_KEYED,front,baselen,n,perm,flags);
	if ( engine == SP_TIER1 || engine == SP_TIER1_KEYED ) return tierSort< FastTier<1> >(engine == SP_TIER1_KEYED,front,baselen,n,perm,flags);
	return 1;
}

// std::sort over an array of structs with the engines' comparator
int sp_expected(uint32_t const * front, uint16_t const * baselen, uint32_t n, int32_t * perm)
{
	std::vector<Key> K(n);
	for ( uint32_t i = 0; i < n; ++i ) { K[i].front = front[i]; K[i].baselen = baselen[i]; K[i].idx = i; }
	std::sort(K.begin(),K.end(),KeyLess());
	for ( uint32_t i = 0; i < n; ++i ) perm[i] = K[i].idx;
	return 0;
}

// McIlroy's adversary ("A killer adversary for quicksort", 1999) against this library's std::sort: rank[i] of input position i, a permutation of
// 0 .. n-1 on which std::sort's median-of-3 keeps choosing a pivot next to the low end (mirror = 0) or the high end (mirror = 1) of its range.
// copies > 1: the adversary answers with tied keys, `copies` consecutive ranks counting as equal (rank[i] / copies is the key it played with,
// so sorting those keys replays its game comparison by comparison)
int sp_killer(uint32_t n, int mirror, uint32_t copies, uint32_t * rank)
{
	if ( !copies ) return 1;
	std::vector<int64_t> val(n); int64_t const gas = mirror ? -1 : static_cast<int64_t>(n);
	int64_t nsolid = 0; int64_t candidate = 0;
	for ( uint32_t i = 0; i < n; ++i ) val[i] = gas;
	std::vector<uint32_t> ptr(n); for ( uint32_t i = 0; i < n; ++i ) ptr[i] = i;
	auto const freeze = [&](uint32_t x) { val[x] = mirror ? static_cast<int64_t>(n)-1-nsolid : nsolid; ++nsolid; };
	auto const cmp = [&](uint32_t x, uint32_t y) -> bool
	{
		if ( val[x] == gas && val[y] == gas ) { if ( static_cast<int64_t>(x) == candidate ) freeze(x); else freeze(y); }
		if ( val[x] == gas ) candidate = x; else if ( val[y] == gas ) candidate = y;
		return (val[x] == gas || val[y] == gas) ? val[x] < val[y] : val[x]/copies < val[y]/copies;
	};
	std::sort(ptr.begin(),ptr.end(),cmp);
	for ( uint32_t i = 0; i < n; ++i ) { if ( val[i] == gas ) freeze(i); rank[i] = static_cast<uint32_t>(val[i]); }
	return 0;
}

}

#if defined(SORTPROBE_MAIN)
// stand-alone run (for a build with -fsanitize=address,undefined): killers, sorted, reversed, equal and random keys through every engine
static uint64_t rng_s = 88172645463325252ull;
static uint32_t rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return static_cast<uint32_t>(rng_s >> 16); }
int main()
{
	uint32_t const sizes[] = { 0, 1, 2, 16, 17, 32, 33, 64, 100, 144, 1000, 2048, 4096, sp_capacity(SP_GENERIC) };
	uint64_t runs = 0, fallbacks = 0, refused = 0, bad = 0;
	for ( uint32_t const n : sizes )
		for ( int kind = 0; kind < 6; ++kind )
		{
			std::vector<uint32_t> fr(n+1), rank(n+1); std::vector<uint16_t> bl(n+1);
			uint32_t const D = std::min<uint32_t>(256,std::max<uint32_t>(4,n/2)), copies = std::max<uint32_t>(1,n/D);
			if ( kind < 2 ) sp_killer(n,kind,copies,rank.data());
			for ( uint32_t i = 0; i < n; ++i )
			{
				uint64_t const q = kind < 2 ? rank[i]/copies : kind == 2 ? static_cast<uint64_t>(i)*D/n : kind == 3 ? static_cast<uint64_t>(n-1-i)*D/n : kind == 4 ? 0 : rnd() % D;
				fr[i] = 1000 + q/16; bl[i] = 12 + q%16;
			}
			std::vector<int32_t> want(n+1), got(n+1);
			sp_expected(fr.data(),bl.data(),n,want.data());
			for ( int engine = 0; engine < 5; ++engine )
			{
				if ( n > sp_capacity(engine) ) continue;
				uint32_t flags = 0; int32_t fb = 0;
				int const rc = sp_sort(engine,fr.data(),bl.data(),n,got.data(),&flags,&fb);
				++runs; fallbacks += fb; refused += (flags & 1024) ? 1 : 0;
				if ( rc || (flags & ~1024u) || (!(flags & 1024) && !std::equal(got.begin(),got.begin()+n,want.begin())) ) { ++bad; std::printf("BAD n=%u kind=%d engine=%d rc=%d flags=0x%x\n",n,kind,engine,rc,flags); }
			}
		}
	std::printf("sortprobe: %llu runs, %llu heapsort fallbacks, %llu refusals with flag 1024, %llu bad\n",(unsigned long long)runs,(unsigned long long)fallbacks,(unsigned long long)refused,(unsigned long long)bad);
	return bad ? 1 : 0;
}
#endif
