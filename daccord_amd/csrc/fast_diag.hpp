/*
 * Design, test and audit aids of the window fast path (fast_window.hpp).  They exist in the emulation build only (DACC_EMUL: the statistics,
 * traces and counters that DACC_EMUL_STATS / _TRAV / _FEAS / _FEASCASES / _FEASNEED write); a device build gets the same macros, empty.
 * The macros expand inside FastEngine and name its members (feascount, over, lane, L, ...), so this header is included in front of the engine.
 */
#ifndef DACC_FAST_DIAG_HPP
#define DACC_FAST_DIAG_HPP
#if defined(DACC_EMUL)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#endif

namespace dacc {

#if defined(DACC_EMUL)
// emulation only: per-window maxima of the variable-size structures (design aid, DACC_EMUL_STATS=<file>)
struct FastStats { enum { N = 33 }; uint32_t v[N]; void clear() { for ( int i = 0; i < N; ++i ) v[i] = 0; } void mx(int i, uint32_t x) { if ( x > v[i] ) v[i] = x; } void add(int i, uint32_t x) { v[i] += x; } };
static FastStats g_fstats;
static inline void fstats_dump(int const tier)
{
	static FILE * sf = 0; static bool tried = false;
	if ( !tried ) { tried = true; char const * fn = getenv("DACC_EMUL_STATS"); if ( fn ) sf = fopen(fn,"w"); }
	if ( sf ) { fprintf(sf,"%d",tier); for ( int i = 0; i < FastStats::N; ++i ) fprintf(sf," %u",g_fstats.v[i]); fprintf(sf,"\n"); fflush(sf); }
}
static inline FILE * ftrav_file() { static FILE * f = 0; static bool tried = false; if ( !tried ) { tried = true; char const * fn = getenv("DACC_EMUL_TRAV"); if ( fn ) f = fopen(fn,"w"); } return f; }
#define FSTAT_MX(i,x) g_fstats.mx(i,x)
#define FSTAT_ADD(i,x) g_fstats.add(i,x)
// design aid (DACC_EMUL_FEAS=<file>): per traversal the feasibility tasks' iteration counts, grouped as the 64 lanes would run them
struct FeasIters { std::vector<uint32_t> it, ln; void clear() { it.clear(); ln.clear(); } };
static FeasIters g_feasit;
static inline void feasit_dump()
{
	static FILE * f = 0; static bool tried = false;
	if ( !tried ) { tried = true; char const * fn = getenv("DACC_EMUL_FEAS"); if ( fn ) f = fopen(fn,"w"); }
	if ( !f ) { g_feasit.clear(); return; }
	std::vector<uint32_t> const & it = g_feasit.it; std::vector<uint32_t> const & ln = g_feasit.ln;
	uint64_t tot = 0, lock = 0, locksorted = 0;
	for ( size_t i = 0; i < it.size(); ++i ) tot += it[i];
	for ( size_t i = 0; i < it.size(); i += 64 ) { uint32_t m = 0; for ( size_t q = i; q < it.size() && q < i+64; ++q ) m = std::max(m,it[q]); lock += m; }
	std::vector< std::pair<uint32_t,uint32_t> > P; for ( size_t i = 0; i < it.size(); ++i ) P.push_back(std::make_pair(ln[i],it[i]));
	std::stable_sort(P.begin(),P.end(),[](std::pair<uint32_t,uint32_t> const & a, std::pair<uint32_t,uint32_t> const & b){ return a.first > b.first; });
	for ( size_t i = 0; i < P.size(); i += 64 ) { uint32_t m = 0; for ( size_t q = i; q < P.size() && q < i+64; ++q ) m = std::max(m,P[q].second); locksorted += m; }
	uint64_t lockcls = 0;
	{
		std::vector< std::pair<uint32_t,uint32_t> > Q; for ( size_t i = 0; i < it.size(); ++i ) { uint32_t c = 0; while ( (2u<<c) <= ln[i] ) ++c; Q.push_back(std::make_pair(c,it[i])); }
		std::stable_sort(Q.begin(),Q.end(),[](std::pair<uint32_t,uint32_t> const & a, std::pair<uint32_t,uint32_t> const & b){ return a.first > b.first; });
		for ( size_t i = 0; i < Q.size(); i += 64 ) { uint32_t m = 0; for ( size_t q = i; q < Q.size() && q < i+64; ++q ) m = std::max(m,Q[q].second); lockcls += m; }
	}
	fprintf(f,"%zu %llu %llu %llu %llu\n",it.size(),(unsigned long long)tot,(unsigned long long)lock,(unsigned long long)locksorted,(unsigned long long)lockcls);
	g_feasit.clear();
}
static inline bool feasit_on() { static int on = -1; if ( on < 0 ) on = getenv("DACC_EMUL_FEAS") ? 1 : 0; return on == 1; }      // single threaded design aid only
#define FEAS_ITERS(t,len,n) { if ( feasit_on() && !feascount ) { g_feasit.it.push_back(n); g_feasit.ln.push_back(len); } }
#define FEAS_DUMP() { if ( feasit_on() && !feascount ) feasit_dump(); }
// test aid (DACC_EMUL_FEASCASES=<file>): per traversal of computeStretchFeasLanes one line of counters that say which situations of the unit
// order, of the task rounds (as 64 lanes would run them, whatever the emulation's width) and of the node pipeline it went through
// (tests/test_feas_pipeline.py asserts that its cases reach each of them).  One window at a time: the emulation of one context is sequential.
struct FeasCases
{
	enum { NU = 0, NCU, NTASK, EMPTY_FIRST, EMPTY_MID, EMPTY_LAST, START_AT_ROUND, START_AT_ROUND_END, SPANS_ROUNDS, ROUNDS, LENMASK, MAXLEN, AT_CLAMP, PAST_CLAMP, MULTI, FAIL0, FAIL1, FAILLAST, NODES, N };
	uint64_t v[N];
	void clear() { for ( int i = 0; i < N; ++i ) v[i] = 0; }
	// widths of the units in processing order, before they become offsets
	template<typename PT> void units(PT W, uint32_t const nu)
	{
		clear();
		v[NU] = nu;
		uint32_t first = nu, last = 0;
		for ( uint32_t q = 0; q < nu; ++q ) if ( W[q] ) { if ( first == nu ) first = q; last = q; }
		uint64_t t = 0;
		for ( uint32_t q = 0; q < nu; ++q )
		{
			uint32_t const w = W[q];
			if ( !w ) { if ( q < first ) ++v[EMPTY_FIRST]; else if ( q > last ) ++v[EMPTY_LAST]; else ++v[EMPTY_MID]; continue; }
			++v[NCU];
			if ( t && t % 64 == 0 ) ++v[START_AT_ROUND];
			if ( t % 64 == 63 ) ++v[START_AT_ROUND_END];
			if ( t/64 != (t+w-1)/64 ) ++v[SPANS_ROUNDS];
			t += w;
		}
		v[NTASK] = t; v[ROUNDS] = (t+63)/64;
	}
	void node(uint32_t const j, uint32_t const len, uint32_t const pp, uint32_t const nrows, uint32_t const f)
	{
		++v[NODES];
		if ( j == 0 ) { v[LENMASK] |= 1ull << (len < 63 ? len : 63); if ( len > v[MAXLEN] ) v[MAXLEN] = len; }
		if ( pp+1 == nrows ) ++v[AT_CLAMP];          // the table word fetched for the node behind this one is the clamp row's
		if ( pp >= nrows ) ++v[PAST_CLAMP];         // a node's own position on or behind the clamp row
		if ( f > 1 ) ++v[MULTI];
	}
	void fail(uint32_t const j, uint32_t const len) { if ( j == 0 ) ++v[FAIL0]; if ( j == 1 ) ++v[FAIL1]; if ( j+1 == len && len > 2 ) ++v[FAILLAST]; }
	void dump(int const tier, uint32_t const nwF, uint32_t const nwR)
	{
		static FILE * f = 0; static bool tried = false;
		if ( !tried ) { tried = true; char const * fn = getenv("DACC_EMUL_FEASCASES"); if ( fn ) f = fopen(fn,"w"); }
		if ( !f ) return;
		fprintf(f,"%d",tier); for ( int i = 0; i < N; ++i ) fprintf(f," %llu",(unsigned long long)v[i]); fprintf(f," %u %u\n",nwF,nwR); fflush(f);
	}
};
static FeasCases g_feascases;
#define FEAS_UNITS(W,nu) { if ( lane == 0 && !feascount ) g_feascases.units(W,nu); }
#define FEAS_NODE(j,len,pp,nrows,f) { if ( !feascount ) g_feascases.node(j,len,pp,nrows,f); }
#define FEAS_FAIL(j,len) { if ( !feascount ) g_feascases.fail(j,len); }
#define FEAS_CASES_DUMP() { if ( lane == 0 && !feascount ) g_feascases.dump(int(CT::maxs),nwF,nwR); }
// audit aid (DACC_EMUL_FEASNEED=<file>): which (stretch, direction, position) triples the filter of computeStretchFeasLanes left out of a
// traversal, and how often the enumerations asked for one of them -- sfFind / csfFind at a left-out position, linkOk on a left-out reverse
// unit.  The filter is exact iff that never happens (tests/test_feas_need.py asserts zero).  The file holds one line of running totals,
// rewritten at every traversal and when the process ends: traversals, units with tasks and tasks without the filter, the same with it,
// weight records written (forward, reverse), probes of left-out forward positions, of left-out reverse positions, links on left-out
// reverse units; then the situations the traversals went through: first and last k-mer candidates strictly inside a stretch, middle
// pieces, traversals with (lmax+1)/2 <= k, passes of the distance relaxation.  One window at a time, like the other aids.
struct FeasNeedAudit
{
	enum { SCAP = 65536 };
	uint64_t outF[SCAP][3], outR[SCAP][3];      // left-out start positions of stretch s, forward and reverse (192 bits each: the table of w = 128 has row 128)
	uint64_t ntrav, units0, tasks0, units1, tasks1, recF, recR, probeF, probeR, linkR, insF, insL, mids, hlek, passes;
	FILE * f; bool tried;
	bool on() { if ( !tried ) { tried = true; char const * fn = getenv("DACC_EMUL_FEASNEED"); if ( fn ) f = fopen(fn,"w"); } return f != 0; }
	static void range(uint64_t * m, uint32_t const lo, uint32_t const hi) { for ( uint32_t p = lo; p < hi && p < 192u; ++p ) m[p>>6] |= 1ull << (p&63u); }
	// unit (s,rev): start positions [lo0,hi0) without the filter, [lo1,hi1) with it
	void unit(uint32_t const s, bool const rev, uint32_t const lo0, uint32_t const hi0, uint32_t const lo1, uint32_t const hi1)
	{
		if ( !on() || s >= SCAP ) return;
		uint64_t * const m = rev ? outR[s] : outF[s];
		m[0] = m[1] = m[2] = 0; range(m,lo0,hi0);
		uint64_t k[3] = {0,0,0}; range(k,lo1,hi1); m[0] &= ~k[0]; m[1] &= ~k[1]; m[2] &= ~k[2];
		if ( hi0 > lo0 ) { ++units0; tasks0 += hi0-lo0; }
		if ( hi1 > lo1 ) { ++units1; tasks1 += hi1-lo1; }
	}
	static bool out(uint64_t const * m, uint32_t const p) { return p < 192u && ((m[p>>6] >> (p&63u)) & 1ull); }
	void probe(uint32_t const s, bool const rev, uint32_t const p) { if ( f && s < SCAP && out(rev ? outR[s] : outF[s],p) ) ++(rev ? probeR : probeF); }
	void link(uint32_t const a, uint32_t const b) { if ( f && a < SCAP && b < SCAP && ((outR[a][0]|outR[a][1]|outR[a][2]) || (outR[b][0]|outR[b][1]|outR[b][2])) ) ++linkR; }
	void dump()
	{
		if ( !f ) return;
		rewind(f);
		fprintf(f,"%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n",(unsigned long long)ntrav,(unsigned long long)units0,(unsigned long long)tasks0,(unsigned long long)units1,(unsigned long long)tasks1,
			(unsigned long long)recF,(unsigned long long)recR,(unsigned long long)probeF,(unsigned long long)probeR,(unsigned long long)linkR,
			(unsigned long long)insF,(unsigned long long)insL,(unsigned long long)mids,(unsigned long long)hlek,(unsigned long long)passes);
		fflush(f);
	}
	~FeasNeedAudit() { dump(); }
};
static FeasNeedAudit g_feasneed;
#define FEAS_NEED_UNIT(s,rev,lo0,hi0,lo1,hi1) { if ( !feascount ) g_feasneed.unit(s,rev,lo0,hi0,lo1,hi1); }
#define FEAS_NEED_PROBE(s,rev,p) g_feasneed.probe(s,rev,p);
#define FEAS_NEED_LINK(a,b) g_feasneed.link(a,b);
#define FEAS_OVER() { if ( !feascount ) over(128); }
#define FEAS_NEED_PASS() { if ( lane == 0 ) ++g_feasneed.passes; }
#define FEAS_NEED_DUMP() { if ( lane == 0 && !feascount && g_feasneed.on() ) { FeasNeedAudit & A_ = g_feasneed; ++A_.ntrav; A_.recF += nwF; A_.recR += nwR; A_.mids += nmid; A_.hlek += (H <= static_cast<int64_t>(k)); \
	for ( uint32_t c_ = 0; c_ < nF; ++c_ ) A_.insF += (L.fnode()[c_] != 0xFFFF && L.parF()[c_] != SNONE); for ( uint32_t c_ = 0; c_ < nL; ++c_ ) A_.insL += (L.lnode()[c_] != 0xFFFF && L.parL()[c_] != SNONE); A_.dump(); } }
#else
#define FEAS_ITERS(t,len,n)
#define FEAS_DUMP()
#define FEAS_UNITS(W,nu)
#define FEAS_NODE(j,len,pp,nrows,f)
#define FEAS_FAIL(j,len)
#define FEAS_CASES_DUMP()
#define FEAS_NEED_UNIT(s,rev,lo0,hi0,lo1,hi1)
#define FEAS_NEED_PROBE(s,rev,p)
#define FEAS_NEED_LINK(a,b)
#define FEAS_NEED_DUMP()
#define FEAS_NEED_PASS()
#define FEAS_OVER() over(128);
#define FSTAT_MX(i,x)
#define FSTAT_ADD(i,x)
#endif
}
#endif
