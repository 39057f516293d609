// TEST HARNESS ONLY (host code, built by tests/test_emit_record.py with -fsanitize=address,undefined): emitPendingRecord
// (daccord_amd/csrc/emit_record.hpp), the routine that turns a pending window record into the final one, against a plain O(mn)
// edit-distance matrix with D[i][0] = i, D[0][j] = j and the same traceback priority (diagonal, then the step that consumes an
// A symbol, then the insertion).  Compared: rec[0], off[0 .. m+1], sym[0 .. nops); the bytes behind are unspecified.
// Final (rec[0] = 1) and empty (rec[0] = 0) records must come back untouched.  Prints one line per m and "ok"; exit status 1 on a difference.
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <random>
#include "../../daccord_amd/csrc/emit_record.hpp"

using namespace dacc;

typedef std::vector<uint8_t> Str;

// the record slot as 64 bit words (emitPendingRecord wants it 8 byte aligned), with a guard slot of 0xA5 behind it
struct Slot
{
	std::vector<uint64_t> w;
	Slot() : w(2*WREC/8) { std::memset(w.data(),0xA5,2*WREC); }
	uint8_t * rec() { return reinterpret_cast<uint8_t *>(w.data()); }
	bool guardIntact() { for ( uint32_t i = WREC; i < 2*WREC; ++i ) if ( rec()[i] != 0xA5 ) return false; return true; }
};

static void makePending(uint8_t * rec, Str const & a, Str const & cons)
{
	uint64_t peq[4] = {0,0,0,0};
	for ( size_t i = 0; i < a.size(); ++i ) peq[a[i]] |= 1ull<<i;
	rec[0] = WREC_PENDING; rec[PEND_LEN] = static_cast<uint8_t>(cons.size());
	std::memcpy(rec+PEND_PEQ,peq,sizeof(peq));
	for ( size_t j = 0; j < cons.size(); ++j ) rec[PEND_CONS+j] = cons[j];
}

// expected rec[0], offsets and symbols from the full matrix
static void expected(Str const & a, Str const & cons, std::vector<uint8_t> & off, std::vector<uint8_t> & sym)
{
	size_t const m = a.size(), n = cons.size();
	std::vector< std::vector<uint32_t> > D(m+1,std::vector<uint32_t>(n+1,0));
	for ( size_t i = 0; i <= m; ++i ) D[i][0] = i;
	for ( size_t j = 0; j <= n; ++j ) D[0][j] = j;
	for ( size_t i = 1; i <= m; ++i )
		for ( size_t j = 1; j <= n; ++j )
		{
			uint32_t v = D[i-1][j-1] + (a[i-1] != cons[j-1]);
			if ( D[i-1][j]+1 < v ) v = D[i-1][j]+1;
			if ( D[i][j-1]+1 < v ) v = D[i][j-1]+1;
			D[i][j] = v;
		}
	std::vector<uint8_t> ops;      // last step first; 0 match, 1 mismatch, 2 insertion (consensus only), 3 deletion (A only)
	size_t i = m, j = n;
	while ( i || j )
	{
		if ( i && j && D[i-1][j-1] + (a[i-1] != cons[j-1]) == D[i][j] ) { ops.push_back(a[i-1] != cons[j-1]); --i; --j; }
		else if ( i && D[i-1][j]+1 == D[i][j] ) { ops.push_back(3); --i; }
		else { ops.push_back(2); --j; }
	}
	off.assign(m+2,0); sym.clear();
	size_t t = ops.size(), cpos = 0;
	for ( size_t r = 0; r <= m; ++r )
	{
		off[r] = static_cast<uint8_t>(sym.size());
		while ( t && ops[t-1] == 2 ) { sym.push_back(cons[cpos++]); --t; }
		if ( r < m ) { uint8_t const op = ops[--t]; sym.push_back(op == 3 ? 4 : cons[cpos++]); }
	}
	off[m+1] = static_cast<uint8_t>(sym.size());
}

static uint64_t ncases = 0;

static bool check(Str const & a, Str const & cons, char const * what)
{
	uint32_t const m = a.size();
	Slot S; makePending(S.rec(),a,cons);
	emitPendingRecord(S.rec(),m);
	std::vector<uint8_t> off, sym; expected(a,cons,off,sym);
	uint8_t const * rec = S.rec();
	bool ok = rec[0] == WREC_FINAL && S.guardIntact() && 1 + (m+2) + sym.size() <= WREC;
	ok = ok && std::memcmp(rec+1,off.data(),m+2) == 0 && std::memcmp(rec+1+(m+2),sym.data(),sym.size()) == 0;
	++ncases;
	if ( !ok ) std::fprintf(stderr,"MISMATCH %s: m %u n %zu\n",what,m,cons.size());
	// converting twice changes nothing: the record is final now
	std::vector<uint8_t> before(rec,rec+WREC);
	emitPendingRecord(S.rec(),m);
	if ( std::memcmp(before.data(),S.rec(),WREC) != 0 ) { std::fprintf(stderr,"a final record was changed (%s, m %u n %zu)\n",what,m,cons.size()); ok = false; }
	return ok;
}

int main()
{
	std::mt19937_64 rng(20240607);
	auto const rnd = [&](uint32_t const n, uint32_t const alpha) { Str s(n); for ( auto & c : s ) c = rng() % alpha; return s; };
	bool ok = true;
	uint32_t const ms[] = {1,2,24,40,63,64};
	for ( uint32_t const m : ms )
	{
		std::vector<uint32_t> ns = {0,1,96};
		for ( int d = -5; d <= 5; ++d ) if ( static_cast<int>(m)+d >= 0 && static_cast<int>(m)+d <= 96 ) ns.push_back(m+d);
		for ( uint32_t const n : ns )
		{
			for ( uint32_t rep = 0; rep < 24; ++rep )
			{
				// unrelated strings over 4, 2 and 1 symbols
				uint32_t const alpha = rep % 3 == 0 ? 4 : (rep % 3 == 1 ? 2 : 1);
				Str const a = rnd(m,alpha);
				ok = check(a,rnd(n,alpha),"random") && ok;
				// one symbol against another one
				if ( rep == 0 ) ok = check(Str(m,1),Str(n,2),"two symbols") && ok;
				// the consensus as a noisy copy of A (what the tiers produce), cut or padded to n
				Str c;
				for ( uint32_t i = 0; i < m; ++i )
				{
					uint32_t const r = rng() % 20;
					if ( r == 0 ) continue;                                   // deletion
					if ( r == 1 ) c.push_back(rng() % 4);                     // insertion
					c.push_back(r == 2 ? static_cast<uint8_t>((a[i]+1+rng()%3)&3) : a[i]);
				}
				while ( c.size() < n ) c.push_back(rng() % alpha);
				c.resize(n);
				ok = check(a,c,"noisy copy") && ok;
				if ( n == m ) ok = check(a,a,"equal") && ok;
			}
		}
		std::printf("m %u: %zu lengths\n",m,ns.size());
		// final and empty records stay as they are, whatever lies behind the status byte
		for ( uint8_t const st : {uint8_t(0),uint8_t(1),uint8_t(3),uint8_t(255)} )
			for ( uint32_t rep = 0; rep < 8; ++rep )
			{
				Slot S; for ( uint32_t i = 0; i < WREC; ++i ) S.rec()[i] = rng();
				if ( rep == 0 ) makePending(S.rec(),rnd(m,4),rnd(m,4));      // a pending record's body under another status
				S.rec()[0] = st;
				std::vector<uint8_t> before(S.rec(),S.rec()+WREC);
				emitPendingRecord(S.rec(),m);
				if ( std::memcmp(before.data(),S.rec(),WREC) != 0 || !S.guardIntact() ) { std::fprintf(stderr,"a record of status %u was changed (m %u)\n",st,m); ok = false; }
			}
	}
	std::printf("%llu pairs\n%s\n",static_cast<unsigned long long>(ncases),ok ? "ok" : "FAILED");
	return ok ? 0 : 1;
}
