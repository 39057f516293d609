/*
 * Consensus -> A window alignment of the LDS / device-memory tiers (H6, HandleContext.hpp:2429-2493), one LANE per window.
 *
 * A tier that has found the consensus of a narrow window (w <= 64) leaves a PENDING record in the window's slot of wrec
 * (dev_types.hpp: WREC_PENDING) instead of aligning on lane 0 while 63 lanes idle.  emitPendingRecord turns one pending record
 * into the final one, in place: global alignment of the A window (pattern, m = w rows, one 64 bit word) against the consensus
 * (text, n <= MAXCONS columns) with Myers' bit-vector recurrence, D[i][0] = i, D[0][j] = j, then the traceback with the
 * product's priority -- diagonal, then the step that consumes an A symbol (DEL), then the insertion (INS) -- and the record
 * of the generic engine's alignAndEmit (dbg_window.hpp): rec[0] = 1, off[r] at rec[1+r] (r = 0 .. m+1), symbols behind them.
 * Bytes behind the last symbol are unspecified.
 *
 * The same function runs in k_emit (capi.hip: one lane per window of the batch), in the host emulation (lane 0, right behind
 * the pending store) and in tests/emit/emit_check.cpp (against an O(mn) matrix), so it uses nothing but plain C++.
 * Every input is read before the first store: the final record lies over the pending one.
 */
#ifndef DACC_EMIT_RECORD_HPP
#define DACC_EMIT_RECORD_HPP
#include <stdint.h>
#include "dev_types.hpp"

#if defined(__HIPCC__) && !defined(DACC_EMUL)
#define DACC_EMIT_FN __host__ __device__ inline
#else
#define DACC_EMIT_FN inline
#endif

namespace dacc {

// pattern mask of symbol ch out of the four of the A window
DACC_EMIT_FN uint64_t emitEq(uint32_t const ch, uint64_t const e0, uint64_t const e1, uint64_t const e2, uint64_t const e3)
{
	return (ch & 2) ? ((ch & 1) ? e3 : e2) : ((ch & 1) ? e1 : e0);
}
// eight symbols, one per byte -> 2 bits each in the low 16 bits
DACC_EMIT_FN uint64_t emitPack8(uint64_t p)
{
	p &= 0x0303030303030303ull;
	p = (p | (p>>6)) & 0x000F000F000F000Full;
	p = (p | (p>>12)) & 0x000000FF000000FFull;
	return (p | (p>>24)) & 0xFFFFull;
}

// rec: the window's record, 8 byte aligned, WREC bytes; m = w in 1 .. 64.  Does nothing unless rec[0] == WREC_PENDING.
DACC_EMIT_FN void emitPendingRecord(uint8_t * const rec, uint32_t const m)
{
	if ( rec[0] != WREC_PENDING ) return;
	uint64_t const * const R8 = reinterpret_cast<uint64_t const *>(rec);
	uint32_t n = rec[PEND_LEN]; if ( n > MAXCONS ) n = MAXCONS;
	uint64_t const e0 = R8[PEND_PEQ/8], e1 = R8[PEND_PEQ/8+1], e2 = R8[PEND_PEQ/8+2], e3 = R8[PEND_PEQ/8+3];
	static_assert(MAXCONS == 96 && (PEND_PEQ & 7) == 0 && (PEND_CONS & 7) == 0 && PEND_CONS + MAXCONS <= WREC,"consensus packed into three 64 bit words");
	uint64_t ck[3] = {0,0,0};      // consensus symbols 0-31, 32-63, 64-95 (symbols behind n: whatever the last word held, never used)
	for ( uint32_t q = 0; q < MAXCONS/8; ++q )
		if ( 8*q < n ) ck[q>>2] |= emitPack8(R8[PEND_CONS/8+q]) << (16*(q&3));
	uint64_t const ck0 = ck[0], ck1 = ck[1], ck2 = ck[2];
	#define DACC_EMIT_SYM(c_) (static_cast<uint32_t>(((c_) < 32 ? ck0 : ((c_) < 64 ? ck1 : ck2)) >> (2*((c_)&31))) & 3u)

	// forward pass: column c+1 = state behind consensus symbol c (vertical deltas Pv / Mv, bottom score)
	uint64_t pvc[MAXCONS+1], mvc[MAXCONS+1]; uint8_t botc[MAXCONS+1];
	uint64_t const mask = (m == 64) ? ~0ull : ((1ull<<m)-1);
	uint64_t const top = 1ull<<(m-1);
	uint64_t Pv = mask, Mv = 0; uint32_t score = m;
	pvc[0] = Pv; mvc[0] = Mv; botc[0] = static_cast<uint8_t>(m);
	for ( uint32_t c = 0; c < n; ++c )
	{
		uint64_t const Eq = emitEq(DACC_EMIT_SYM(c),e0,e1,e2,e3);
		uint64_t const Xv = Eq | Mv;
		uint64_t const Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
		uint64_t Ph = Mv | ~(Xh | Pv);
		uint64_t Mh = Pv & Xh;
		if ( Ph & top ) ++score; else if ( Mh & top ) --score;
		Ph = (Ph<<1) | 1ull; Mh <<= 1;
		Pv = (Mh | ~(Xv | Ph)) & mask;
		Mv = (Ph & Xv) & mask;
		pvc[c+1] = Pv; mvc[c+1] = Mv; botc[c+1] = static_cast<uint8_t>(score);
	}

	// traceback (last step first): 0 = match, 1 = mismatch, 2 = INS (consensus symbol only), 3 = DEL (A symbol only)
	uint8_t ops[64+MAXCONS];
	uint32_t i = m, j = n, d = score, nops = 0;
	// column j (its Pv) and column j-1 (Pv, Mv, bottom score) in registers
	uint64_t pvj = Pv, pv1 = 0, mv1 = 0; uint32_t bot1 = 0;
	if ( j ) { pv1 = pvc[j-1]; mv1 = mvc[j-1]; bot1 = botc[j-1]; }
	while ( i || j )
	{
		uint32_t op = 2; bool done = false, left = false;
		if ( i && j )
		{
			// D[i-1][j-1] from column j-1: bottom minus the vertical deltas of rows i .. m
			uint32_t const sh = i-1;
			uint32_t const dd = bot1 - static_cast<uint32_t>(__builtin_popcountll(pv1>>sh)) + static_cast<uint32_t>(__builtin_popcountll(mv1>>sh));
			uint32_t const neq = ((emitEq(DACC_EMIT_SYM(j-1),e0,e1,e2,e3) >> sh) & 1ull) ? 0u : 1u;      // A[i-1] != cons[j-1]
			if ( dd + neq == d ) { op = neq; --i; --j; d = dd; done = true; left = true; }
		}
		if ( !done && i )
		{
			if ( (pvj >> (i-1)) & 1ull ) { op = 3; --i; d = d-1; done = true; }      // D[i-1][j] = d - 1
		}
		if ( !done ) { op = 2; --j; d = d-1; left = true; }
		if ( left )
		{
			pvj = pv1;
			if ( j ) { pv1 = pvc[j-1]; mv1 = mvc[j-1]; bot1 = botc[j-1]; }
		}
		ops[nops++] = static_cast<uint8_t>(op);
	}

	// the record, put together in a buffer of the lane and stored in 8 byte words.  Group r (r = 0 .. m) = the consensus symbols
	// inserted in front of A position r, followed (r < m) by the symbol aligned to it ('D' = 4 for a deletion); off[r] = index of its
	// first symbol, off[m+1] = number of symbols = number of steps
	uint64_t outw[WREC/8];
	uint8_t * const out = reinterpret_cast<uint8_t *>(outw);
	uint8_t * const off = out+1; uint8_t * const sym = out + 1 + (m+2);
	out[0] = WREC_FINAL;
	uint32_t so = 0, cpos = 0, t = nops;
	for ( uint32_t r = 0; r <= m; ++r )
	{
		off[r] = static_cast<uint8_t>(so);
		while ( t && ops[t-1] == 2 ) { sym[so++] = static_cast<uint8_t>(DACC_EMIT_SYM(cpos)); ++cpos; --t; }
		if ( r < m )
		{
			uint32_t const op = ops[--t];
			if ( op == 3 ) sym[so++] = 4; else { sym[so++] = static_cast<uint8_t>(DACC_EMIT_SYM(cpos)); ++cpos; }
		}
	}
	off[m+1] = static_cast<uint8_t>(so);
	#undef DACC_EMIT_SYM
	uint32_t const nbytes = 1 + (m+2) + so;      // <= 1 + 66 + 64 + MAXCONS
	static_assert(1 + 66 + 64 + MAXCONS <= WREC,"a final record fits its slot");
	uint64_t * const W8 = reinterpret_cast<uint64_t *>(rec);
	for ( uint32_t q = 0; 8*q < nbytes; ++q ) W8[q] = outw[q];
}

}
#endif
