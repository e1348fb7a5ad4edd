// The per-base difference strings of an alignment record -- write_cs_core / write_MD_core / write_cs_or_MD (LR/format.c:150-268) -- as
// one wavefront computes them: the per-lane statements, written once for the device kernel (map_diffstr.hip.h) and for the host
// emulator that drives them on 64 emulated lanes (tests/emul/diffstr_emul.cpp).
// What is wave-wide comes in through a small interface W:
//     unsigned lane;                      this lane, 0..63
//     uint64_t ballot(bool p);            bit l = p of lane l
//     unsigned prefix(uint64_t m);        set bits of m below this lane
//     uint32_t uni(uint32_t v);           v of the first lane (the value is wave-uniform; on the device this names it scalar)
//     void put(char *out, uint32_t at, char c);  out[at] = c (out: wave-uniform, at: this lane's 32-bit offset)
// Everything about the record as a whole -- the CIGAR operation, the offsets into both sequences, the output position, the carried
// run of identical bases -- is wave-uniform: it follows from the record, the CIGAR and the ballots alone.  The loop structure depends
// on the CIGAR only, never on a ballot.  With out == nullptr nothing is stored and the function returns the length (the count pass).
// An M operation goes 64 bases per round: one compare and one ballot; what a mismatch lane prints, and where, follows from the mask
// and the carried run (distance to the previous set bit, its decimal digit count, the bytes of the items before it as population
// counts of masks derived from the ballot).  No lane ever walks the bases of a record.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GDD_HD __host__ __device__ __forceinline__
#else
#define GDD_HD static inline
#endif

enum { GDD_MD = 0, GDD_CS = 1, GDD_CS_LONG = 2 };

struct GddRec { // one alignment record (mm_reg1_t reduced to what the strings read) and where its CIGAR words are
	int32_t read, qs, qe, rs, re, rid, rev;
	uint32_t n_cigar;
	int64_t cig_off;
};

struct GddIn {
	const GddRec *rec;
	const uint32_t *cig;     // BAM words, len << 4 | op
	const uint8_t *reads;    // nt4 codes 0..4, forward strand, all reads packed
	const int64_t *roff;     // read i = reads[roff[i] .. roff[i + 1])
	const uint32_t *S;       // mm_idx_t::S, 4-bit packed
	const uint64_t *seq_off; // contig offsets into S (in bases)
	const uint32_t *seq_len;
	int32_t qstrand;         // MM_F_QSTRAND: forward read against mm_idx_getseq2's reverse target (LR/format.c:245-248)
};

GDD_HD int gdd_popc(uint64_t m) { return __builtin_popcountll(m); }
GDD_HD int gdd_digits(uint32_t v)
{
	return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7 : v < 100000000 ? 8 : v < 1000000000 ? 9 : 10;
}
GDD_HD uint32_t gdd_digit(uint32_t v, int k) // the k-th decimal digit of v counted from the units
{
	uint32_t p = 1;
	for (int i = 0; i < k; ++i) p *= 10;
	return v / p % 10;
}
// "ACGTN"[c] / "acgtn"[c] for a code 0..4, without a table in memory
GDD_HD char gdd_up(uint32_t c) { return (char)(c < 4 ? 0x54474341u >> (c << 3) & 0xff : 'N'); }
GDD_HD char gdd_lo(uint32_t c) { return (char)(gdd_up(c) | 0x20); }
template <class W> GDD_HD uint64_t gdd_uni64(W &w, uint64_t v) { return (uint64_t)w.uni((uint32_t)v) | (uint64_t)w.uni((uint32_t)(v >> 32)) << 32; }

// the sequences as write_cs_or_MD lays them out (LR/format.c:245-259).  Everything here is wave-uniform; a base is named by a uniform
// 64-bit offset into the record's stretch plus this lane's small offset, so that what a lane computes stays 32 bits wide.
struct GddSeqs {
	const uint8_t *q;  // the read
	const uint32_t *S; // mm_idx_t::S
	int64_t q0;        // index (in q) of query base 0; a reverse-strand query is walked downwards from it
	int64_t t0;        // likewise for the target, in bases of S
	int32_t qrev, trev;
};
template <class W> GDD_HD GddSeqs gdd_seqs(W &w, const GddIn &in, const GddRec &r)
{
	GddSeqs s;
	const int64_t ro = (int64_t)gdd_uni64(w, (uint64_t)in.roff[r.read]);
	const int64_t so = (int64_t)gdd_uni64(w, in.seq_off[r.rid]);
	s.q = in.reads, s.S = in.S;
	s.qrev = r.rev && !in.qstrand, s.trev = r.rev && in.qstrand;
	s.q0 = s.qrev ? ro + r.qe - 1 : ro + r.qs;
	// mm_idx_getseq_rev of this tree (LR/index.c:168-181) takes st / en on the reverse strand: base j is the complement of contig base len - rs - 1 - j
	s.t0 = s.trev ? so + (int64_t)w.uni(in.seq_len[r.rid]) - r.rs - 1 : so + r.rs;
	return s;
}
// query base iu + l (iu: wave-uniform, l: this lane's)
GDD_HD uint32_t gdd_q(const GddSeqs &s, int64_t iu, uint32_t l)
{
	const uint8_t *p = s.q + (s.qrev ? s.q0 - iu : s.q0 + iu);
	uint32_t c = p[s.qrev ? -(int32_t)l : (int32_t)l];
	if (c > 4) c = 4;
	return s.qrev ? (c >= 4 ? 4u : 3u - c) : c;
}
// target base ju + l: mm_seq4_get (LR/mmpriv.h:32) of base u +- l with u = t0 +- ju; v = (u & 7) +- l names the word (v >> 3, floor) next to
// u's and the nibble in it (v & 7)
GDD_HD uint32_t gdd_t(const GddSeqs &s, int64_t ju, uint32_t l)
{
	const int64_t u = s.trev ? s.t0 - ju : s.t0 + ju; // (>= 0: ju names a base of the record; signed, so that >> 3 is a floor and never wraps)
	const uint32_t *p = s.S + (u >> 3);
	const int32_t v = (int32_t)(u & 7) + (s.trev ? -(int32_t)l : (int32_t)l);
	uint32_t c = p[v >> 3] >> ((v & 7) << 2) & 0xf;
	if (c > 4) c = 4;
	return s.trev ? (c < 4 ? 3u - c : c) : c;
}

// "<v>" in decimal at out[at ..): the lanes below its digit count write one digit each; returns the digit count
template <class W> GDD_HD int gdd_put_num(W &w, char *out, int64_t at, uint32_t v)
{
	const int dg = gdd_digits(v);
	if (out && (int)w.lane < dg) w.put(out + at, w.lane, (char)('0' + gdd_digit(v, dg - 1 - (int)w.lane)));
	return dg;
}

// `len` bases of one sequence from `from` on, in upper or lower case, at out[at ..): 64 per round, one per lane
template <class W, bool TARGET, bool UPPER> GDD_HD void gdd_put_bases(W &w, char *out, int64_t at, const GddSeqs &s, int64_t from, uint32_t len)
{
	if (!out) return;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
	for (uint32_t base = 0; base < len; base += 64) {
		if (w.lane < len - base) {
			const uint32_t c = TARGET ? gdd_t(s, from + base, w.lane) : gdd_q(s, from + base, w.lane);
			w.put(out + at + base, w.lane, UPPER ? gdd_up(c) : gdd_lo(c));
		}
	}
}

// One record in mode MODE (a template argument: each mode's statements compile apart, which keeps the device kernel's register count
// down).  Returns the length of its string; out == nullptr: count only.
template <int MODE, class W> GDD_HD int64_t gdd_record(W &w, const GddIn &in, int64_t rec_idx, char *out)
{
	GddRec r;
	{
		const GddRec &g = in.rec[rec_idx];
		r.read = (int32_t)w.uni((uint32_t)g.read), r.qs = (int32_t)w.uni((uint32_t)g.qs), r.qe = (int32_t)w.uni((uint32_t)g.qe);
		r.rs = (int32_t)w.uni((uint32_t)g.rs), r.re = (int32_t)w.uni((uint32_t)g.re), r.rid = (int32_t)w.uni((uint32_t)g.rid);
		r.rev = (int32_t)w.uni((uint32_t)g.rev), r.n_cigar = w.uni(g.n_cigar);
		r.cig_off = (int64_t)gdd_uni64(w, (uint64_t)g.cig_off);
	}
	const GddSeqs s = gdd_seqs(w, in, r);
	const int mode = MODE;
	const uint64_t below = (1ull << w.lane) - 1;
	int64_t o = 0;         // bytes so far
	int64_t qo = 0, to = 0;
	uint32_t run = 0;      // MD: l_MD, carried over the whole record; cs: the identity run of the current M operation
	for (uint32_t k = 0; k < r.n_cigar; ++k) {
		const uint32_t c = w.uni(in.cig[r.cig_off + k]), op = c & 0xf, len = c >> 4;
		if (op == 0 || op == 7 || op == 8) {
			if (mode != GDD_MD) run = 0;
#if defined(__HIPCC__)
#pragma unroll 1 // (not unrolled: the device kernel must stay within 32 VGPRs, map_diffstr.hip.h)
#endif
			for (uint32_t base = 0; base < len; base += 64) {
				const uint32_t nv = len - base < 64 ? len - base : 64;
				uint32_t qb = 0, tb = 0;
				if (w.lane < nv) qb = gdd_q(s, qo + base, w.lane), tb = gdd_t(s, to + base, w.lane);
				const uint64_t m = w.ballot(w.lane < nv && qb != tb);
				const uint64_t valid = nv == 64 ? ~0ull : (1ull << nv) - 1;
				const bool mine = m >> w.lane & 1;
				char *const po = out ? out + o : nullptr; // (wave-uniform; what a lane adds is a 32-bit offset)
				if (mode == GDD_CS_LONG) {
					// every lane writes: a matching base (behind '=' where a run starts), or "*tq"
					const uint64_t e = ~m & valid;
					uint64_t starts = e & ~(e << 1);
					if (run) starts &= ~1ull; // the run goes on from the round before
					if (out && w.lane < nv) {
						const uint32_t at = w.prefix(e) + 3 * w.prefix(m) + w.prefix(starts);
						if (mine) w.put(po, at, '*'), w.put(po, at + 1, gdd_lo(tb)), w.put(po, at + 2, gdd_lo(qb));
						else if (starts >> w.lane & 1) w.put(po, at, '='), w.put(po, at + 1, gdd_up(qb));
						else w.put(po, at, gdd_up(qb));
					}
					o += gdd_popc(e) + 3 * gdd_popc(m) + gdd_popc(starts);
					run = m >> (nv - 1) & 1 ? 0 : 1; // (only "in a run or not" matters here)
				} else if (m) {
					// the first mismatch of the round closes the carried run, every other one the gap to the set bit before it (< 64: one
					// or two digits); g1 / g10: the mismatches behind the first whose gap is at least 1 / at least 10
					const int first = __builtin_ctzll(m);
					const uint64_t mf = m & (m - 1);
					uint64_t sm = m << 1;
					const uint64_t g1 = mf & ~sm;
					sm |= sm << 1, sm |= sm << 2, sm |= sm << 4, sm |= sm << 2; // set bits of m moved up by 1 .. 10
					const uint64_t g10 = mf & ~sm;
					const uint32_t d0 = run + (uint32_t)first;
					const int dg0 = gdd_digits(d0);
					const uint64_t mb = m & below;
					const uint32_t d = mb ? w.lane - 1 - (63 - __builtin_clzll(mb)) : d0; // this lane's, if it holds a mismatch
					if (mode == GDD_MD) { // "<run><T>", the run printed even when it is 0
						gdd_put_num(w, out, o, d0);
						if (out && mine) {
							if (!mb) w.put(po, (uint32_t)dg0, gdd_up(tb));
							else {
								uint32_t at = (uint32_t)dg0 + 1 + 2 * (w.prefix(m) - 1) + w.prefix(g10);
								if (d >= 10) w.put(po, at++, (char)('0' + d / 10));
								w.put(po, at, (char)('0' + d % 10)), w.put(po, at + 1, gdd_up(tb));
							}
						}
						o += dg0 + 1 + 2 * (gdd_popc(m) - 1) + gdd_popc(g10);
					} else { // cs: [":<run>"] "*<t><q>", the run only when it is > 0
						const int s0 = d0 ? 1 + dg0 : 0;
						if (d0) {
							if (out && w.lane == 0) w.put(out + o, 0, ':');
							gdd_put_num(w, out, o + 1, d0);
						}
						if (out && mine) {
							uint32_t at = (uint32_t)s0;
							if (mb) {
								at += 3 * w.prefix(m) + 2 * w.prefix(g1) + w.prefix(g10);
								if (d) w.put(po, at++, ':');
								if (d >= 10) w.put(po, at++, (char)('0' + d / 10));
								if (d) w.put(po, at++, (char)('0' + d % 10));
							}
							w.put(po, at, '*'), w.put(po, at + 1, gdd_lo(tb)), w.put(po, at + 2, gdd_lo(qb));
						}
						o += s0 + 3 * gdd_popc(m) + 2 * gdd_popc(g1) + gdd_popc(g10);
					}
					run = nv - 1 - (63 - (uint32_t)__builtin_clzll(m));
				} else run += nv;
			}
			if (mode == GDD_CS && run) { // the identity run is flushed at the end of every M operation (LR/format.c:174-180)
				if (out && w.lane == 0) w.put(out + o, 0, ':');
				o += 1 + gdd_put_num(w, out, o + 1, run);
			}
			qo += len, to += len;
		} else if (op == 1) {
			if (mode != GDD_MD) {
				if (out && w.lane == 0) w.put(out + o, 0, '+');
				gdd_put_bases<W, false, false>(w, out, o + 1, s, qo, len);
				o += 1 + (int64_t)len;
			}
			qo += len;
		} else if (op == 2) {
			if (mode == GDD_MD) { // "<run>^<bases>", the run printed even when it is 0
				const int dg = gdd_put_num(w, out, o, run);
				if (out && w.lane == 0) w.put(out + o + dg, 0, '^');
				gdd_put_bases<W, true, true>(w, out, o + dg + 1, s, to, len);
				o += dg + 1 + (int64_t)len, run = 0;
			} else {
				if (out && w.lane == 0) w.put(out + o, 0, '-');
				gdd_put_bases<W, true, false>(w, out, o + 1, s, to, len);
				o += 1 + (int64_t)len;
			}
			to += len;
		} else { // N: "~<t0><t1><len><t[len-2]><t[len-1]>" in cs, nothing in MD (the host has checked len >= 2)
			if (mode != GDD_MD) {
				const int dg = gdd_put_num(w, out, o + 3, len);
				if (out && w.lane == 0) w.put(out + o, 0, '~');
				// the first two and the last two bases, each pair from a uniform offset inside the record (never one in front of it: an N may
				// be the record's first operation, at base 0 of S)
				gdd_put_bases<W, true, false>(w, out, o + 1, s, to, 2);
				gdd_put_bases<W, true, false>(w, out, o + 3 + dg, s, to + len - 2, 2);
				o += 5 + dg;
			}
			to += len;
		}
	}
	if (mode == GDD_MD && run) o += gdd_put_num(w, out, o, run);
	return o;
}

// what the host checks before anything is launched (the reference's assertions LR/format.c:156,199,232 turned into an error; it is
// also what keeps every read of the kernel in bounds).  The caller has checked r.read and r.rid; 0 = fine, else which condition failed
GDD_HD int gdd_check_record(const GddRec &r, const uint32_t *cig, int64_t read_len, uint32_t contig_len, int cs)
{
	if (r.qs < 0 || r.qe < r.qs || r.qe > read_len) return 2;
	if (r.rs < 0 || r.re < r.rs || (uint32_t)r.re > contig_len) return 3;
	int64_t q = 0, t = 0;
	for (uint32_t k = 0; k < r.n_cigar; ++k) {
		const uint32_t op = cig[k] & 0xf, len = cig[k] >> 4;
		if (op == 0 || op == 7 || op == 8) q += len, t += len;
		else if (op == 1) q += len;
		else if (op == 2) t += len;
		else if (op == 3) { if (cs && len < 2) return 5; t += len; }
		else return 4;
	}
	if (q != r.qe - r.qs || t != r.re - r.rs) return 6;
	return 0;
}
