// The reference FASTA as the device reads it: the per-lane statements of the three block passes and of the packing pass, written once
// for the kernels (ref_fasta.hip.h) and for the host emulator that runs them as loops (tests/emul/ref_fasta_emul.cpp); the sequential
// grammar as a byte-at-a-time machine (GdRefGrammar) for the blocks the device does not claim; and the loop over the blocks of a file
// (gd_ref_one_block) that both the driver (ref_fasta_driver.hip.h) and the emulator run.  No HIP in here.
//
// THE RESULT is defined by kseq_read (LR/kseq.h:191-232; read_record of fastx_reader.h) alone: the names and sequences it returns for
// the file, in file order.  The device claims a block only where its passes provably compute that.
//
// WHY A CLAIMED BLOCK IS kseq_read's.  The state at a byte is one of: LS, the sequence loop (kseq.h:207-212) is about to read the first
// byte of a line; HD, the parser is inside a header line (ks_getuntil for the name, :201, or for the rest of the line, :202); SQ, it is
// inside a line of the sequence (the ks_getuntil2 of :211).  A block is claimed when it holds no '\r', no line starts with '+' or '@',
// and -- for the first block of the file, where the parser still scans for ANY '>' or '@' (:195-199: not only one at a line start) --
// byte 0 is '>', so that this scan ends on the first byte it reads, as it would at a line start.  Then, by induction over the lines:
//   * LS: the loop reads the line's first byte c.  '\n': an empty line is skipped (:209), the next byte is again a line's first.  '>':
//     the loop ends, last_char = '>' (:213), the record is returned and the next call goes straight to the name (:200-201): a header line
//     starts.  '+' and '@' do not occur.  Anything else: c is kept (:210) and the rest of the line up to its '\n' is appended (:211):
//     every byte of the line but the '\n' is a base, spaces and other bytes included (they become code 4 in seq_nt4_table).  No '\r' is in
//     the line, so nothing is trimmed from its end (kseq.h:141).
//   * HD: the name ends at the first byte isspace() accepts; if that was not the '\n', the rest of the line is skipped (:202).  Either
//     way the header line ends at its first '\n', and the sequence loop starts on the next line: LS.
//   * SQ: bytes up to the '\n' are bases, then LS.
// So every line that starts with '>' is a header, every other line is sequence, and the bases are the bytes of the sequence lines
// without their '\n': what the passes below count and place.  A header without '\n' and a sequence line without '\n' end with the
// file, where ks_getuntil2 and the loop stop as they do at a '\n'.  A '>' that ends the file with nothing behind it is no record
// (:201 returns -1): GdRefGrammar::finish drops it for both routes.
// A block that is not claimed is not claimed to be wrong: it goes through GdRefGrammar, and so do the blocks behind it until that
// machine stands in one of the three states again (with no '\r' pending at the end of a line).
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "fastx_dev.h"

enum { GDR_LS = 0, GDR_HD = 1, GDR_SQ = 2 };

struct GdrHdr { uint32_t gt_off, nl_off, base_rank; }; // one header line that STARTS in the block: its '>', its '\n' (GDX_NONE: none in the block), bases of the block in front of it
struct GdrCnt { uint32_t bases, hstart, hend, pad; };   // per tile; summed over tiles
struct GdrMeta { uint32_t bad, run_nl; };               // bad != 0: not claimed; run_nl: the '\n' of the header running into the block (GDX_NONE: none)

struct GdrLane { uint32_t nl, start, hdr, bad; }; // 16-bit masks over the lane's bytes: '\n'; first byte of a line; ... which is '>'; disqualifying bytes

// prev_nl: the byte in front of the lane's first is a '\n' (or the block starts at a line start and this is its first lane)
GDX_HD GdrLane gdr_lane_masks(const uint32_t w[4], uint32_t valid, bool prev_nl)
{
	GdrLane L;
	const uint32_t vm = valid >= GDX_LANE_BYTES ? 0xffffu : (1u << valid) - 1u;
	L.nl = gdx_eq_mask16(w, '\n', valid);
	L.start = ((L.nl << 1) | (prev_nl ? 1u : 0u)) & vm;
	L.hdr = L.start & gdx_eq_mask16(w, '>', valid);
	L.bad = gdx_eq_mask16(w, '\r', valid) | (L.start & (gdx_eq_mask16(w, '+', valid) | gdx_eq_mask16(w, '@', valid)));
	return L;
}
// class of the last line that starts in the lane (0: none does)
GDX_HD uint32_t gdr_lane_code(const GdrLane &L)
{
	if (!L.start) return 0;
	const uint32_t t = 31u - (uint32_t)__builtin_clz(L.start);
	return (L.hdr >> t & 1u) ? (uint32_t)GDR_HD : (uint32_t)GDR_SQ;
}
// take-the-last over (lanes of a tile | tiles of a block): has / ishdr = one bit per lane, "a line starts here" / "the last one is a header"
GDX_HD uint32_t gdr_class_in(uint64_t has, uint64_t ishdr, uint32_t lane, uint32_t tile_in)
{
	const uint64_t m = lane ? has & (~0ull >> (64 - lane)) : 0;
	if (!m) return tile_in;
	const uint32_t t = 63u - (uint32_t)__builtin_clzll(m);
	return (ishdr >> t & 1u) ? (uint32_t)GDR_HD : (uint32_t)GDR_SQ;
}
// class of the last line that starts in the tile (0: none does)
GDX_HD uint32_t gdr_tile_code(uint64_t has, uint64_t ishdr)
{
	if (!has) return 0;
	const uint32_t t = 63u - (uint32_t)__builtin_clzll(has);
	return (ishdr >> t & 1u) ? (uint32_t)GDR_HD : (uint32_t)GDR_SQ;
}
GDX_HD uint32_t gdr_take_last(uint32_t a, uint32_t b) { return b ? b : a; }
// the lane's bytes by class, cls_in being the class of the line running into it: bases = bytes of sequence lines but their '\n'; hend =
// the '\n' of header lines
GDX_HD void gdr_lane_split(const GdrLane &L, uint32_t valid, uint32_t cls_in, uint32_t &bases, uint32_t &hend)
{
	uint32_t cls = cls_in, b = 0, e = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
	for (uint32_t j = 0; j < GDX_LANE_BYTES; ++j) {
		const uint32_t bit = 1u << j;
		if (L.start & bit) cls = (L.hdr & bit) ? (uint32_t)GDR_HD : (uint32_t)GDR_SQ;
		if (L.nl & bit) e |= cls == GDR_HD ? bit : 0u;
		else b |= cls == GDR_SQ ? bit : 0u;
	}
	bases = b & (valid >= GDX_LANE_BYTES ? 0xffffu : (1u << valid) - 1u); // (bytes behind the block's end are nobody's; nl and start are masked already)
	hend = e;
}
// whether the lane's first byte starts a line: the byte in front of it is a '\n', or it is byte 0 of a block that starts at a line start
GDX_HD bool gdr_prev_nl(const uint8_t *blk, uint32_t at, uint32_t n, int state_in) { return at == 0 ? state_in == GDR_LS : (at <= n && blk[at - 1] == '\n'); }
// The lane's stores of the write pass.  rb / rs / re: bases, header starts and header ends of the block in front of the lane.  Header end e
// closes header start e - hd_in (hd_in: the block starts inside a header line, whose end is end 0 and goes to meta).  nt4 has room for
// nt4_cap bases, rows for row_cap headers; every store is checked against them.
GDX_HD void gdr_lane_write(const GdrLane &L, uint32_t bases, uint32_t hend, const uint32_t w[4], uint32_t at, uint32_t rb, uint32_t rs, uint32_t re, uint32_t hd_in,
                           uint8_t *nt4, uint64_t base0, uint64_t nt4_cap, GdrHdr *rows, uint32_t row_cap, GdrMeta *meta)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
	for (uint32_t j = 0; j < GDX_LANE_BYTES; ++j) { // (all three masks are empty behind the block's last byte)
		const uint32_t bit = 1u << j;
		if (L.hdr & bit) {
			if (rs < row_cap) rows[rs].gt_off = at + j, rows[rs].base_rank = rb;
			++rs;
		}
		if (bases & bit) {
			if (base0 + rb < nt4_cap) nt4[base0 + rb] = (uint8_t)gdx_nt4(w[j >> 2] >> (8 * (j & 3)) & 0xffu);
			++rb;
		}
		if (hend & bit) {
			if (re < hd_in) meta->run_nl = at + j;
			else if (re - hd_in < row_cap) rows[re - hd_in].nl_off = at + j;
			++re;
		}
	}
}
// word i of S from the nt4 bytes of its eight bases (LR/mmpriv.h:31: base o in bits 4 (o & 7) ..): the inverse of idx_unpack_kernel;
// nibbles behind the last base are zero, as gd_index_pack_S leaves them
GDX_HD uint32_t gdr_pack_word(uint64_t bytes8, uint64_t i, uint64_t sum)
{
	uint32_t wd = 0;
	for (int b = 0; b < 8; ++b)
		if (8 * i + (uint64_t)b < sum) wd |= (uint32_t)((bytes8 >> (8 * b)) & 0xf) << (4 * b);
	return wd;
}

// ---- the sequential grammar, one byte at a time -------------------------------------------------------------------------------------
// kseq_read's record loop as a machine that can stop and go on at any byte, keeping names and base ranks only (a reference needs no
// quality and no comment).  Every statement names the line of read_record (fastx_reader.h) / ks_getuntil2 it stands for; the emulator
// checks the machine against read_record on every input of tests/ref_fasta_inputs.py.
struct GdRefGrammar {
	enum { PRE, NAME, COMMENT, LS, SQ, PLUS, QUAL };
	int st = PRE;                    // PRE: last_char == 0, scanning for any '>' or '@'
	std::vector<std::string> names;
	std::vector<uint64_t> start;     // base rank of every record's first base
	uint64_t rank = 0;               // bases so far
	uint64_t hdr_bytes = 0;          // bytes read behind the '>' / '@' of the current header
	uint64_t line_bytes = 0;         // SQ / QUAL: bytes ks_getuntil2 has read of the current line
	bool last_cr = false;            // the last byte appended to the sequence / quality string is '\r'
	uint64_t qual_len = 0;
	// bases the machine produced and nobody has stored yet: hb[i] is the base of rank hb_base + i
	std::vector<uint8_t> hb;
	uint64_t hb_base = 0;

	void push(uint32_t c)
	{
		if (hb.empty()) hb_base = rank;
		hb.push_back((uint8_t)gdx_nt4(c)), ++rank, last_cr = c == '\r';
	}
	void rewind(uint64_t to) // bases [to, rank) are taken back (a trimmed '\r'; a record that is dropped)
	{
		if (to >= hb_base && !hb.empty()) hb.resize((size_t)(to - hb_base));
		else hb.clear(), hb_base = to;
		rank = to;
	}
	void begin_record() { names.emplace_back(), start.push_back(rank), hdr_bytes = 0, st = NAME; }
	void drop_record() { rewind(start.back()), names.pop_back(), start.pop_back(); }
	// ks_getuntil2's trim at the end of a line (kseq.h:141): a '\r' at the end of a string of more than one byte
	void trim_seq() { if (last_cr && rank - start.back() > 1) rewind(rank - 1), last_cr = false; }
	void trim_qual() { if (last_cr && qual_len > 1) --qual_len, last_cr = false; }
	void end_fastq() // read_record: last_char = 0; the lengths must agree
	{
		if (qual_len != rank - start.back()) drop_record();
		st = PRE;
	}
	void feed(const uint8_t *p, size_t n)
	{
		for (size_t i = 0; i < n; ++i) {
			const uint32_t c = p[i];
			switch (st) {
			case PRE: if (c == '>' || c == '@') begin_record(); break;
			case NAME:
				++hdr_bytes;
				if (gdx_space(c)) st = c == '\n' ? LS : COMMENT;
				else names.back().push_back((char)c);
				break;
			case COMMENT: { // the rest of the header line
				const void *q = memchr(p + i, '\n', n - i);
				if (!q) { hdr_bytes += n - i, i = n; break; }
				hdr_bytes += (size_t)((const uint8_t *)q - (p + i)) + 1, i = (size_t)((const uint8_t *)q - p), st = LS;
				break;
			}
			case LS:
				if (c == '\n') break; // an empty line
				if (c == '>' || c == '@') { begin_record(); break; }
				if (c == '+') { st = PLUS; break; }
				push(c), line_bytes = 0, st = SQ;
				break;
			case SQ:
				++line_bytes;
				if (c == '\n') trim_seq(), st = LS;
				else push(c);
				break;
			case PLUS: if (c == '\n') st = QUAL, qual_len = 0, line_bytes = 0, last_cr = false; break;
			case QUAL: // lines are appended while the string is shorter than the sequence; the test comes behind every line, not before the first
				++line_bytes;
				if (c == '\n') {
					trim_qual(), line_bytes = 0;
					if (qual_len >= rank - start.back()) end_fastq();
				} else ++qual_len, last_cr = c == '\r';
				break;
			}
		}
	}
	void finish() // the end of the file
	{
		if (st == NAME && hdr_bytes == 0) drop_record();            // ks_getuntil2 has read nothing: kseq_read returns -1
		else if (st == SQ) { if (line_bytes) trim_seq(); }          // (with nothing read it returns before the trim)
		else if (st == PLUS) drop_record();                         // no quality string: -2
		else if (st == QUAL) { if (line_bytes) trim_qual(); end_fastq(); }
		st = PRE;
	}
	// the state the device may take the next block in, or -1.  At the very start of the file the device's condition "byte 0 is '>'" stands
	// in for the scan of PRE.
	int device_state(bool at_file_start) const
	{
		if (st == LS) return GDR_LS;
		if (st == NAME || st == COMMENT) return GDR_HD;
		if (st == SQ && !last_cr) return GDR_SQ;
		if (st == PRE && at_file_start) return GDR_LS;
		return -1;
	}
	// the bytes [0, end) of a header line the device found: the name goes on up to the first byte isspace() accepts
	void header_bytes(const uint8_t *p, size_t end, bool closed)
	{
		hdr_bytes += end + (closed ? 1 : 0);
		if (st == NAME) {
			size_t e = 0;
			while (e < end && !gdx_space(p[e])) ++e;
			names.back().append((const char *)p, e);
			if (e < end) st = COMMENT;
		}
		if (closed) st = LS;
	}
	// a block the device claimed: its header rows, the bases it placed, the state at its end
	void device_block(const uint8_t *text, uint32_t n, const GdrHdr *rows, uint32_t n_rows, uint32_t run_nl, uint32_t bases, int state_out)
	{
		const uint64_t base0 = rank;
		if (st == PRE) st = LS; // (the start of the file)
		if (st == NAME || st == COMMENT) header_bytes(text, run_nl == GDX_NONE ? n : run_nl, run_nl != GDX_NONE);
		for (uint32_t r = 0; r < n_rows; ++r) {
			rank = base0 + rows[r].base_rank;
			begin_record();
			const uint32_t from = rows[r].gt_off + 1, to = rows[r].nl_off == GDX_NONE ? n : rows[r].nl_off;
			header_bytes(text + from, to - from, rows[r].nl_off != GDX_NONE);
		}
		rank = base0 + bases;
		if (state_out == GDR_LS) st = LS;
		else if (state_out == GDR_SQ) st = SQ, line_bytes = 1, last_cr = false;
		// (GDR_HD: header_bytes left NAME or COMMENT)
	}
};

// ---- the loop over the blocks of a file ---------------------------------------------------------------------------------------------
struct GdrBlockOut {
	uint32_t claimed = 0;          // n or 0
	int state_out = -1;
	uint32_t bases = 0, run_nl = GDX_NONE;
	std::vector<GdrHdr> rows;
};
// what runs the passes on a block and keeps the bases: the device (ref_fasta_driver.hip.h) or the emulator
struct GdRefExec {
	virtual ~GdRefExec() {}
	// the passes on text[0, n) in state state_in, the bases going to ranks base0 ..; < 0: failed (why)
	virtual int block(const uint8_t *text, uint32_t n, int state_in, uint64_t base0, GdrBlockOut &out, std::string &why) = 0;
	// bases the host grammar produced, to ranks at ..
	virtual int store(uint64_t at, const uint8_t *nt4, size_t n, std::string &why) = 0;
};
struct GdRefStats {
	int64_t file_bytes = 0, text_bytes = 0, blocks = 0, blocks_host = 0, bases_device = 0, bases_host = 0;
	double s_read = 0, s_inflate = 0, s_device = 0, s_host = 0, s_build = 0;
};
// the state at the end of a claimed block, from its last byte and its header counts
static inline int gdr_state_out(const uint8_t *text, uint32_t n, int state_in, uint32_t n_hstart, uint32_t n_hend)
{
	if (n == 0) return state_in;
	if (text[n - 1] == '\n') return GDR_LS;
	return (state_in == GDR_HD ? 1u : 0u) + n_hstart > n_hend ? GDR_HD : GDR_SQ;
}
// One block: the device's if it claims it, else the grammar's.  file_start: no byte of the file has been read before this block.
static inline int gd_ref_one_block(GdRefGrammar &G, GdRefExec &X, GdRefStats &S, const uint8_t *text, size_t n, bool file_start, double (*now)(), std::string &why)
{
	++S.blocks, S.text_bytes += (int64_t)n;
	const int sin = n < ((size_t)1 << 31) ? G.device_state(file_start) : -1;
	if (sin >= 0 && !(file_start && n && text[0] != '>')) {
		const double t0 = now();
		GdrBlockOut out;
		if (X.block(text, (uint32_t)n, sin, G.rank, out, why) < 0) return -1;
		S.s_device += now() - t0;
		if (out.claimed == n) {
			G.device_block(text, (uint32_t)n, out.rows.data(), (uint32_t)out.rows.size(), out.run_nl, out.bases, out.state_out);
			S.bases_device += out.bases;
			return 0;
		}
	}
	const double t0 = now();
	++S.blocks_host;
	const uint64_t before = G.rank;
	G.feed(text, n);
	if (G.rank > before) S.bases_host += (int64_t)(G.rank - before); // (bases taken back later are not subtracted: the count says who did the work)
	S.s_host += now() - t0;
	return 0;
}
// what the grammar has produced since the last call goes to the executor's buffer
static inline int gd_ref_flush(GdRefGrammar &G, GdRefExec &X, std::string &why)
{
	if (G.hb.empty()) return 0;
	const int rc = X.store(G.hb_base, G.hb.data(), G.hb.size(), why);
	G.hb.clear();
	return rc;
}
