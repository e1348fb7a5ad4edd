// The host's half of the device SAM formatter: alignment records (GdReg) and their read -> rows of the flat table sam_record.h defines,
// with the pools the rows point into.  Plain C++; no HIP in here (the driver in sam_driver.hip.h and the emulator tests/emul/sam_emul.cpp
// both run it).  The sibling of bam_flatten.h, which stays as it is.
//
// Which lines exist, which slice of SEQ / QUAL they carry, their clips and the order of their tags are those of gd_sam_batch_impl's loop
// and gd_write_sam (map_host.h) for the same arguments: gds_flatten_read is their twin, field by field, and calls the same helpers for
// the SA tag and the difference tag.  The de:f: text is formatted here, with gd_write_tags's own statements.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>
#include "sam_record.h"
#include "map_host.h"

// rows and pools of a run of reads; offsets are relative to the pools of this part until the driver merges the parts (gd_sam_flatten)
struct GdsPart {
	std::vector<GdsRec> rec;
	std::vector<uint8_t> text, blob;
	std::vector<uint32_t> cig;
	uint64_t bytes = 0; // of the lines: the sum of their sizes
	void clear() { rec.clear(), text.clear(), blob.clear(), cig.clear(), bytes = 0; }
};

// the index's contig names behind one another, and where each starts (n_seq + 1 entries): RNAME of every row of a batch
static inline void gds_rname_pool(const GdRefView &R, std::vector<uint8_t> &pool, std::vector<uint64_t> &off)
{
	pool.clear(), off.assign((size_t)R.n_seq + 1, 0);
	for (uint32_t i = 0; i < R.n_seq; ++i) {
		pool.insert(pool.end(), R.seq[i].name.begin(), R.seq[i].name.end());
		off[i + 1] = pool.size();
	}
}

// the text behind "\tde:f:" as gd_write_tags prints it (mm_event_identity); returns its length
static inline uint32_t gds_de_text(const GdReg &r, char buf[16])
{
	int32_t n_gap = 0, n_gapo = 0;
	for (uint32_t cg : r.cigar) if ((cg & 0xf) == 1 || (cg & 0xf) == 2) ++n_gapo, n_gap += (int32_t)(cg >> 4);
	const double ident = (double)r.mlen / (r.blen + (int)r.n_ambi - n_gap + n_gapo);
	const double div = 1.0 - ident;
	if (div == 0.0) buf[0] = '0', buf[1] = 0;
	else snprintf(buf, 16, "%.4f", 1.0 - ident);
	return (uint32_t)strlen(buf);
}

// The lines of one read, in the order and under the rules of gd_sam_batch_impl's loop body + gd_write_sam.  ds_of(j, &len): the
// difference string of record j (nullptr: none).  Returns "" or why the read cannot be written.
template <class DsOf>
static inline std::string gds_flatten_read(GdsPart &P, const GdRefView &R, const char *qname, const char *seq, const char *qual, int l_seq, const std::vector<GdReg> &regs,
                                           int64_t opt_flag, const char *rg_id, const char *comment, DsOf ds_of)
{
	if (opt_flag & GD_F_NO_QUAL) qual = nullptr;
	if (!(opt_flag & GD_F_COPY_COMMENT)) comment = nullptr;
	const int nr = (int)regs.size();
	if (nr == 0 && (opt_flag & GD_F_SAM_HIT_ONLY)) return "";
	const size_t l_name = strlen(qname);
	if (l_name > 0x7fffffffu) return "read " + std::string(qname, 32) + "...: a name of 2 GiB or more";
	if (l_seq < 0) return "read " + std::string(qname) + ": negative length";
	// what every line of the read shares: its text, and the blobs of its read group and its comment
	const uint64_t name_at = P.text.size();
	P.text.insert(P.text.end(), qname, qname + l_name);
	const uint64_t seq_at = P.text.size();
	P.text.insert(P.text.end(), seq, seq + l_seq);
	const uint64_t qual_at = P.text.size();
	if (qual) P.text.insert(P.text.end(), qual, qual + l_seq);
	auto put = [&](const char *s, size_t n) { P.blob.insert(P.blob.end(), s, s + n); };
	const uint64_t rg_at = P.blob.size();
	if (rg_id && rg_id[0]) put("\tRG:Z:", 6), put(rg_id, strlen(rg_id));
	const uint64_t cm_at = P.blob.size();
	if (comment) put("\t", 1), put(comment, strlen(comment));
	const uint64_t cm_end = P.blob.size();
	if (cm_at - rg_at > 0xffffffffull || cm_end - cm_at > 0xffffffffull) return "read " + std::string(qname) + ": a read group or comment of 4 GiB or more";
	auto finish = [&](GdsRec &g) {
		g.size = gds_line_size(g), g.out = P.bytes, P.bytes += g.size;
		P.rec.push_back(g);
	};
	for (int j = nr == 0 ? -1 : 0; j < nr; ++j) {
		GdsRec g;
		memset(&g, 0, sizeof g);
		g.name = name_at, g.l_name = (uint32_t)l_name, g.seq = seq_at, g.qual = qual_at, g.has_qual = qual ? 1 : 0;
		g.blob[0] = rg_at, g.blob_len[0] = (uint32_t)(cm_at - rg_at), g.blob[2] = cm_at, g.blob_len[2] = (uint32_t)(cm_end - cm_at), g.blob[1] = P.blob.size();
		if (j < 0) { // the unmapped line
			g.flag = 4, g.l_seq = (uint32_t)l_seq;
			finish(g);
			break;
		}
		const GdReg &r = regs[j];
		if ((opt_flag & GD_F_NO_PRINT_2ND) && r.id != r.parent) continue;
		if (r.rid < 0 || (uint32_t)r.rid >= R.n_seq || r.qs < 0 || r.qe < r.qs || r.qe > l_seq)
			return "read " + std::string(qname) + " record " + std::to_string(j) + ": rid or qs / qe outside the index or the read";
		if (R.seq[r.rid].name.size() > 0xffffffffull || r.cigar.size() >= (1ull << 31)) return "read " + std::string(qname) + " record " + std::to_string(j) + ": a contig name or CIGAR too long";
		uint32_t flag = 0;
		if (r.rev) flag |= 0x10;
		if (r.parent != r.id) flag |= 0x100;
		else if (!r.sam_pri) flag |= 0x800;
		g.flag = flag, g.rid = (uint32_t)r.rid, g.l_rname = (uint32_t)R.seq[r.rid].name.size(), g.pos = r.rs + 1, g.mapq = r.mapq, g.mapped = 1, g.has_p = r.has_p ? 1 : 0, g.rev = r.rev ? 1 : 0;
		const bool whole = (flag & 0x900) == 0 || (opt_flag & GD_F_SOFTCLIP);
		if (whole) g.l_seq = (uint32_t)l_seq;
		else if (flag & 0x100) g.l_seq = 0, g.has_qual = 0, g.seq_star = 1;
		else g.l_seq = (uint32_t)(r.qe - r.qs), g.seq = seq_at + (uint32_t)r.qs, g.qual = qual_at + (uint32_t)r.qs;
		if (r.has_p) {
			g.clip0 = r.rev ? (uint32_t)(l_seq - r.qe) : (uint32_t)r.qs, g.clip1 = r.rev ? (uint32_t)r.qs : (uint32_t)(l_seq - r.qe);
			// (a clip travels as an operation, len << 4 | code, like the CIGAR's own: the limit of 2^28 bases is BAM's, and F4's)
			if (g.clip0 >= (1u << 28) || g.clip1 >= (1u << 28)) return "read " + std::string(qname) + " record " + std::to_string(j) + ": a clip of 2^28 bases or more";
			g.clip_ch = (flag & 0x800) && !(opt_flag & GD_F_SOFTCLIP) ? 'H' : 'S';
			g.cig = P.cig.size(), g.n_cig = (uint32_t)r.cigar.size();
			P.cig.insert(P.cig.end(), r.cigar.begin(), r.cigar.end());
			if ((opt_flag & GD_F_LONG_CIGAR) && r.cigar.size() > 65535 - 2) g.in_tag = r.cigar.size() + (r.qs != 0) + (r.qe != l_seq) > 65535;
			// the text lengths of the column and of the CG:B:I list, summed while the operations are at hand
			uint64_t col = 0, list = 0;
			const uint32_t n = gds_ops(g);
			for (uint32_t k = 0; k < n; ++k) {
				const uint32_t op = gds_clipped_op(g, P.cig.data(), k);
				col += 1 + gds_u32_width(op >> 4), list += 1 + gds_u32_width(op);
			}
			if (col > 0xffffffffull || list > 0xffffffffull) return "read " + std::string(qname) + " record " + std::to_string(j) + ": a CIGAR text of 4 GiB or more";
			g.cig_text = (uint32_t)col, g.cg_text = g.in_tag ? (uint32_t)list : 0;
			g.ph_s = (int32_t)g.l_seq, g.ph_n = r.re - r.rs;
			g.de_len = gds_de_text(r, (char *)g.de); // (little-endian: byte k of the text is byte k of the two words)
		}
		g.nm = r.blen - r.mlen + (int)r.n_ambi, g.ms = r.dp_max, g.as = r.dp_score, g.nn = r.n_ambi, g.tp = r.id == r.parent ? 'P' : 'S';
		g.cm = r.cnt, g.s1 = r.score, g.has_s2 = r.parent == r.id, g.s2 = r.subsc;
		{ // blob[1]: the SA tag and the difference tag, as gd_write_sam orders them
			std::string t;
			gd_write_sa_tag(t, R, regs, j, l_seq);
			if (r.has_p && !r.cigar.empty()) {
				size_t dl = 0;
				const char *ds = ds_of(j, &dl);
				gd_write_ds_tag(t, opt_flag, ds, dl);
			}
			if (t.size() > 0xffffffffull) return "read " + std::string(qname) + " record " + std::to_string(j) + ": tags of 4 GiB or more";
			put(t.data(), t.size());
			g.blob_len[1] = (uint32_t)t.size();
		}
		finish(g);
	}
	return "";
}
