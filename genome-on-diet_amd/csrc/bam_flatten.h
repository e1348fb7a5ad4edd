// The host's half of the BAM encoder: alignment records (GdReg) and their read -> rows of the flat table bam_record.h defines, with the
// pools the rows point into, the BAM header, and the parser that turns a read's comment into ready tag bytes.  Plain C++; no HIP in here
// (the driver in bam_driver.hip.h and the emulator tests/emul/bam_emul.cpp both run it).
//
// Which records exist, which slice of SEQ / QUAL they carry, their clips and the order of their tags are those of gd_write_sam
// (map_host.h) for the same arguments: gdb_flatten_read is its twin, field by field, and calls the same helpers for the SA tag.
// de:f: is evaluated here: the float32 nearest to the decimal text the SAM line prints ("%.4f", or 0).
#pragma once
#include <stdlib.h>
#include <string>
#include <vector>
#include "bam_record.h"
#include "map_host.h"

// rows and pools of a run of reads; offsets are relative to the pools of this part until the driver merges the parts (gd_bam_flatten)
struct GdbPart {
	std::vector<GdbRec> rec;
	std::vector<uint8_t> text, blob;
	std::vector<uint32_t> cig;
	uint64_t bytes = 0; // of the records: sum of 4 + block_size
	void clear() { rec.clear(), text.clear(), blob.clear(), cig.clear(), bytes = 0; }
};

static inline void gdb_put_le(std::vector<uint8_t> &b, uint64_t v, int n) { for (int k = 0; k < n; ++k) b.push_back((uint8_t)(v >> (8 * k))); }
static inline void gdb_put_z(std::vector<uint8_t> &b, const char *tag2, const char *s, size_t n)
{
	b.push_back((uint8_t)tag2[0]), b.push_back((uint8_t)tag2[1]), b.push_back('Z');
	b.insert(b.end(), s, s + n), b.push_back(0);
}

// One field of a comment, "XX:T:value" with T in A i f Z H B (B subtypes cCsSiIf), appended as a BAM tag.  false: it is no tag.
static inline bool gdb_parse_tag(const char *f, size_t n, std::vector<uint8_t> &b)
{
	auto alnum = [](char c, bool first) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (!first && c >= '0' && c <= '9'); };
	if (n < 5 || f[2] != ':' || f[4] != ':' || !alnum(f[0], true) || !alnum(f[1], false)) return false;
	const std::string v(f + 5, n - 5);
	auto whole_int = [](const std::string &t, long long &out) {
		size_t k = 0;
		if (k < t.size() && (t[k] == '-' || t[k] == '+')) ++k;
		if (k == t.size() || t.size() - k > 10) return false;
		for (size_t j = k; j < t.size(); ++j) if (t[j] < '0' || t[j] > '9') return false;
		out = strtoll(t.c_str(), nullptr, 10);
		return true;
	};
	auto whole_float = [](const std::string &t, float &out) {
		// [-+]?[0-9]*\.?[0-9]+([eE][-+]?[0-9]+)? of the SAM specification, then the nearest float32
		auto digit = [&](size_t k) { return k < t.size() && t[k] >= '0' && t[k] <= '9'; };
		size_t k = 0, d = 0;
		if (k < t.size() && (t[k] == '-' || t[k] == '+')) ++k;
		while (digit(k)) ++k, ++d;
		if (k < t.size() && t[k] == '.') { ++k, d = 0; while (digit(k)) ++k, ++d; }
		if (d == 0) return false;
		if (k < t.size() && (t[k] == 'e' || t[k] == 'E')) {
			++k;
			if (k < t.size() && (t[k] == '-' || t[k] == '+')) ++k;
			if (!digit(k)) return false;
			while (digit(k)) ++k;
		}
		if (k != t.size()) return false;
		out = strtof(t.c_str(), nullptr);
		return true;
	};
	const size_t at0 = b.size();
	b.push_back((uint8_t)f[0]), b.push_back((uint8_t)f[1]);
	bool ok = false;
	switch (f[3]) {
	case 'A': if (v.size() == 1 && v[0] >= '!' && v[0] <= '~') b.push_back('A'), b.push_back((uint8_t)v[0]), ok = true; break;
	case 'i': {
		long long x;
		if (whole_int(v, x) && x >= -2147483648LL && x <= 4294967295LL) b.push_back((uint8_t)gdb_int_type(x)), gdb_put_le(b, (uint64_t)x, (int)gdb_int_width(x)), ok = true;
		break;
	}
	case 'f': {
		float x;
		if (whole_float(v, x)) { uint32_t u; memcpy(&u, &x, 4); b.push_back('f'), gdb_put_le(b, u, 4), ok = true; }
		break;
	}
	case 'Z': b.push_back('Z'), b.insert(b.end(), v.begin(), v.end()), b.push_back(0), ok = true; break;
	case 'H': {
		ok = v.size() % 2 == 0;
		for (char c : v) ok = ok && ((c >= '0' && c <= '9') || (c >= 'A' && c <= 'F') || (c >= 'a' && c <= 'f'));
		if (ok) b.push_back('H'), b.insert(b.end(), v.begin(), v.end()), b.push_back(0);
		break;
	}
	case 'B': {
		static const char sub[] = "cCsSiIf";
		static const int width[] = {1, 1, 2, 2, 4, 4, 4};
		static const long long lo[] = {-128, 0, -32768, 0, -2147483648LL, 0}, hi[] = {127, 255, 32767, 65535, 2147483647LL, 4294967295LL};
		const char *s = v.empty() ? nullptr : strchr(sub, v[0]);
		if (!s || !v[0]) break;
		const int t = (int)(s - sub);
		b.push_back('B'), b.push_back((uint8_t)v[0]);
		const size_t cnt_at = b.size();
		gdb_put_le(b, 0, 4);
		uint32_t cnt = 0;
		size_t p = 1;
		ok = true;
		while (ok && p < v.size()) {
			if (v[p] != ',') { ok = false; break; }
			const size_t q = v.find(',', p + 1);
			const std::string item = v.substr(p + 1, q == std::string::npos ? q : q - p - 1);
			if (t == 6) {
				float x;
				uint32_t u;
				if ((ok = whole_float(item, x))) memcpy(&u, &x, 4), gdb_put_le(b, u, 4);
			} else {
				long long x;
				if ((ok = whole_int(item, x) && x >= lo[t] && x <= hi[t])) gdb_put_le(b, (uint64_t)x, width[t]);
			}
			++cnt, p = q == std::string::npos ? v.size() : q;
		}
		if (ok) for (int k = 0; k < 4; ++k) b[cnt_at + k] = (uint8_t)(cnt >> (8 * k));
		break;
	}
	default: break;
	}
	if (!ok) b.resize(at0);
	return ok;
}

// every tab-separated field of a comment; false (and nothing appended) if one of them is no tag
static inline bool gdb_parse_comment(const char *cm, std::vector<uint8_t> &b)
{
	const size_t at0 = b.size();
	for (const char *p = cm;;) {
		const char *e = strchr(p, '\t');
		const size_t n = e ? (size_t)(e - p) : strlen(p);
		if (!gdb_parse_tag(p, n, b)) { b.resize(at0); return false; }
		if (!e) return true;
		p = e + 1;
	}
}

// de:f: of gd_write_tags as BAM stores it
static inline float gdb_de_value(const GdReg &r)
{
	int32_t n_gap = 0, n_gapo = 0;
	for (uint32_t cg : r.cigar) if ((cg & 0xf) == 1 || (cg & 0xf) == 2) ++n_gapo, n_gap += (int32_t)(cg >> 4);
	const double ident = (double)r.mlen / (r.blen + (int)r.n_ambi - n_gap + n_gapo);
	if (1.0 - ident == 0.0) return 0.0f;
	char buf[32];
	snprintf(buf, sizeof buf, "%.4f", 1.0 - ident);
	return strtof(buf, nullptr);
}

// The records of one read, in the order and under the rules of gd_sam_batch_impl's loop body + gd_write_sam.  ds / ds_len: the
// difference string of record j (nullptr: none).  Returns "" or why the read cannot be stored.
template <class DsOf>
static inline std::string gdb_flatten_read(GdbPart &P, const GdRefView &R, const char *qname, const char *seq, const char *qual, int l_seq, const std::vector<GdReg> &regs,
                                           int64_t opt_flag, const char *rg_id, const char *comment, DsOf ds_of)
{
	if (opt_flag & GD_F_NO_QUAL) qual = nullptr;
	if (!(opt_flag & GD_F_COPY_COMMENT)) comment = nullptr;
	const int nr = (int)regs.size();
	if (nr == 0 && (opt_flag & GD_F_SAM_HIT_ONLY)) return "";
	const size_t l_name = strlen(qname);
	if (l_name > GDB_MAX_NAME) return "read " + std::string(qname, 32) + "...: a name of " + std::to_string(l_name) + " bytes; BAM holds 254";
	if (l_seq < 0) return "read " + std::string(qname) + ": negative length";
	// what every record of the read shares: its text, and the blobs of its read group and its comment
	const uint64_t name_at = P.text.size();
	P.text.insert(P.text.end(), qname, qname + l_name);
	const uint64_t seq_at = P.text.size();
	P.text.insert(P.text.end(), seq, seq + l_seq);
	const uint64_t qual_at = P.text.size();
	if (qual) P.text.insert(P.text.end(), qual, qual + l_seq);
	const uint64_t rg_at = P.blob.size();
	if (rg_id && rg_id[0]) gdb_put_z(P.blob, "RG", rg_id, strlen(rg_id));
	const uint32_t rg_len = (uint32_t)(P.blob.size() - rg_at);
	const uint64_t cm_at = P.blob.size();
	if (comment && !gdb_parse_comment(comment, P.blob)) return "read " + std::string(qname) + ": its comment is not a list of SAM tags (XX:T:value separated by tabs), so BAM cannot store it";
	const uint32_t cm_len = (uint32_t)(P.blob.size() - cm_at);
	auto finish = [&](GdbRec &g) {
		const uint64_t bs = gdb_block_size(g);
		if (bs > 0x7fffffffull) return false;
		g.block_size = (uint32_t)bs, g.out = P.bytes, P.bytes += 4 + bs;
		P.rec.push_back(g);
		return true;
	};
	for (int j = nr == 0 ? -1 : 0; j < nr; ++j) {
		GdbRec g;
		memset(&g, 0, sizeof g);
		g.name = name_at, g.l_name = (uint32_t)l_name + 1, g.seq = seq_at, g.qual = qual_at, g.has_qual = qual ? 1 : 0;
		g.blob[0] = rg_at, g.blob_len[0] = rg_len, g.blob[2] = cm_at, g.blob_len[2] = cm_len, g.blob[1] = P.blob.size();
		if (j < 0) { // the unmapped record
			g.refID = -1, g.pos = -1, g.bin = GDB_UNMAPPED_BIN, g.flag = 4, g.l_seq = (uint32_t)l_seq;
			if (!finish(g)) return "read " + std::string(qname) + ": a record of 2 GiB or more";
			break;
		}
		const GdReg &r = regs[j];
		if ((opt_flag & GD_F_NO_PRINT_2ND) && r.id != r.parent) continue;
		if (r.rid < 0 || (uint32_t)r.rid >= R.n_seq || r.qs < 0 || r.qe < r.qs || r.qe > l_seq)
			return "read " + std::string(qname) + " record " + std::to_string(j) + ": rid or qs / qe outside the index or the read";
		uint32_t flag = 0;
		if (r.rev) flag |= 0x10;
		if (r.parent != r.id) flag |= 0x100;
		else if (!r.sam_pri) flag |= 0x800;
		g.flag = flag, g.refID = r.rid, g.pos = r.rs, g.mapq = r.mapq, g.mapped = 1, g.has_p = r.has_p ? 1 : 0, g.rev = r.rev ? 1 : 0;
		const bool whole = (flag & 0x900) == 0 || (opt_flag & GD_F_SOFTCLIP);
		if (whole) g.l_seq = (uint32_t)l_seq;
		else if (flag & 0x100) g.l_seq = 0, g.has_qual = 0;
		else g.l_seq = (uint32_t)(r.qe - r.qs), g.seq = seq_at + (uint32_t)r.qs, g.qual = qual_at + (uint32_t)r.qs;
		uint64_t ref_len = 0;
		if (r.has_p) {
			g.clip0 = r.rev ? (uint32_t)(l_seq - r.qe) : (uint32_t)r.qs, g.clip1 = r.rev ? (uint32_t)r.qs : (uint32_t)(l_seq - r.qe);
			g.clip_op = (flag & 0x800) && !(opt_flag & GD_F_SOFTCLIP) ? 5 : 4;
			g.cig = P.cig.size(), g.n_cig = (uint32_t)r.cigar.size();
			P.cig.insert(P.cig.end(), r.cigar.begin(), r.cigar.end());
			for (uint32_t cg : r.cigar) if ((0x18d >> (cg & 0xf)) & 1) ref_len += cg >> 4; // M D N = X
			const uint64_t n_op = (uint64_t)gdb_cg_ops(g);
			g.in_tag = n_op > GDB_MAX_OPS, g.n_op = g.in_tag ? 2 : (uint32_t)n_op;
			if (ref_len >= (1ull << 28) || g.clip0 >= (1u << 28) || g.clip1 >= (1u << 28)) return "read " + std::string(qname) + ": a CIGAR length of 2^28 or more";
		}
		g.ref_len = (uint32_t)ref_len;
		g.bin = gdb_reg2bin(r.rs, (int64_t)r.rs + (ref_len ? (int64_t)ref_len : 1));
		g.nm = r.blen - r.mlen + (int)r.n_ambi, g.ms = r.dp_max, g.as = r.dp_score, g.nn = r.n_ambi, g.tp = r.id == r.parent ? 'P' : 'S';
		g.cm = r.cnt, g.s1 = r.score, g.has_s2 = r.parent == r.id, g.s2 = r.subsc;
		if (r.has_p) g.de = gdb_de_value(r);
		{ // blob[1]: SA:Z: and the difference string, as gd_write_sam orders them
			std::string sa;
			gd_write_sa_tag(sa, R, regs, j, l_seq);
			if (!sa.empty()) gdb_put_z(P.blob, "SA", sa.data() + 6, sa.size() - 6); // behind "\tSA:Z:"
			size_t dl = 0;
			const char *ds = ds_of(j, &dl);
			if (r.has_p && !r.cigar.empty() && ds && (opt_flag & (GD_F_OUT_CS | GD_F_OUT_MD))) gdb_put_z(P.blob, (opt_flag & GD_F_OUT_MD) ? "MD" : "cs", ds, dl);
			g.blob_len[1] = (uint32_t)(P.blob.size() - g.blob[1]);
		}
		if (!finish(g)) return "read " + std::string(qname) + ": a record of 2 GiB or more";
	}
	return "";
}

// "BAM\1", the header text (no NUL), and the reference dictionary
static inline std::string gdb_header(const GdRefView &R, const std::string &text)
{
	std::string s("BAM\1", 4);
	auto put32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) s += (char)(v >> (8 * k)); };
	put32((uint32_t)text.size()), s += text, put32(R.n_seq);
	for (uint32_t i = 0; i < R.n_seq; ++i) {
		put32((uint32_t)R.seq[i].name.size() + 1), s += R.seq[i].name, s += '\0';
		put32(R.seq[i].len);
	}
	return s;
}
