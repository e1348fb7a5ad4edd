// Stand-alone host run of the device SAM formatter, meant to be built with -fsanitize=address,undefined: the host's flattening
// (sam_flatten.h) and the statements of sam_encode_kernel (sam_record.h: gds_format) as loops over 64 lanes, on exact-size copies of the
// pools and of the stream, so that a read or a store outside them is a sanitizer report.  It reads the dumps of samopts_emul.cpp (same
// items, same grammar: MODE sam, FLAG, RG, HDR, SQ, READ, COMMENT, REG) and repeats the record loop of the batch formatter twice.
//
//   sam_emul fmt <dump> <out.sam>   prints the SAM text of the dump as the existing writer gives it (gd_sam_header / gd_write_sam) and
//                                   writes the text of the same records as the 64 lanes give it to <out.sam> (the header first when the
//                                   dump has an HDR item), and gds_line_size of every row, one per line, to <out.sam>.sizes.  Every line is
//                                   formatted twice, with the lanes running 0..63 and 63..0; the wave scan is a loop (gds_wave_scan).
// Exit status 0; 2 usage / open errors; 3 a malformed dump; 4 a refused read group; 6 a read the flattening refuses (the reason, which
// names the read, goes to stderr; nothing is written); 7 the two lane orders differ, a line's bytes do not end at its size, its size is
// not gds_line_size of its row, or a byte of the stream was left unwritten.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>
#include "sam_flatten.h"

static std::vector<std::string> split_tabs(const std::string &l)
{
	std::vector<std::string> f;
	size_t at = 0;
	for (;;) {
		const size_t t = l.find('\t', at);
		f.push_back(l.substr(at, t == std::string::npos ? t : t - at));
		if (t == std::string::npos) break;
		at = t + 1;
	}
	return f;
}

struct Read {
	std::string qname, seq, qual, comment;
	bool has_qual = false, has_comment = false;
	std::vector<GdReg> regs;
	std::vector<std::string> ds;
	std::vector<bool> has_ds;
};

// exact-size heap copy (a vector's capacity may exceed its size: reads behind size would go unseen)
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T> &v)
{
	std::unique_ptr<T[]> p(new T[v.size()]);
	for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
	return p;
}

static int encode(const GdsPart &P, const std::vector<uint8_t> &rname_v, const std::vector<uint64_t> &roff_v, std::string &out)
{
	const auto text = exact(P.text), blob = exact(P.blob), rname = exact(rname_v);
	const auto cig = exact(P.cig);
	const auto roff = exact(roff_v);
	std::string run[2];
	for (int down = 0; down < 2; ++down) {
		std::unique_ptr<uint8_t[]> stream(new uint8_t[P.bytes]);
		for (uint64_t k = 0; k < P.bytes; ++k) stream[k] = 0xA5;
		uint64_t at = 0;
		for (const GdsRec &r : P.rec) {
			if (r.out != at || r.size != gds_line_size(r)) return 7; // the prefix sum of the line sizes
			if (r.out > P.bytes || P.bytes - r.out < r.size) return 7; // the kernel's own guard
			for (uint32_t i = 0; i < 64; ++i) {
				const uint32_t lane = down ? 63 - i : i;
				if (gds_format(r, text.get(), cig.get(), blob.get(), rname.get(), roff.get(), stream.get(), lane) != r.size) return 7;
			}
			at += r.size;
		}
		if (at != P.bytes) return 7;
		run[down].assign((const char *)stream.get(), P.bytes);
	}
	if (run[0] != run[1]) return 7;
	// every byte of a line is written: format again over a stream of another fill and compare
	{
		std::unique_ptr<uint8_t[]> stream(new uint8_t[P.bytes]);
		for (uint64_t k = 0; k < P.bytes; ++k) stream[k] = 0x5A;
		for (const GdsRec &r : P.rec)
			for (uint32_t lane = 0; lane < 64; ++lane) (void)gds_format(r, text.get(), cig.get(), blob.get(), rname.get(), roff.get(), stream.get(), lane);
		if (run[0] != std::string((const char *)stream.get(), P.bytes)) return 7;
	}
	out += run[0];
	return 0;
}

static int run_fmt(std::istream &in, const char *out_path)
{
	std::string l, mode, rg_line, rg_id, err, version;
	int64_t flag = 0;
	bool with_hdr = false;
	std::vector<std::string> argv_s;
	std::vector<GdSeqInfo> sq;
	std::vector<Read> reads;
	while (std::getline(in, l)) {
		const std::vector<std::string> f = split_tabs(l);
		if (f[0] == "MODE" && f.size() == 2) mode = f[1];
		else if (f[0] == "FLAG" && f.size() == 2) flag = strtoll(f[1].c_str(), nullptr, 10);
		else if (f[0] == "RG" && f.size() == 2) {
			if (!gd_parse_rg_line(f[1].c_str(), rg_line, rg_id, err)) { fprintf(stderr, "%s\n", err.c_str()); return 4; }
		} else if (f[0] == "HDR" && f.size() >= 2) {
			with_hdr = true, version = f[1];
			argv_s.assign(f.begin() + 2, f.end());
		} else if (f[0] == "SQ" && f.size() == 3) {
			GdSeqInfo s;
			s.name = f[1], s.offset = 0, s.len = (uint32_t)strtoul(f[2].c_str(), nullptr, 10);
			sq.push_back(s);
		} else if (f[0] == "READ" && f.size() == 4) {
			Read r;
			r.qname = f[1], r.seq = f[2], r.has_qual = f[3] != "*", r.qual = f[3];
			if (r.has_qual && r.qual.size() != r.seq.size()) return 3;
			reads.push_back(r);
		} else if (f[0] == "COMMENT" && !reads.empty()) {
			reads.back().has_comment = true, reads.back().comment = l.substr(8);
		} else if (f[0] == "REG" && f.size() == 4 && !reads.empty()) {
			GdReg r;
			int hp = 0;
			if (sscanf(f[1].c_str(), "%d %d %d %d %d %d %d %d %d %d %d %d %u %u %u %d %d %u %d", &r.id, &r.cnt, &r.rid, &r.score, &r.qs, &r.qe, &r.rs, &r.re,
			           &r.parent, &r.subsc, &r.mlen, &r.blen, &r.mapq, &r.rev, &r.sam_pri, &r.dp_score, &r.dp_max, &r.n_ambi, &hp) != 19) return 3;
			r.has_p = hp != 0;
			if (r.rid < 0 || (size_t)r.rid >= sq.size() || r.qs < 0 || r.qe < r.qs || (size_t)r.qe > reads.back().seq.size()) return 3;
			if (f[2] != "*") {
				const char *p = f[2].c_str();
				while (*p) {
					char *e;
					const unsigned long n = strtoul(p, &e, 10);
					const char *op = *e ? strchr("MIDNSHP=XB", *e) : nullptr;
					if (e == p || !op || n >= (1ul << 28)) return 3;
					r.cigar.push_back((uint32_t)(n << 4 | (uint32_t)(op - "MIDNSHP=XB")));
					p = e + 1;
				}
			}
			reads.back().regs.push_back(r);
			reads.back().has_ds.push_back(f[3] != "-");
			reads.back().ds.push_back(f[3]);
		} else return 3;
	}
	if (mode != "sam") return 3;
	GdRefView R;
	R.S = nullptr, R.seq = sq.data(), R.n_seq = (uint32_t)sq.size();
	std::string s, dev;
	if (with_hdr) {
		std::vector<const char *> av;
		for (const std::string &a : argv_s) av.push_back(a.c_str());
		const std::string h = gd_sam_header(R, rg_line, version == "-" ? nullptr : version.c_str(), (int)av.size(), av.data());
		s += h, dev += h;
	}
	const char *rg = rg_id.empty() ? nullptr : rg_id.c_str();
	GdsPart P;
	for (const Read &rd : reads) { // the loop of gd_sam_batch_impl, once per formatter
		const int nr = (int)rd.regs.size();
		const char *cm = rd.has_comment && (flag & GD_F_COPY_COMMENT) ? rd.comment.c_str() : nullptr;
		const char *q = rd.has_qual ? rd.qual.c_str() : nullptr;
		const int l_seq = (int)rd.seq.size();
		const std::string why = gds_flatten_read(P, R, rd.qname.c_str(), rd.seq.c_str(), q, l_seq, rd.regs, flag, rg, rd.has_comment ? rd.comment.c_str() : nullptr,
		                                         [&](int j, size_t *n) { *n = rd.has_ds[j] ? rd.ds[j].size() : 0; return rd.has_ds[j] ? rd.ds[j].c_str() : (const char *)nullptr; });
		if (!why.empty()) { fprintf(stderr, "%s\n", why.c_str()); return 6; }
		if (nr == 0) {
			if (flag & GD_F_SAM_HIT_ONLY) continue;
			gd_write_sam(s, R, rd.qname.c_str(), rd.seq.c_str(), q, l_seq, rd.regs, -1, flag, nullptr, 0, rg, cm), s += '\n';
			continue;
		}
		for (int j = 0; j < nr; ++j) {
			if ((flag & GD_F_NO_PRINT_2ND) && rd.regs[j].id != rd.regs[j].parent) continue;
			const char *ds = rd.has_ds[j] ? rd.ds[j].c_str() : nullptr;
			gd_write_sam(s, R, rd.qname.c_str(), rd.seq.c_str(), q, l_seq, rd.regs, j, flag, ds, rd.has_ds[j] ? rd.ds[j].size() : 0, rg, cm), s += '\n';
		}
	}
	std::vector<uint8_t> rname;
	std::vector<uint64_t> roff;
	gds_rname_pool(R, rname, roff);
	const int rc = encode(P, rname, roff, dev);
	if (rc) return rc;
	FILE *fo = fopen(out_path, "wb");
	if (!fo) { perror(out_path); return 2; }
	if (fwrite(dev.data(), 1, dev.size(), fo) != dev.size() || fclose(fo) != 0) return 2;
	const std::string sp = std::string(out_path) + ".sizes";
	fo = fopen(sp.c_str(), "wb");
	if (!fo) { perror(sp.c_str()); return 2; }
	for (const GdsRec &r : P.rec) fprintf(fo, "%llu\n", (unsigned long long)gds_line_size(r));
	if (fclose(fo) != 0) return 2;
	fwrite(s.data(), 1, s.size(), stdout);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 4 || std::string(argv[1]) != "fmt") { fprintf(stderr, "usage: sam_emul fmt <dump> <out.sam>\n"); return 2; }
	std::ifstream in(argv[2]);
	if (!in) { perror(argv[2]); return 2; }
	return run_fmt(in, argv[3]);
}
