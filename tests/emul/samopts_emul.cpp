// Stand-alone host run of the SAM / PAF record writers and the read-group / header code of map_host.h under the output options
// (-Y, -L, -Q, -y, -R, --sam-hit-only), meant to be built with -fsanitize=address,undefined.  It repeats the record loop of the batch
// formatters (map_pipeline.hip.h: gd_sam_batch_impl / gd_paf_batch_impl), which needs no device when no difference string is asked for.
//
//   samopts_emul fmt <file>    prints the SAM or PAF text of a dump.  One item per line, fields separated by tabs:
//        MODE  sam|paf
//        FLAG  <mm_mapopt_t::flag, decimal>
//        RG    <the -R argument as typed>                         (optional; a refused line ends the run with status 4)
//        HDR   <version>  <argv[0]>  <argv[1]> ...                (optional: the header is printed first)
//        SQ    <name>  <length>                                   (one per reference sequence, in index order)
//        READ  <qname>  <seq>  <qual or *>
//        COMMENT <the rest of the line, tabs included>            (optional, behind its READ)
//        REG   <id> <cnt> <rid> <score> <qs> <qe> <rs> <re> <parent> <subsc> <mlen> <blen> <mapq> <rev> <sam_pri> <dp_score> <dp_max>
//              <n_ambi> <has_p>  <CIGAR text or *>  <difference string or ->       (the numbers separated by blanks; behind its READ)
//   samopts_emul rg <file>     one -R argument per line; prints "ok\t<id>\t<escaped line>" or "err\t<message>" for each
// Exit status 0 when the whole input was read and processed, 2 for usage / open errors, 3 for a malformed dump.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "map_host.h"

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

static int run_rg(std::istream &in)
{
	std::string l, line, id, err;
	while (std::getline(in, l)) {
		if (gd_parse_rg_line(l.c_str(), line, id, err)) printf("ok\t%s\t%s\n", id.c_str(), line.c_str());
		else {
			if (!line.empty() || !id.empty()) return 5; // a refused line leaves nothing behind
			printf("err\t%s\n", err.c_str());
		}
	}
	return 0;
}

static int run_fmt(std::istream &in)
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
	if (mode != "sam" && mode != "paf") return 3;
	GdRefView R;
	R.S = nullptr, R.seq = sq.data(), R.n_seq = (uint32_t)sq.size();
	std::string s;
	if (with_hdr) {
		std::vector<const char *> av;
		for (const std::string &a : argv_s) av.push_back(a.c_str());
		s += gd_sam_header(R, rg_line, version == "-" ? nullptr : version.c_str(), (int)av.size(), av.data());
	}
	const char *rg = rg_id.empty() ? nullptr : rg_id.c_str();
	for (const Read &rd : reads) { // the loop of gd_sam_batch_impl / gd_paf_batch_impl
		const int nr = (int)rd.regs.size();
		const char *cm = rd.has_comment && (flag & GD_F_COPY_COMMENT) ? rd.comment.c_str() : nullptr;
		const char *q = rd.has_qual ? rd.qual.c_str() : nullptr;
		const int l_seq = (int)rd.seq.size();
		if (nr == 0) {
			if (mode == "sam") {
				if (flag & GD_F_SAM_HIT_ONLY) continue;
				gd_write_sam(s, R, rd.qname.c_str(), rd.seq.c_str(), q, l_seq, rd.regs, -1, flag, nullptr, 0, rg, cm), s += '\n';
			} else if (flag & GD_F_PAF_NO_HIT) gd_write_paf(s, R, rd.qname.c_str(), l_seq, rd.regs, -1, flag), s += '\n';
			continue;
		}
		for (int j = 0; j < nr; ++j) {
			if ((flag & GD_F_NO_PRINT_2ND) && rd.regs[j].id != rd.regs[j].parent) continue;
			const char *ds = rd.has_ds[j] ? rd.ds[j].c_str() : nullptr;
			const size_t dl = rd.has_ds[j] ? rd.ds[j].size() : 0;
			if (mode == "sam") gd_write_sam(s, R, rd.qname.c_str(), rd.seq.c_str(), q, l_seq, rd.regs, j, flag, ds, dl, rg, cm), s += '\n';
			else gd_write_paf(s, R, rd.qname.c_str(), l_seq, rd.regs, j, flag, ds, dl, cm), s += '\n';
		}
	}
	fwrite(s.data(), 1, s.size(), stdout);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: samopts_emul fmt|rg <file>\n"); return 2; }
	std::ifstream in(argv[2]);
	if (!in) { perror(argv[2]); return 2; }
	const std::string what = argv[1];
	if (what == "rg") return run_rg(in);
	if (what == "fmt") return run_fmt(in);
	return 2;
}
