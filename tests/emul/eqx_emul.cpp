// Stand-alone host run of what map_post_kernel<true> does per alignment: gdp_update_extra, then gdp_cigar_eqx on the sequences moved by
// the shifts (map_post.h), meant to be built with -fsanitize=address,undefined.  Every CIGAR sits in a heap block of exactly qlen + tlen
// words -- the size of its slot on the device -- and the two sequences in blocks of exactly their lengths, so the backwards in-place
// expansion and the eight-base loads cannot step outside without the sanitizer seeing it.
//   eqx_emul <file>      file: the text tests/eqx_ref.py:write_emul_input writes (record count; per record "n_cigar qlen tlen", the CIGAR
//                        words, the query codes, the target codes)
// The record bookkeeping of the host stages (map_host.h: gd_update_extra with is_eqx, on a vector that grows) runs on the same input and
// must give the same CIGAR (exit status 5 otherwise).
// Prints one rewritten CIGAR per record with the shifts, mlen and blen; exit status 0 when every record was read and processed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "map_host.h"

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: eqx_emul <file>\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) { perror(argv[1]); return 2; }
	long n_rec = 0;
	if (fscanf(f, "%ld", &n_rec) != 1) return 3;
	int8_t mat[25]; // the sr preset's matrix (a = 2, b = 8; SR/map.c:864-865)
	for (int i = 0; i < 25; ++i) mat[i] = (i / 5 == 4 || i % 5 == 4) ? 0 : (i / 5 == i % 5 ? 2 : -8);
	for (long r = 0; r < n_rec; ++r) {
		unsigned n, ql, tl;
		if (fscanf(f, "%u %u %u", &n, &ql, &tl) != 3 || n == 0 || n > ql + tl) return 3;
		uint32_t *cg = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)ql + tl));
		uint8_t *q = (uint8_t *)malloc(ql ? ql : 1), *t = (uint8_t *)malloc(tl ? tl : 1);
		unsigned v;
		for (unsigned i = 0; i < n; ++i) { if (fscanf(f, "%u", &v) != 1) return 3; cg[i] = v; }
		for (unsigned i = 0; i < ql; ++i) { if (fscanf(f, "%u", &v) != 1) return 3; q[i] = (uint8_t)v; }
		for (unsigned i = 0; i < tl; ++i) { if (fscanf(f, "%u", &v) != 1) return 3; t[i] = (uint8_t)v; }
		GdReg hr;
		hr.has_p = true, hr.cigar.assign(cg, cg + n);
		gd_update_extra(hr, q, t, mat, 12, 2, 0, 1);
		uint32_t nc = n;
		GdPostOut P;
		gdp_update_extra(cg, &nc, q, t, mat, 12, 2, 0, &P);
		const uint32_t n_fixed = nc;
		gdp_cigar_eqx(cg, &nc, q + P.qshift, t + P.tshift);
		if (nc > ql + tl || nc < n_fixed) return 4;
		if (hr.cigar.size() != nc || (nc && memcmp(hr.cigar.data(), cg, sizeof(uint32_t) * nc)) || hr.mlen != P.mlen || hr.blen != P.blen) return 5;
		for (uint32_t i = 0; i < nc; ++i) printf("%u%c", cg[i] >> 4, "MIDNSHP=XB"[cg[i] & 0xf]);
		printf("\t%d\t%d\t%d\t%d\n", P.qshift, P.tshift, P.mlen, P.blen);
		free(cg), free(q), free(t);
	}
	fclose(f);
	return 0;
}
