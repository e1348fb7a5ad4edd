// What the emulators of the two accumulators (cov_emul.cpp, pile_emul.cpp) share: reading a file, the driver's walk over the records
// (csrc/bam_starts.h), and the statements both scatter kernels open with on a record -- the head, PASS 1 over the lanes in either order,
// the verdict (gdc_record_pass1 of csrc/cov.hip.h) -- with the bookkeeping of the call's first bad record.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "bam_starts.h"
#include "cov.h"

static bool slurp(const char *path, std::string &out)
{
	std::ifstream f(path, std::ios::binary);
	if (!f) { perror(path); return false; }
	std::stringstream ss;
	ss << f.rdbuf();
	out = ss.str();
	return true;
}

// the driver's walk: block_size alone.  0, or the exit status 3 with the reason on stderr
static int record_starts(const std::string &data, std::vector<uint64_t> &start)
{
	std::string why;
	if (gd_record_starts(data.data(), data.size(), start, why) == 0) return 0;
	fprintf(stderr, "%s\n", why.c_str());
	return 3;
}

// one wavefront on the record at buf + at: its head and PASS 1, the lanes 0..63 or (down) 63..0; returns the reason
static uint32_t record_pass1(const uint8_t *buf, uint64_t len, uint64_t at, uint32_t n_ref, const uint32_t *clen, bool down, GdcHead *H)
{
	const uint32_t head = gdc_head(buf, len, at, H);
	const uint8_t *rec = buf + at;
	uint64_t ref = 0, qry = 0;
	uint32_t bad_op = 0;
	if (!head)
		for (uint32_t i = 0; i < 64; ++i) {
			const uint32_t lane = down ? 63 - i : i;
			for (uint32_t k = lane; k < H->n_ops; k += 64) {
				uint32_t L, rl, ql;
				(void)gdc_op(rec, *H, k, &L, &rl, &ql, &bad_op);
				ref += rl, qry += ql;
			}
		}
	return gdc_decide(*H, head, n_ref, clen, ref, qry, bad_op);
}

// the kernels' atomicMin on the cell of the first bad record
static void note_bad(uint64_t *first_bad, uint64_t j, uint32_t reason)
{
	if (reason && (j << 8 | reason) < *first_bad) *first_bad = j << 8 | reason;
}
static void print_bad(uint64_t first_bad)
{
	if (first_bad != ~(uint64_t)0)
		printf("BAD %llu %u %s\n", (unsigned long long)(first_bad >> 8), (unsigned)(first_bad & 0xff), gdc_reason_text((uint32_t)(first_bad & 0xff)));
}
