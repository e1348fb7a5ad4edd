// The walk over a host buffer of whole uncompressed BAM records that the accumulators' add_bam calls make (accum_driver.hip.h) and the
// emulators of their kernels repeat (tests/emul/record_emul.h).  No HIP in here.
#pragma once
#include <string>
#include <vector>
#include "bam_sort.h"

// The starts of the records recs[0, len): nothing but block_size is looked at here, the kernels validate the rest.  0, or -1 with why:
// nothing was seen
static inline int gd_record_starts(const void *recs, size_t len, std::vector<uint64_t> &start, std::string &why)
{
	const uint8_t *b = (const uint8_t *)recs;
	size_t pos = 0;
	while (len - pos >= 4) {
		const int32_t bs = (int32_t)gds_le32(b + pos);
		if (bs < 32) {
			why = "BAM record " + std::to_string(start.size()) + " at offset " + std::to_string(pos) + ": a block_size of " + std::to_string(bs) + ", below the 32 fixed bytes";
			return -1;
		}
		if (len - pos - 4 < (size_t)bs) break;
		start.push_back(pos);
		pos += 4 + (size_t)bs;
	}
	if (pos != len) { why = "offset " + std::to_string(pos) + ": the range ends inside a record"; return -1; }
	if (start.size() > 0x7fffffffull) { why = "2^31 records or more in one call"; return -1; }
	return 0;
}
