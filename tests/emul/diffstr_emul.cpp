// Host emulator of the difference-string kernel: map_diffstr.h compiled for the host, gdd_record run on 64 emulated lanes exactly as
// map_diffstr_kernel runs it -- a count pass (out == nullptr) that gives every record's length, an exclusive scan, a write pass.
// A lane is run from the first statement to the last before the next one starts.  That is possible because the loop structure of
// gdd_record depends on the record and its CIGAR only: every lane meets the same sequence of ballots.  So a record is run twice per pass:
// a dry round in which every lane contributes its bit to the k-th ballot (stores switched off, ballots answered with 0), then the
// real round in which the k-th ballot returns the collected mask.
// What the device names scalar with readfirstlane (uni) must really be wave-uniform: lane 0 of the dry round records every value passed to
// uni, and every other lane of both rounds must pass the same value at the same place.
// Checked on the way: all 64 lanes return the same length; the write pass returns the counted length; every byte of a record's slice
// is stored exactly once and no store falls outside it.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "map_diffstr.h"

namespace {
struct EmuWave {
	unsigned lane = 0;
	bool dry = false;
	std::vector<uint64_t> *masks = nullptr;
	size_t k = 0;
	std::vector<uint32_t> *unis = nullptr; // the values lane 0 passed to uni in the dry round
	size_t ku = 0;
	char *lo = nullptr, *hi = nullptr; // the record's slice
	uint8_t *seen = nullptr;           // per byte of the slice: times stored
	int *err = nullptr;
	uint64_t ballot(bool p)
	{
		if (dry) {
			if (masks->size() <= k) masks->push_back(0);
			if (p) (*masks)[k] |= 1ull << lane;
			++k;
			return 0;
		}
		if (k >= masks->size()) { *err = -10; return 0; } // a ballot the dry round did not meet
		return (*masks)[k++];
	}
	unsigned prefix(uint64_t m) const { return (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1)); }
	uint32_t uni(uint32_t v)
	{
		if (dry && lane == 0) { unis->push_back(v); ++ku; return v; }
		if (ku >= unis->size() || (*unis)[ku] != v) { *err = -16; return v; } // not wave-uniform: the device would take lane 0's value
		return (*unis)[ku++];
	}
	void put(char *out, uint32_t at, char c)
	{
		if (dry) return;
		char *p = out + at;
		if (p < lo || p >= hi) { *err = -11; return; }
		if (seen[p - lo]++) *err = -12;
		*p = c;
	}
};
} // namespace

// off[n + 1]: written by the count pass (text == nullptr), read by the write pass.  Returns 0, or -10 ballots out of step, -11 a store
// outside the slice, -12 a byte stored twice, -13 a byte never stored, -14 lanes disagree on the length, -15 write pass != count pass, -16 a value passed to uni differs between lanes
extern "C" int64_t diffstr_emul(int64_t n, const GddRec *rec, const uint32_t *cig, const uint8_t *reads, const int64_t *roff, const uint32_t *S,
                                const uint64_t *seq_off, const uint32_t *seq_len, int mode, int qstrand, int64_t *off, char *text)
{
	GddIn in = {rec, cig, reads, roff, S, seq_off, seq_len, qstrand};
	int err = 0;
	std::vector<uint64_t> masks;
	std::vector<uint32_t> unis;
	std::vector<uint8_t> seen;
	if (!text) off[0] = 0;
	for (int64_t i = 0; i < n; ++i) {
		masks.clear(), unis.clear();
		char *out = text ? text + off[i] : nullptr;
		const int64_t want = text ? off[i + 1] - off[i] : 0;
		seen.assign((size_t)want, 0);
		int64_t len0 = -1;
		for (int round = 0; round < 2; ++round)
			for (unsigned lane = 0; lane < 64; ++lane) {
				EmuWave w;
				w.lane = lane, w.dry = round == 0, w.masks = &masks, w.unis = &unis, w.lo = out, w.hi = out + want, w.seen = seen.data(), w.err = &err;
				const int64_t len = mode == GDD_MD ? gdd_record<GDD_MD>(w, in, i, out) : mode == GDD_CS ? gdd_record<GDD_CS>(w, in, i, out) : gdd_record<GDD_CS_LONG>(w, in, i, out);
				if (round == 1) {
					if (len0 < 0) len0 = len;
					if (len != len0) return -14;
					if (w.k != masks.size()) return -10;
				}
				if (err) return err;
			}
		if (!text) off[i + 1] = off[i] + len0;
		else {
			if (len0 != want) return -15;
			for (int64_t b = 0; b < want; ++b) if (seen[(size_t)b] != 1) return -13;
		}
	}
	return 0;
}

// the host check of the driver (gdd_check_record) over a record table: index of the first record it refuses, -1 if none
extern "C" int64_t diffstr_check(int64_t n, const GddRec *rec, const uint32_t *cig, const int64_t *roff, const uint32_t *seq_len, uint32_t n_seq, int cs)
{
	for (int64_t i = 0; i < n; ++i) {
		const GddRec &r = rec[i];
		if (r.rid < 0 || (uint32_t)r.rid >= n_seq) return i;
		if (gdd_check_record(r, cig + r.cig_off, roff[r.read + 1] - roff[r.read], seq_len[r.rid], cs)) return i;
	}
	return -1;
}
