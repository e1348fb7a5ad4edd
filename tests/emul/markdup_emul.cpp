// Stand-alone host run of duplicate marking, meant to be built with -fsanitize=address,undefined: the statements of dup_key_kernel,
// dup_decide_kernel and dup_apply_kernel (bam_markdup.h) as loops over records and over 64 lanes, on exact-size copies of every buffer,
// so that a read or a store outside them is a sanitizer report.  std::stable_sort stands for hipCUB's two radix sorts, a loop over the
// lanes for the ballot and the wave sums.  The sorter's host executor, the loops of the sort pass and the resident deflater are those of
// bam_sort_emul.cpp, taken in whole (its main is renamed); the executor here adds the four duplicate methods to them.
//
//   markdup_emul mark <in.records> <out.records>
//       the kernel-level boundary over one buffer: every record's entry is computed with the lanes running 0..63 and 63..0 and with the
//       buffer at each of the four alignments mod 4 (the QUAL sum takes dwords from the first 4-byte boundary on), all eight must agree.
//       Prints "examined eligible duplicates max_group".
//   markdup_emul sorter <in.records> <records per batch> <run bytes> <chunk bytes> <tmp dir> <header file> <device 0|1> <out.bam> <markdup 0|1>
//       GdqSorter over the host executor with marking on or off.  Prints the sorter's six counts and the four duplicate counts.
// Exit status 0; 2 usage / file errors; 3 malformed or bad records (the reason goes to stderr); 4 open refused; 5 add or close failed;
// 6 set_markdup behind an add was NOT refused; 7 two variants of one pass differ.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <memory>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>
#define main bam_sort_emul_main
#include "bam_sort_emul.cpp"
#undef main
#include "bam_markdup.h"
#include "bam_starts.h"

// the statements of dup_key_kernel for the record at buf + at; the lanes run 63..0 if down
static uint32_t key_record(const uint8_t *buf, uint64_t len, uint64_t at, bool down, uint64_t *key, uint32_t *score)
{
	GdcHead H;
	uint32_t reason = gdc_head(buf, len, at, &H);
	const uint8_t *rec = buf + at;
	*key = GDM_SENTINEL, *score = 0;
	if (reason || !gdm_eligible(H.flag, H.refID, H.pos)) return reason;
	const uint32_t rev = H.flag >> 4 & 1u;
	uint32_t first = H.n_ops, last1 = 0, bad_op = 0;
	uint64_t ref = 0, clip = 0;
	for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
		uint64_t m = 0;
		for (uint32_t i = 0; i < 64; ++i) {
			const uint32_t lane = down ? 63 - i : i;
			if (gdm_round_lane(rec, H, b0 + lane, &ref, &bad_op)) m |= (uint64_t)1 << lane;
		}
		gdm_round_mask(m, b0, H.n_ops, &first, &last1);
	}
	for (uint32_t i = 0; i < 64; ++i) clip += gdm_clip_lane(rec, H, rev ? last1 : 0u, rev ? H.n_ops : first, down ? 63 - i : i);
	reason = bad_op ? (uint32_t)GDC_BAD_OP : gdm_key(H.refID, H.pos, rev, ref, clip, key);
	if (reason) { *key = GDM_SENTINEL; return reason; }
	for (uint32_t i = 0; i < 64; ++i) *score += gdm_qual_share(rec, H, down ? 63 - i : i);
	return 0;
}

// the key pass over data[0, n) whose records start at start[k]: eight variants that must agree.  0, 3 (why), 7
static int key_pass(const std::string &data, const std::vector<uint64_t> &start, std::vector<uint64_t> &key, std::vector<uint32_t> &score, std::string &why)
{
	const size_t n = start.size();
	key.assign(n, 0), score.assign(n, 0);
	for (int variant = 0; variant < 8; ++variant) {
		const int shift = variant >> 1, down = variant & 1;
		std::unique_ptr<uint8_t[]> buf(new uint8_t[data.size() + shift]); // (new[] returns 16-byte aligned memory: shift is the alignment mod 4; the buffer ends where the records end)
		uint8_t *b = buf.get() + shift;
		if (!data.empty()) memcpy(b, data.data(), data.size());
		for (size_t k = 0; k < n; ++k) {
			uint64_t kk;
			uint32_t sc;
			const uint32_t reason = key_record(b, data.size(), start[k], down != 0, &kk, &sc);
			if (reason) { why = "record " + std::to_string(k) + " of the buffer: " + gdm_reason_text(reason); return 3; }
			if (variant == 0) key[k] = kk, score[k] = sc;
			else if (key[k] != kk || score[k] != sc) return 7;
		}
	}
	return 0;
}

// the decision over entries in output order: the bitmap by place and the counts
static void decide(const std::vector<uint64_t> &key, const std::vector<uint32_t> &score, std::vector<uint32_t> &bitmap, GdmStats *st)
{
	const size_t n = key.size();
	std::vector<uint32_t> idx(n);
	std::iota(idx.begin(), idx.end(), 0u);
	std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return score[a] > score[b]; });
	std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
	std::unique_ptr<uint64_t[]> skey(new uint64_t[n + 1]);
	for (size_t i = 0; i < n; ++i) skey[i] = key[idx[i]];
	bitmap.assign((n + 31) / 32 + 1, 0u);
	*st = GdmStats();
	st->examined = (int64_t)n;
	for (size_t i = 0; i < n; ++i) {
		const bool elig = skey[i] != GDM_SENTINEL, dup = gdm_is_dup(skey.get(), i);
		if (dup) bitmap[idx[i] >> 5] |= 1u << (idx[i] & 31u), ++st->duplicates;
		if (elig) ++st->eligible;
		if (elig && !dup) st->max_group = std::max<int64_t>(st->max_group, (int64_t)(gdm_group_end(skey.get(), n, i) - i));
	}
}

static int run_mark(const char *in_path, const char *out_path)
{
	std::string data, why;
	if (!read_file(in_path, data)) return 2;
	std::vector<uint64_t> start;
	if (gd_record_starts(data.data(), data.size(), start, why)) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
	std::vector<uint64_t> key;
	std::vector<uint32_t> score, bitmap;
	const int rc = key_pass(data, start, key, score, why);
	if (rc) { fprintf(stderr, "%s\n", why.c_str()); return rc; }
	GdmStats st;
	decide(key, score, bitmap, &st);
	const auto out = exact(data);
	for (size_t k = 0; k < start.size(); ++k)
		if (start[k] <= data.size() && data.size() - start[k] >= 20) (void)gdm_apply(out.get() + start[k], gdm_bit(bitmap.data(), k));
	printf("%lld %lld %lld %lld\n", (long long)st.examined, (long long)st.eligible, (long long)st.duplicates, (long long)st.max_group);
	return write_file(out_path, out.get(), data.size()) ? 0 : 2;
}

// ---- the sorter's host executor with the four duplicate methods ----------------------------------------------------------------------------
struct DupEx : HostEx {
	size_t fl = 0; // the resident result is res = [front of fl bytes | records]
	int sort_run(const uint64_t *start, uint64_t n, uint64_t bytes, const uint8_t *front, size_t front_len, std::string &why)
	{
		fl = front_len;
		return HostEx::sort_run(start, n, bytes, front, front_len, why);
	}
	int gather(const uint8_t *side, uint64_t side_len, const uint64_t *src, const uint64_t *psize, const uint64_t *dst, uint64_t n, uint64_t bytes, const uint8_t *front, size_t front_len,
	           std::string &why)
	{
		fl = front_len;
		return HostEx::gather(side, side_len, src, psize, dst, n, bytes, front, front_len, why);
	}
	int dup_keys(uint64_t n, uint64_t *key, uint32_t *score, std::string &why)
	{
		if (n != rows.size()) { why = "another number of rows"; return -1; }
		std::vector<uint64_t> start, k;
		std::vector<uint32_t> s;
		for (const GdsRow &r : rows) start.push_back(r.out);
		if (key_pass(res.substr(fl), start, k, s, why)) { if (why.empty()) why = "two variants of the key pass differ"; return -1; }
		std::copy(k.begin(), k.end(), key), std::copy(s.begin(), s.end(), score);
		return 0;
	}
	int dup_decide(const uint64_t *key, const uint32_t *score, uint64_t n, uint32_t *bitmap, GdmStats *st, std::string &)
	{
		std::vector<uint32_t> bm;
		decide(std::vector<uint64_t>(key, key + n), std::vector<uint32_t>(score, score + n), bm, st);
		std::copy(bm.begin(), bm.begin() + (size_t)((n + 31) / 32), bitmap);
		return 0;
	}
	int dup_apply(const uint32_t *bitmap, uint32_t bit0, uint64_t n, std::string &why)
	{
		if (n != rows.size()) { why = "another number of rows"; return -1; }
		const std::unique_ptr<uint32_t[]> bm(new uint32_t[(size_t)((bit0 + n + 31) / 32)]); // exactly the words the slice needs
		std::copy(bitmap, bitmap + (size_t)((bit0 + n + 31) / 32), bm.get());
		const auto recs = exact(res.substr(fl));
		const uint64_t len = res.size() - fl;
		for (uint64_t k = 0; k < n; ++k) {
			const uint64_t at = rows[(size_t)k].out;
			if (at > len || len - at < 20) continue;
			rows[(size_t)k].flag = (uint16_t)gdm_apply(recs.get() + at, gdm_bit(bm.get(), (uint64_t)bit0 + k));
		}
		res.replace(fl, (size_t)len, (const char *)recs.get(), (size_t)len);
		return 0;
	}
	int dup_mark_resident(uint64_t n, GdmStats *st, std::string &why)
	{
		std::vector<uint64_t> key((size_t)n);
		std::vector<uint32_t> score((size_t)n), bitmap((size_t)((n + 31) / 32) + 1);
		*st = GdmStats();
		if (n == 0) return 0;
		if (dup_keys(n, key.data(), score.data(), why) || dup_decide(key.data(), score.data(), n, bitmap.data(), st, why)) return -1;
		return dup_apply(bitmap.data(), 0, n, why);
	}
};
static_assert(GdqHasDup<DupEx>::value && !GdqHasDup<HostEx>::value, "the trait tells the two executors apart");

static int run_dup_sorter(const char *in_path, uint64_t per_batch, uint64_t run_bytes, uint64_t chunk_bytes, const char *tmp, const char *header_path, bool device, const char *out_path,
                          bool markdup)
{
	std::string data, header, why;
	if (!read_file(in_path, data) || !read_file(header_path, header) || per_batch == 0) return 2;
	std::vector<uint64_t> start;
	if (gd_record_starts(data.data(), data.size(), start, why)) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
	start.push_back(data.size());
	{ // the executor without the methods refuses the option, and sorts on
		GdqSorter<HostEx> plain;
		if (plain.set_markdup(true) == 0 || plain.set_markdup(false) != 0) return 6;
	}
	GdqSorter<DupEx> q;
	if (q.open(out_path, (const uint8_t *)header.data(), header.size(), device, 1, 2, run_bytes, chunk_bytes, tmp, true,
	           device ? std::shared_ptr<GdBgzfDeflater>(std::make_shared<HostResidentDeflater>()) : std::shared_ptr<GdBgzfDeflater>())) {
		fprintf(stderr, "%s\n", q.msg.c_str());
		(void)q.close();
		return 4;
	}
	if (q.set_markdup(markdup)) return 5;
	int rc = 0;
	for (size_t k = 0; k + 1 < start.size() && !rc; k += per_batch) {
		const size_t k1 = std::min(start.size() - 1, k + (size_t)per_batch);
		const std::string batch = data.substr(start[k], start[k1] - start[k]);
		std::vector<uint64_t> rec_out;
		for (size_t i = k; i < k1; ++i) rec_out.push_back(start[i] - start[k]);
		rc = q.add(&batch, batch.size(), rec_out.data(), rec_out.size());
		if (!rc && q.set_markdup(!markdup) == 0) return 6; // behind an add the choice is closed
	}
	if (q.close() || rc) { fprintf(stderr, "%s\n", q.msg.c_str()); return 5; }
	const GdqStats &s = q.st;
	printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)s.records, (long long)s.runs, (long long)s.spooled_bytes, (long long)s.chunks, (long long)s.members,
	       (long long)s.n_no_coor, (long long)q.dup.examined, (long long)q.dup.eligible, (long long)q.dup.duplicates, (long long)q.dup.max_group);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "mark" && argc == 4) return run_mark(argv[2], argv[3]);
	if (mode == "sorter" && argc == 11)
		return run_dup_sorter(argv[2], strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10), argv[6], argv[7], argv[8][0] == '1', argv[9],
		                      argv[10][0] == '1');
	fprintf(stderr, "usage: markdup_emul mark <in> <out> | sorter <in> <records per batch> <run bytes> <chunk bytes> <tmp dir> <header> <device> <out.bam> <markdup>\n");
	return 2;
}
