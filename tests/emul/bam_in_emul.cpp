// Stand-alone host run of BAM input, meant to be built with -fsanitize=address,undefined: the walk (bam_in.h: gdi_walk), the statements of
// bam_unpack_kernel (gdi_unpack) as loops over 64 lanes on exact-size copies of the records and of the text, so that a read or a store
// outside them is a sanitizer report, and the host grammar inside a real GdFastx (fastx_reader.h).
//
//   bam_in_emul unpack <records> <with_qual> <out>
//        <records> holds whole uncompressed alignment records (no header).  Every row is unpacked twice, with the lanes running 0..63 and
//        63..0.  <out>: "<n> <text_len>\n", then n x 4 int64 offsets (name and aux fields in the records, -1: no aux field; seq and qual
//        in the text, -1: no quality), n int32 lengths, and the text -- what gdiet_hip_bam_in_unpack returns.
//   bam_in_emul read <path> <chunk_size> <with_qual> <with_comment> <frag_mode> <threads> <out>
//        the file through gd_fastx_open / read_batch.  <out>: per batch "B <n> <truncated>\n" and per read the four fields name, comment,
//        seq, qual, each as "<length>\n<bytes>\n" (-1: NULL); at the end "E <0 | -1> <message>\n" and "S <host> <device> <format>\n".
//   bam_in_emul mutate <path> <count> <seed> <scratch file> <with_comment>
//        <count> copies of the file with one byte changed each, read to the end as above; prints how they ended.
// Exit status 0; 2 usage / open errors; 5 a malformed record or a range that ends inside one (the message goes to stderr); 7 the two lane
// orders differ or a byte of the text was left unwritten.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "fastx_reader.h"

static bool slurp(const char *path, std::string &out)
{
	std::ifstream f(path, std::ios::binary);
	if (!f) return false;
	std::stringstream ss;
	ss << f.rdbuf();
	out = ss.str();
	return true;
}

static int unpack(const char *path, bool with_qual, const char *out_path)
{
	std::string in;
	if (!slurp(path, in)) return 2;
	std::unique_ptr<uint8_t[]> recs(new uint8_t[in.size()]); // exact size
	memcpy(recs.get(), in.data(), in.size());
	GdiWalk W;
	gdi_walk(recs.get(), 0, in.size(), with_qual, false, 0, 0, W);
	if (W.bad) { fprintf(stderr, "%s\n", W.msg.c_str()); return 5; }
	if (W.pos != in.size()) { fprintf(stderr, "offset %zu: the range ends inside a record\n", W.pos); return 5; }
	if (!gdi_rows_inside(W.rows.data(), W.rows.size(), in.size(), W.text_len)) return 7;
	std::string run[2];
	for (int down = 0; down < 2; ++down) {
		std::unique_ptr<uint8_t[]> text(new uint8_t[W.text_len]);
		for (uint64_t k = 0; k < W.text_len; ++k) text[k] = down ? 0x5A : 0xA5; // (a byte no lane stores differs between the two runs)
		for (const GdiRow &r : W.rows)
			for (int l = 0; l < 64; ++l) gdi_unpack(r, recs.get(), text.get(), (uint32_t)(down ? 63 - l : l), 64);
		for (const GdiRow &r : W.rows) {
			const uint64_t n = ((uint64_t)r.l_seq + 1) * ((r.flags & GDI_NOQUAL) ? 1 : 2);
			if (r.dst_end - r.dst != n) return 7;
			if (text[r.dst + r.l_seq] != 0 || text[r.dst_end - 1] != 0) return 7;
			for (uint64_t k = 0; k < r.l_seq; ++k) if (!memchr("=ACMGRSVTWYHKDBN", text[r.dst + k], 16)) return 7;
		}
		run[down].assign((const char *)text.get(), (size_t)W.text_len);
	}
	if (run[0] != run[1]) return 7;
	std::ofstream o(out_path, std::ios::binary);
	if (!o) return 2;
	o << W.rows.size() << " " << W.text_len << "\n";
	for (size_t k = 0; k < W.rows.size(); ++k) {
		const GdiRow &R = W.rows[k];
		const int64_t off[4] = {(int64_t)W.host[k].name_off, W.host[k].aux_len ? (int64_t)W.host[k].aux_off : -1, (int64_t)R.dst,
		                        (R.flags & GDI_NOQUAL) ? -1 : (int64_t)(R.dst + R.l_seq + 1)};
		o.write((const char *)off, sizeof(off));
	}
	for (const GdiRow &R : W.rows) {
		const int32_t l = (int32_t)R.l_seq;
		o.write((const char *)&l, 4);
	}
	o << run[0];
	return 0;
}

static void put(std::ostream &o, const char *s)
{
	if (!s) { o << "-1\n"; return; }
	const size_t l = strlen(s);
	o << l << "\n";
	o.write(s, (std::streamsize)l);
	o << "\n";
}

// the whole file, batch by batch; returns the last read_batch's value (0 at the end of the input, -1 after a read error)
static int read_all(GdFastx *fx, int64_t chunk, bool wq, bool wc, bool frag, std::ostream *o, long *n_reads, long *n_trunc)
{
	for (;;) {
		bool bad = false;
		const int n = fx->read_batch(chunk, wq, wc, frag, &bad);
		if (n < 0) return n;
		if (n == 0 && !bad) return 0;
		if (o) *o << "B " << n << " " << (bad ? 1 : 0) << "\n";
		for (int i = 0; i < n; ++i) {
			if (fx->format == 1 && (size_t)fx->v_len[i] != strlen(fx->v_seq[i])) abort(); // (a BAM sequence holds letters only: no NUL inside)
			if (o) put(*o, fx->v_name[i]), put(*o, fx->v_comment[i]), put(*o, fx->v_seq[i]), put(*o, fx->v_qual[i]);
		}
		*n_reads += n, *n_trunc += bad ? 1 : 0;
	}
}

static int read_file(char **a)
{
	GdFastx *fx = gd_fastx_open(a[0]);
	if (!fx) return 2;
	fx->n_threads = atoi(a[5]);
	std::ofstream o(a[6], std::ios::binary);
	if (!o) return 2;
	long nr = 0, nt = 0;
	const int rc = read_all(fx, atoll(a[1]), atoi(a[2]) != 0, atoi(a[3]) != 0, atoi(a[4]) != 0, &o, &nr, &nt);
	o << "E " << rc << " " << fx->io_msg << "\n";
	o << "S " << fx->n_rec_host << " " << fx->n_rec_device << " " << fx->format << "\n";
	gd_fastx_close(fx);
	return 0;
}

static int mutate(char **a)
{
	std::string in;
	if (!slurp(a[0], in) || in.empty()) return 2;
	const long count = atol(a[1]);
	uint64_t x = (uint64_t)atoll(a[2]) * 2654435761u + 88172645463325252ull;
	auto rnd = [&]() { x ^= x << 13, x ^= x >> 7, x ^= x << 17; return x; };
	long ended[3] = {0, 0, 0}, reads = 0; // clean, truncated, read error
	for (long k = 0; k < count; ++k) {
		std::string m = in;
		const size_t at = (size_t)(rnd() % m.size());
		m[at] = (char)(m[at] ^ (1 + rnd() % 255));
		{
			std::ofstream o(a[3], std::ios::binary);
			if (!o) return 2;
			o.write(m.data(), (std::streamsize)m.size());
		}
		GdFastx *fx = gd_fastx_open(a[3]);
		if (!fx) return 2;
		fx->n_threads = 1 + (int)(k % 3);
		long nr = 0, nt = 0;
		const int rc = read_all(fx, 1000, true, atoi(a[4]) != 0, false, nullptr, &nr, &nt);
		++ended[rc < 0 ? 2 : nt ? 1 : 0], reads += nr;
		gd_fastx_close(fx);
	}
	printf("%ld clean, %ld truncated, %ld read errors, %ld reads\n", ended[0], ended[1], ended[2], reads);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "unpack" && argc == 5) return unpack(argv[2], atoi(argv[3]) != 0, argv[4]);
	if (mode == "read" && argc == 9) return read_file(argv + 2);
	if (mode == "mutate" && argc == 7) return mutate(argv + 2);
	fprintf(stderr, "usage: bam_in_emul unpack <records> <with_qual> <out> | read <path> <chunk> <with_qual> <with_comment> <frag> <threads> <out> | mutate <path> <count> <seed> <scratch> <with_comment>\n");
	return 2;
}
