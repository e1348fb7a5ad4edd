// CPU emulator of the BGZF route (csrc/bgzf.h, csrc/bgzf_inflate.h: the statements of bgzf_inflate_kernel as loops over 64 lanes), built
// with -fsanitize=address,undefined by tests/test_bgzf.py.  Every range the scan or the decoder is given is copied into a heap block of
// exactly its size first, so a read past its end is an AddressSanitizer report.
//
//     bgzf_emul scan FILE [N ...]             the member table of the first N bytes (default: all) of FILE, one line per member, then
//                                             "incomplete X" or "notbgzf X: why", then "route R" (what the reader would do with the file);
//                                             the same again for every further N
//     bgzf_emul decode FILE                   every member through the emulated kernel and through zlib's raw inflate: equal bytes and lengths
//     bgzf_emul trunc FILE                    every member cut at every length: the decoder must return (and never succeed where zlib fails)
//     bgzf_emul fuzz FILE SEED N              N single-bit and single-byte mutations of every member, likewise
//     bgzf_emul agree FILE                    every member, valid or not, likewise; prints "member K code C (its text) out N" per member: what
//                                             the decoder returned and the bytes it had produced by then
//     bgzf_emul reader BGZF PLAIN BLOCK CHUNK attached|host THREADS
//                                             the reader on BGZF (the emulated device inflating and parsing, or zlib on THREADS threads) hands
//                                             out the batches of the unattached reader on PLAIN; prints the BGZF statistics and the
//                                             number of blocks read.  THREADS < 0: one thread for the first batch, -THREADS from then on.  A read
//                                             error ends it with status 3 and "read error: MESSAGE".
// Any difference ends the program with status 1.
#define main fastx_dev_emul_main
#include "fastx_dev_emul.cpp" // EmulDevice: the device's parse passes as loops (and its checks against the sequential grammar)
#undef main
#include "bgzf.h"
#include "bgzf_inflate.h"
#include <random>

static std::vector<unsigned char> slurp(const char *path)
{
	FILE *f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
	std::vector<unsigned char> v;
	unsigned char buf[65536];
	for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
	fclose(f);
	return v;
}

static GdzLds *g_lds = new GdzLds(); // one wavefront's local memory

// the kernel's body on an exact-size copy of the stream, into an exact-size output at every alignment in turn
static uint32_t emul_inflate(const unsigned char *in, uint32_t in_len, uint32_t isize, std::vector<unsigned char> &out, uint32_t *out_len)
{
	static uint32_t turn = 0;
	const uint32_t shift = turn++ & 15u;
	unsigned char *src = (unsigned char *)malloc(in_len ? in_len : 1);
	memcpy(src, in, in_len);
	unsigned char *dst = (unsigned char *)malloc((size_t)shift + isize + (shift + isize ? 0 : 1)); // (16-byte aligned: the output starts `shift` behind that, and ends where the block ends)
	memset(dst, 0xee, shift);
	const uint32_t rc = gdz_inflate(*g_lds, src, in_len, dst + shift, isize, out_len);
	for (uint32_t k = 0; k < shift; ++k) if (dst[k] != 0xee) { printf("MISMATCH a write in front of the output\n"); exit(1); }
	out.assign(dst + shift, dst + shift + (rc == GDZ_OK ? *out_len : 0));
	free(dst), free(src);
	return rc;
}

static int zlib_inflate(const unsigned char *in, uint32_t in_len, uint32_t cap, std::vector<unsigned char> &out)
{
	z_stream z;
	memset(&z, 0, sizeof(z));
	if (inflateInit2(&z, -15) != Z_OK) exit(2);
	out.assign((size_t)cap + 1, 0);
	z.next_in = const_cast<unsigned char *>(in), z.avail_in = in_len, z.next_out = out.data(), z.avail_out = cap;
	const int rc = inflate(&z, Z_FINISH);
	out.resize(cap - z.avail_out);
	inflateEnd(&z);
	return rc;
}

// the decoder against zlib on one stream; strict: both must succeed.  Returns whether the stream was valid; code, produced: what the
// decoder returned and the bytes it had produced by then.
static bool compare(const unsigned char *in, uint32_t in_len, uint32_t isize, bool strict, const char *what, long k, uint32_t *code = nullptr, uint32_t *produced = nullptr)
{
	std::vector<unsigned char> got, want;
	uint32_t out_len = 0;
	const uint32_t rc = emul_inflate(in, in_len, isize, got, &out_len);
	if (code) *code = rc;
	if (produced) *produced = out_len;
	const int zrc = zlib_inflate(in, in_len, isize, want);
	const bool ok = rc == GDZ_OK, zok = zrc == Z_STREAM_END;
	if (out_len > isize) { printf("MISMATCH %s %ld: %u bytes into room for %u\n", what, k, out_len, isize); exit(1); }
	if (ok != zok) { printf("MISMATCH %s %ld: decoder says %u (%s), zlib says %d\n", what, k, rc, gdz_strerror(rc), zrc); exit(1); }
	if (ok && got != want) { printf("MISMATCH %s %ld: bytes differ (%zu vs %zu)\n", what, k, got.size(), want.size()); exit(1); }
	if (strict && !ok) { printf("MISMATCH %s %ld: a valid member is refused: %s\n", what, k, gdz_strerror(rc)); exit(1); }
	return ok;
}

static std::vector<GdBgzfMember> scan_all(const std::vector<unsigned char> &file)
{
	std::vector<GdBgzfMember> tab;
	size_t inc = 0, bad = 0;
	std::string why;
	if (gd_bgzf_scan(file.data(), file.size(), tab, &inc, &bad, &why) != GD_BGZF_OK || inc != file.size()) { printf("MISMATCH the input is not a series of whole members\n"); exit(1); }
	return tab;
}

struct BgzfEmulDevice : EmulDevice {
	int inflate(const unsigned char *raw, size_t raw_len, const GdBgzfMember *m, size_t n, unsigned char *dst, size_t dst_len, uint32_t *out_len, std::string &why) override
	{
		for (size_t i = 0; i < n; ++i) { // what the driver checks before it launches
			if (m[i].in_off + m[i].in_len > raw_len || m[i].out_off + m[i].isize > dst_len) { why = "a member outside its buffers"; return -1; }
			std::vector<unsigned char> out;
			const uint32_t rc = emul_inflate(raw + m[i].in_off, m[i].in_len, m[i].isize, out, &out_len[i]);
			if (rc != GDZ_OK) { why = std::string("BGZF member ") + std::to_string(i) + ": " + gdz_strerror(rc); return -2; }
			if (!out.empty()) memcpy(dst + m[i].out_off, out.data(), out.size());
		}
		return 0;
	}
};

static std::string bgzf_digest(const char *path, int mode, int threads, size_t block, int64_t chunk, long *n_out, long *batches, int64_t st[5])
{
	GdFastx *fx = gd_fastx_open(path);
	if (!fx) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
	fx->block_size = block, fx->n_threads = threads < 0 ? 1 : threads;
	if (mode == 1) fx->dev = std::make_shared<BgzfEmulDevice>();
	std::string d;
	long n = 0;
	*batches = 0;
	for (;;) {
		bool bad = false;
		const int k = fx->read_batch(chunk, true, true, false, &bad);
		if (k < 0) { printf("read error: %s\n", fx->io_msg.c_str()); gd_fastx_close(fx); exit(3); }
		if (k == 0 && !bad) break;
		fx->u_to_t_on_host();
		for (int i = 0; i < k; ++i) {
			d += fx->v_name[i], d += '\t', d += fx->v_comment[i] ? fx->v_comment[i] : "-", d += '\t', d += fx->v_seq[i], d += '\t';
			d += fx->v_qual[i] ? fx->v_qual[i] : "-", d += '\n';
		}
		d += bad ? "==bad==\n" : "==\n";
		n += k, ++*batches;
		if (threads < 0) fx->n_threads = -threads; // (what gdiet_hip_fastx_set_threads does, in mid-file)
	}
	st[4] = fx->n_blocks;
	st[0] = fx->bz_members_device, st[1] = fx->bz_members_host, st[2] = fx->bz_bytes_in, st[3] = fx->bz_bytes_out;
	gd_fastx_close(fx);
	*n_out = n;
	return d;
}

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	const std::string cmd = argv[1];
	if (cmd == "scan") {
		std::vector<unsigned char> file = slurp(argv[2]);
		for (int a = 3; a == 3 || a < argc; ++a) {
		const size_t n = argc > 3 ? std::min<size_t>(file.size(), (size_t)atol(argv[a])) : file.size();
		unsigned char *p = (unsigned char *)malloc(n ? n : 1);
		memcpy(p, file.data(), n);
		std::vector<GdBgzfMember> tab;
		size_t inc = 0, bad = 0;
		std::string why;
		const int rc = gd_bgzf_scan(p, n, tab, &inc, &bad, &why);
		for (const GdBgzfMember &m : tab) printf("member %llu %u %llu %u %u\n", (unsigned long long)m.in_off, m.in_len, (unsigned long long)m.out_off, m.isize, m.crc);
		if (rc == GD_BGZF_OK) printf("incomplete %zu\n", inc);
		else printf("notbgzf %zu: %s\n", bad, why.c_str());
		free(p);
		const int fd = ::open(argv[2], O_RDONLY);
		printf("route %d\n", fd >= 0 && gd_fastx_takes_bgzf_route(fd) ? 1 : 0);
		if (fd >= 0) ::close(fd);
		}
		return 0;
	}
	if (cmd == "decode" || cmd == "trunc" || cmd == "fuzz" || cmd == "agree") {
		const std::vector<unsigned char> file = slurp(argv[2]);
		const std::vector<GdBgzfMember> tab = scan_all(file);
		long n_valid = 0, n_tried = 0;
		size_t bytes = 0;
		if (cmd == "decode")
			for (size_t k = 0; k < tab.size(); ++k) compare(file.data() + tab[k].in_off, tab[k].in_len, tab[k].isize, true, "member", (long)k), bytes += tab[k].isize, ++n_tried, ++n_valid;
		else if (cmd == "agree")
			for (size_t k = 0; k < tab.size(); ++k) {
				uint32_t code = 0, produced = 0;
				n_valid += compare(file.data() + tab[k].in_off, tab[k].in_len, tab[k].isize, false, "member", (long)k, &code, &produced), ++n_tried;
				printf("member %zu code %u (%s) out %u\n", k, code, gdz_strerror(code), produced);
			}
		else if (cmd == "trunc")
			for (size_t k = 0; k < tab.size(); ++k)
				for (uint32_t len = 0; len < tab[k].in_len; ++len) n_valid += compare(file.data() + tab[k].in_off, len, tab[k].isize, false, "truncation of member", (long)k), ++n_tried;
		else {
			if (argc < 5) return 2;
			std::mt19937_64 rng((uint64_t)atol(argv[3]));
			const long n = atol(argv[4]);
			for (size_t k = 0; k < tab.size(); ++k) {
				std::vector<unsigned char> m(file.begin() + (long)tab[k].in_off, file.begin() + (long)(tab[k].in_off + tab[k].in_len));
				if (m.empty()) continue;
				for (long t = 0; t < n; ++t) {
					const size_t at = (size_t)(rng() % m.size());
					const unsigned char old = m[at];
					if (t & 1) m[at] = (unsigned char)(rng() & 255); else m[at] ^= (unsigned char)(1u << (rng() & 7));
					n_valid += compare(m.data(), (uint32_t)m.size(), tab[k].isize, false, "mutation of member", (long)k), ++n_tried;
					m[at] = old;
				}
			}
		}
		printf("ok members %zu streams %ld valid %ld bytes %zu\n", tab.size(), n_tried, n_valid, bytes);
		return 0;
	}
	if (cmd == "reader") {
		if (argc < 8) return 2;
		const size_t block = (size_t)atol(argv[4]);
		const int64_t chunk = atol(argv[5]);
		const int mode = !strcmp(argv[6], "attached") ? 1 : 0, threads = atoi(argv[7]);
		long n0 = 0, n1 = 0, b0 = 0, b1 = 0;
		int64_t s0[5], s1[5];
		const std::string want = bgzf_digest(argv[3], 0, 1, block, chunk, &n0, &b0, s0);
		const std::string got = bgzf_digest(argv[2], mode, threads, block, chunk, &n1, &b1, s1);
		if (want != got) { printf("MISMATCH the reader on the BGZF file and on the plain file differ (%ld vs %ld records)\n", n1, n0); return 1; }
		if (s0[0] || s0[1] || s0[2] || s0[3]) { printf("MISMATCH BGZF statistics of a plain file\n"); return 1; }
		printf("ok records %ld batches %ld members_device %lld members_host %lld bytes_in %lld bytes_out %lld blocks %lld\n", n1, b1, (long long)s1[0], (long long)s1[1], (long long)s1[2],
		       (long long)s1[3], (long long)s1[4]);
		return 0;
	}
	return 2;
}
