// CPU emulator of the BGZF writing side (csrc/bgzf_deflate.h: the statements of bgzf_deflate_kernel as loops over 64 lanes; csrc/bgzf_out.h:
// the stream writer without a device), built by tests/test_bgzf_deflate.py with -fsanitize=address,undefined, once as it is and once with
// -DGDD_LANES_DOWN (the lane loops run 63..0): both builds must write the same bytes.  Input and slot of every member are heap blocks of
// exactly their size, so a read or a write past either is an AddressSanitizer report.
//
//     bgzf_deflate_emul deflate IN OUT        IN cut every 65280 bytes, every member through the emulated kernel; the members and the
//                                             end-of-file member go to OUT.  Checked here for every member: zlib's raw inflate of the
//                                             stream gives the input back; the trailer's CRC32 is zlib's and ISIZE the length; BSIZE + 1
//                                             is the member's length, at most 65536; gd_bgzf_scan finds exactly these members; the
//                                             project's own decoder (gdz_inflate, emulated) returns GDZ_OK and the same bytes.  Prints
//                                             "member K in N out M type T maxdist D cut A B C" per member (T: the first block's BTYPE; D:
//                                             the longest distance among the tokens of its last block; A, B, C: the blocks in which
//                                             gdd_build_lengths had to cut the literal/length code, the distance code, the code-length
//                                             code to its limit, whether or not the block was then written with those codes) and
//                                             "ok members K bytes_in N bytes_out M".
//     bgzf_deflate_emul lengths MAXBITS F...  gdd_build_lengths on the frequencies F: prints the lengths
//     bgzf_deflate_emul writer IN OUT LEVEL THREADS OP...
//                                             the stream writer without a device on consecutive pieces of IN: OP is a number of bytes
//                                             to write or "f" for a flush; then close.  Prints the writer's statistics.
// Any difference ends the program with status 1.
#include <stdio.h>
#include <stdlib.h>
#include <fcntl.h>
#include <vector>
#include <string>
#include "bgzf.h"
#include "bgzf_inflate.h"
#include "bgzf_deflate.h"
#include "bgzf_out.h"

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

static GddLds *g_lds = new GddLds();
static GdzLds *g_zlds = new GdzLds();
static uint32_t g_maxdist = 0, g_cuts[3];

#define FAIL(...) do { printf("MISMATCH " __VA_ARGS__); printf("\n"); exit(1); } while (0)

// the kernel's body on one member: exact-size copy of the input, a slot of exactly 65536 bytes
static std::vector<unsigned char> emul_member(const unsigned char *in, uint32_t n)
{
	unsigned char *src = (unsigned char *)malloc(n ? n : 1);
	if (n) memcpy(src, in, n);
	unsigned char *slot = (unsigned char *)malloc(GDD_SLOT);
	memset(slot, 0xee, GDD_SLOT);
	memset((void *)g_lds, 0xa5, sizeof(GddLds)); // (nothing may depend on what local memory held)
	memset((void *)g_lds->tok, 0, sizeof(g_lds->tok)); // (... but the token buffer is read below, for the longest distance)
	uint32_t len = 0;
	g_cuts[0] = g_cuts[1] = g_cuts[2] = 0;
	const uint32_t rc = gdd_deflate(*g_lds, src, n, slot, &len, g_cuts);
	if (rc != GDD_OK) FAIL("gdd_deflate returns %u", rc);
	if (len < 28 || len > GDD_SLOT) FAIL("member of %u bytes", len);
	for (uint32_t k = (len + 3) / 4 * 4; k < GDD_SLOT; ++k) if (slot[k] != 0xee) FAIL("a write behind the member at %u", k);
	std::vector<unsigned char> m(slot, slot + len);
	free(slot), free(src);
	g_maxdist = 0; // of the tokens the buffer still holds: all of them for a member of one block
	for (uint32_t k = 0; k < GDD_TOK; ++k) if (g_lds->tok[k] >> 31) g_maxdist = std::max(g_maxdist, (g_lds->tok[k] & 32767u) + 1u);
	return m;
}

static void check_member(const std::vector<unsigned char> &m, const unsigned char *in, uint32_t n, size_t k)
{
	if (gd_bgzf_le16(m.data() + 16) + 1 != m.size()) FAIL("member %zu: BSIZE + 1 = %u, length %zu", k, gd_bgzf_le16(m.data() + 16) + 1, m.size());
	if (m.size() > 18u + 5u + n + 8u) FAIL("member %zu: %zu bytes, a stored one is %u", k, m.size(), 18u + 5u + n + 8u);
	const uint32_t crc = gd_bgzf_le32(m.data() + m.size() - 8), isize = gd_bgzf_le32(m.data() + m.size() - 4);
	if (isize != n) FAIL("member %zu: ISIZE %u, input %u", k, isize, n);
	if (crc != (uint32_t)(n ? crc32(crc32(0L, Z_NULL, 0), in, n) : crc32(0L, Z_NULL, 0))) FAIL("member %zu: CRC32 %08x is not zlib's", k, crc);
	std::vector<GdBgzfMember> tab;
	size_t inc = 0, bad = 0;
	std::string why;
	if (gd_bgzf_scan(m.data(), m.size(), tab, &inc, &bad, &why) != GD_BGZF_OK || inc != m.size() || tab.size() != 1) FAIL("member %zu: the scan refuses it: %s", k, why.c_str());
	if (tab[0].in_off != 18 || tab[0].in_len != m.size() - 26 || tab[0].isize != n || tab[0].crc != crc) FAIL("member %zu: the scan's table differs", k);
	// zlib's raw inflate: the whole stream, nothing behind it
	z_stream z;
	memset(&z, 0, sizeof(z));
	if (inflateInit2(&z, -15) != Z_OK) exit(2);
	std::vector<unsigned char> out((size_t)n + 1);
	z.next_in = const_cast<unsigned char *>(m.data() + 18), z.avail_in = (uInt)(m.size() - 26), z.next_out = out.data(), z.avail_out = n + 1;
	const int rc = inflate(&z, Z_FINISH);
	const size_t got = (size_t)n + 1 - z.avail_out, left = z.avail_in;
	inflateEnd(&z);
	if (rc != Z_STREAM_END || got != n || left != 0 || (n && memcmp(out.data(), in, n))) FAIL("member %zu: zlib's inflate: rc %d, %zu bytes of %u, %zu stream bytes left", k, rc, got, n, left);
	// the project's own decoder on exact-size copies
	unsigned char *src = (unsigned char *)malloc(m.size() - 26 ? m.size() - 26 : 1), *dst = (unsigned char *)malloc(n ? n : 1);
	memcpy(src, m.data() + 18, m.size() - 26);
	uint32_t out_len = 0;
	const uint32_t zrc = gdz_inflate(*g_zlds, src, (uint32_t)(m.size() - 26), dst, n, &out_len);
	if (zrc != GDZ_OK || out_len != n || (n && memcmp(dst, in, n))) FAIL("member %zu: gdz_inflate: %s, %u bytes of %u", k, gdz_strerror(zrc), out_len, n);
	free(src), free(dst);
}

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	const std::string cmd = argv[1];
	if (cmd == "deflate") {
		if (argc < 4) return 2;
		const std::vector<unsigned char> in = slurp(argv[2]);
		FILE *f = fopen(argv[3], "wb");
		if (!f) return 2;
		size_t k = 0, total = 0;
		for (size_t at = 0; at < in.size(); at += GDD_MAX_IN, ++k) {
			const uint32_t n = (uint32_t)std::min<size_t>(GDD_MAX_IN, in.size() - at);
			const std::vector<unsigned char> m = emul_member(in.data() + at, n);
			check_member(m, in.data() + at, n, k);
			printf("member %zu in %u out %zu type %u maxdist %u cut %u %u %u\n", k, n, m.size(), (m[18] >> 1) & 3u, g_maxdist, g_cuts[0], g_cuts[1], g_cuts[2]);
			fwrite(m.data(), 1, m.size(), f), total += m.size();
		}
		if (in.empty()) { // what gdiet_hip_bgzf_deflate does not write, but the kernel must handle: a member of no bytes
			const std::vector<unsigned char> m = emul_member(in.data(), 0);
			check_member(m, in.data(), 0, 0);
			printf("empty member out %zu type %u\n", m.size(), (m[18] >> 1) & 3u);
		}
		fwrite(GD_BGZF_EOF, 1, GD_BGZF_EOF_LEN, f);
		fclose(f);
		printf("ok members %zu bytes_in %zu bytes_out %zu\n", k, in.size(), total);
		return 0;
	}
	if (cmd == "lengths") {
		const uint32_t max_bits = (uint32_t)atoi(argv[2]), n = (uint32_t)(argc - 3);
		if (n > GDD_LITS) return 2;
		uint32_t *freq = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
		uint8_t *lens = (uint8_t *)malloc(n ? n : 1);
		for (uint32_t i = 0; i < n; ++i) freq[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10), lens[i] = 0xee;
		memset((void *)g_lds, 0xa5, sizeof(GddLds));
		gdd_build_lengths(freq, n, max_bits, lens, g_lds->build);
		for (uint32_t i = 0; i < n; ++i) printf("%u%c", lens[i], i + 1 < n ? ' ' : '\n');
		if (!n) printf("\n");
		free(freq), free(lens);
		return 0;
	}
	if (cmd == "writer") {
		if (argc < 6) return 2;
		const std::vector<unsigned char> in = slurp(argv[2]);
		GdBgzfOut w;
		w.fd = ::open(argv[3], O_WRONLY | O_CREAT | O_TRUNC, 0644);
		if (w.fd < 0) return 2;
		w.level = atoi(argv[4]), w.threads = atoi(argv[5]);
		size_t at = 0;
		for (int a = 6; a < argc; ++a) {
			if (!strcmp(argv[a], "f")) { if (w.flush()) { printf("write error: %s\n", w.msg.c_str()); return 3; } continue; }
			const size_t n = (size_t)atol(argv[a]);
			if (at + n > in.size()) return 2;
			unsigned char *p = (unsigned char *)malloc(n ? n : 1); // (an exact-size copy: the writer reads nothing behind what it is given)
			memcpy(p, in.data() + at, n);
			const int rc = w.write(p, n);
			free(p);
			if (rc) { printf("write error: %s\n", w.msg.c_str()); return 3; }
			at += n;
		}
		if (w.close()) { printf("write error: %s\n", w.msg.c_str()); return 3; }
		printf("ok members_device %lld members_host %lld bytes_in %lld bytes_out %lld\n", (long long)w.members_device, (long long)w.members_host, (long long)w.bytes_in, (long long)w.bytes_out);
		return 0;
	}
	return 2;
}
