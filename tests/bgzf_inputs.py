"""inputs of the BGZF tests (tests/test_bgzf.py on the CPU emulator, tests/test_bgzf_gpu.py on the GPU): a BGZF writer, the member matrix
(every compression strategy crossed with every kind of content) and a few hand-assembled deflate streams from a bit writer.
tools/make_bgzf.py is a thin command line around the writer."""
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_MEMBER_BYTES = 65280  # bgzip's own block size; level 0 on random bytes adds 36 and still fits BSIZE


def member_of_stream(deflate, data, extra_front=b""):
    """one BGZF member around a finished raw deflate stream of `data`; extra_front: other subfields in front of BC"""
    extra = extra_front + b"BC" + struct.pack("<H", 2)
    xlen = len(extra) + 2
    total = 12 + xlen + len(deflate) + 8
    assert total <= 65536, total
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", xlen) + extra + struct.pack("<H", total - 1) + deflate +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, extra_front=b""):
    return member_of_stream(deflate_raw(data, level, strategy, flush_at), data, extra_front)


def members_of(data, member_bytes=MAX_MEMBER_BYTES, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """the members of `data` cut every member_bytes bytes, without the end marker"""
    assert 1 <= member_bytes <= MAX_MEMBER_BYTES
    return [member(data[i:i + member_bytes], level, strategy) for i in range(0, len(data), member_bytes)]


def bgzf(data, member_bytes=MAX_MEMBER_BYTES, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """`data` as a complete BGZF file"""
    return b"".join(members_of(data, member_bytes, level, strategy)) + EOF_MARKER


def member_table(members):
    """[(in_off, in_len, out_off, isize, crc)] of a file made of these members, as gd_bgzf_scan must report it"""
    out, at, o = [], 0, 0
    for m in members:
        xlen = struct.unpack_from("<H", m, 10)[0]
        crc, isize = struct.unpack_from("<II", m, len(m) - 8)
        out.append((at + 12 + xlen, len(m) - 12 - xlen - 8, o, isize, crc))
        at += len(m)
        o += isize
    return out


STRATEGIES = [("default1", 1, zlib.Z_DEFAULT_STRATEGY), ("default6", 6, zlib.Z_DEFAULT_STRATEGY), ("default9", 9, zlib.Z_DEFAULT_STRATEGY),
              ("fixed6", 6, zlib.Z_FIXED), ("rle", 6, zlib.Z_RLE), ("huffman", 6, zlib.Z_HUFFMAN_ONLY), ("stored", 0, zlib.Z_DEFAULT_STRATEGY)]


def fastq_text(rng, n=25):
    out = []
    for i in range(n):
        ln = int(rng.integers(30, 160))
        out.append(b"@read%d/%d len=%d\n" % (i, 1 + i % 2, ln) + bytes(rng.choice(list(b"ACGT"), size=ln).tolist()) + b"\n+\n" +
                   bytes(rng.integers(35, 74, size=ln).astype("uint8").tolist()) + b"\n")
    return b"".join(out)


def contents(rng):
    """name -> (bytes, keyword arguments of member()): the variants of the matrix"""
    rnd = lambda n: bytes(rng.integers(0, 256, size=n).astype("uint8").tolist())
    half = bytes(rng.integers(48, 112, size=32768).astype("uint8").tolist())  # (64 values: Huffman coding alone makes it fit a member)
    return {
        "fastq": (fastq_text(rng), {}),
        "one_byte_repeated": (b"A" * 3000, {}),           # distance 1, chains of length-258 matches
        "period2": (b"AC" * 1500, {}),
        "period3": (b"ACG" * 1000 + b"AC", {}),
        "random": (rnd(3000), {}),                        # stored blocks inside a dynamic stream
        "max_distance": (half + half, {"stored": half[:32600] * 2}),  # a match at distance 32768 (65536 stored bytes do not fit a member)
        "empty": (b"", {}),
        "one_byte": (b"Q", {}),
        # 65280 input bytes: random ones at level 0 (65316 bytes in all, which still fits BSIZE), FASTQ text at the other rows (random
        # bytes do not fit a member there: a compressed block of them is larger than a stored one)
        "full_member": (rnd(MAX_MEMBER_BYTES), {"compressible": fastq_text(rng, 600)[:MAX_MEMBER_BYTES]}),
        "full_flush": (fastq_text(rng, 12), {"flush_at": 700}),  # an empty stored block and realignment in the middle
        "extra_subfield": (fastq_text(rng, 6), {"extra_front": b"XY" + struct.pack("<H", 5) + b"hello"}),
    }


class BitWriter:
    """deflate bit order: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.bits(int(format(v, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def _fixed_lit(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xc0 + sym - 280, 8)


CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _dynamic_header(w, hlit, hdist, clen_lengths, final=1):
    """block header up to the code-length code; returns {symbol: (code, bits)} of that code (canonical)"""
    hclen = max(i for i, sym in enumerate(CLEN_ORDER) if clen_lengths.get(sym, 0)) + 1
    hclen = max(hclen, 4)
    w.bits(final, 1), w.bits(2, 2), w.bits(hlit - 257, 5), w.bits(hdist - 1, 5), w.bits(hclen - 4, 4)
    for sym in CLEN_ORDER[:hclen]:
        w.bits(clen_lengths.get(sym, 0), 3)
    codes, code = {}, 0
    for n in range(1, 8):
        for sym in sorted(clen_lengths):
            if clen_lengths[sym] == n:
                codes[sym] = (code, n)
                code += 1
        code <<= 1
    return codes, hclen


def hand_streams():
    """name -> raw deflate stream; the tests check each against zlib.decompress(..., -15) before they use it"""
    out = {}
    w = BitWriter()  # a stored block of length 0, twice (the second one final)
    for final in (0, 1):
        w.bits(final, 1), w.bits(0, 2), w.align(), w.bits(0, 16), w.bits(0xffff, 16)
    out["stored_len0"] = w.done()
    # fixed blocks: 'a', 127 x <258 (code 285), distance 1 (code 0)>, 'b' = 32768 bytes; then <3, distance 32768 (code 29, all extra bits set)>
    w = BitWriter()
    w.bits(0, 1), w.bits(1, 2)
    _fixed_lit(w, ord("a"))
    for _ in range(127):
        _fixed_lit(w, 285), w.code(0, 5)
    _fixed_lit(w, ord("b")), _fixed_lit(w, 256)
    w.bits(1, 1), w.bits(1, 2)
    _fixed_lit(w, 257), w.code(29, 5), w.bits(8191, 13)
    _fixed_lit(w, 256)
    out["fixed_285_dist0_dist29"] = w.done()
    # HCLEN at the minimum at which a block can state a length that is not zero: 5, reaching 16 17 18 0 8.  Literal/length lengths: 8 for
    # the symbols 0..254 and 256 (256 codes of length 8: complete), 0 for 255; one distance length, 0: no distance code.
    w = BitWriter()
    cc, hclen = _dynamic_header(w, 257, 1, {0: 1, 8: 2, 18: 2})
    assert hclen == 5
    for sym in range(257):
        w.code(*cc[0 if sym == 255 else 8])
    w.code(*cc[0])
    for ch in b"hclen":
        w.code(ch, 8)  # canonical: symbol s < 255 -> s, 256 -> 255
    w.code(255, 8)
    out["dynamic_hclen_min"] = w.done()
    # exactly one distance code: literal/length 'x' -> 1 bit, 256 and 257 -> 2 bits; distance code 0 -> 1 bit (an incomplete code of one)
    w = BitWriter()
    cc, _ = _dynamic_header(w, 258, 1, {0: 2, 1: 2, 2: 2, 18: 2})
    w.code(*cc[18]), w.bits(120 - 11, 7), w.code(*cc[1]), w.code(*cc[18]), w.bits(135 - 11, 7), w.code(*cc[2]), w.code(*cc[2])
    w.code(*cc[1])
    w.code(0, 1), w.code(3, 2), w.code(0, 1), w.code(2, 2)  # 'x', <3, distance 1>, end of block
    out["dynamic_one_distance_code"] = w.done()
    return out


HAND_EXPECT = {"stored_len0": b"", "fixed_285_dist0_dist29": b"a" * 32767 + b"b" + b"aaa", "dynamic_hclen_min": b"hclen", "dynamic_one_distance_code": b"xxxx"}


def matrix(rng):
    """[(name, member bytes, plain bytes)]: every strategy crossed with every content, then the hand-assembled streams"""
    out = []
    for cname, (data0, kw) in contents(rng).items():
        for sname, level, strategy in STRATEGIES:
            alt, alt0 = kw.get("compressible"), kw.get("stored")
            data, args = data0, {k: v for k, v in kw.items() if k not in ("compressible", "stored")}
            if alt is not None and level != 0:
                assert len(alt) == len(data)
                data = alt
            if alt0 is not None and level == 0:
                data = alt0
            out.append(("%s-%s" % (cname, sname), member(data, level, strategy, **args), data))
    for name, stream in hand_streams().items():
        data = zlib.decompress(stream, -15)
        out.append(("hand-" + name, member_of_stream(stream, data), data))
    return out


def corrupt_crc(m):
    return m[:-8] + bytes([m[-8] ^ 1]) + m[-7:]


def corrupt_isize(m):
    """ISIZE one larger than the stream's output"""
    return m[:-4] + struct.pack("<I", struct.unpack("<I", m[-4:])[0] + 1)
