"""DEFLATE streams that zlib never writes, for the decoder of csrc/bgzf_inflate.h (tests/test_deflate_streams.py on the CPU emulator,
tests/test_deflate_streams_gpu.py on the GPU): a bit-level reader that records which features of RFC 1951 a stream uses, a writer that
leaves every bit to its caller, the designed families, a seeded random family and a fixed list of streams that must be refused.

The reader is the instrument, not the judge: the expected bytes of every stream are zlib.decompress(stream, -15), and the tests hold
the reader, the bytes a family states and zlib against one another before a stream goes anywhere else.  Nothing here is read from a file:
every stream is built from seeds at run time."""
import bisect
import struct
import zlib
from collections import Counter
from fractions import Fraction

import numpy as np

import bgzf_inputs as bi
from bgzf_inputs import CLEN_ORDER, BitWriter

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
MAX_STREAM = 65536 - 26  # what fits one BGZF member beside the header and the trailer
MAX_OUT = 65536

# the classes of gdz_strerror (csrc/bgzf_inflate.h)
E_INPUT = "the deflate stream ends before its last block does"
E_BTYPE = "invalid block type"
E_STORED = "stored block lengths do not match"
E_LENS = "invalid set of code lengths"
E_CODE = "invalid code"
E_DIST = "distance too far back"
E_OUTPUT = "output longer than ISIZE"


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
class Record:
    """what a stream, or a set of streams, uses of the format"""

    def __init__(self):
        self.streams = 0
        self.block_types = Counter()    # BTYPE -> blocks
        self.max_blocks = 0             # blocks of the stream that has most
        self.hlit, self.hdist, self.hclen = set(), set(), set()
        self.len_syms, self.dist_syms = set(), set()  # symbols decoded (257.., 0..)
        self.lit_bits, self.dist_bits, self.clen_bits = Counter(), Counter(), Counter()  # length of the code -> symbols decoded with it
        self.reps, self.crossing = Counter(), Counter()  # 16 / 17 / 18 -> times seen, times run across the literal/distance boundary
        self.rep16_zero = 0             # 16s that repeat a zero
        self.no_dist_blocks = self.one_dist_blocks = 0  # dynamic blocks without a distance code, with exactly one
        self.copies = 0
        self.overlaps = set()           # (dist, len) of the copies with dist < len
        self.reach_first = 0            # copies with dist == the bytes produced so far
        self.max_out = 0

    def merge(self, o):
        self.streams += o.streams
        self.max_blocks, self.max_out = max(self.max_blocks, o.max_blocks), max(self.max_out, o.max_out)
        for k in ("block_types", "lit_bits", "dist_bits", "clen_bits", "reps", "crossing"):
            getattr(self, k).update(getattr(o, k))
        for k in ("hlit", "hdist", "hclen", "len_syms", "dist_syms", "overlaps"):
            getattr(self, k).update(getattr(o, k))
        for k in ("rep16_zero", "no_dist_blocks", "one_dist_blocks", "copies", "reach_first"):
            setattr(self, k, getattr(self, k) + getattr(o, k))
        return self

    def summary(self):
        """one line, for the record of a run"""
        span = lambda c: "%d-%d" % (min(c), max(c)) if c else "none"
        missing = lambda have, all_: ",".join(str(s) for s in all_ if s not in have) or "none"
        return ("streams %d, blocks/stream <= %d, types %s, length symbols %d/29 (missing %s), distance symbols %d/30 (missing %s), code bits used: "
                "lit %s dist %s clen %s, HLIT %d-%d HDIST %d-%d HCLEN %d-%d, 16/17/18 seen %d/%d/%d crossing %d/%d/%d, 16 on zero %d, blocks with "
                "no / one distance code %d/%d, copies %d (dist < len: %d pairs), longest output %d" %
                (self.streams, self.max_blocks, dict(self.block_types), len(self.len_syms), missing(self.len_syms, range(257, 286)), len(self.dist_syms),
                 missing(self.dist_syms, range(30)), span(self.lit_bits), span(self.dist_bits), span(self.clen_bits), min(self.hlit or [0]), max(self.hlit or [0]),
                 min(self.hdist or [0]), max(self.hdist or [0]), min(self.hclen or [0]), max(self.hclen or [0]), self.reps[16], self.reps[17], self.reps[18],
                 self.crossing[16], self.crossing[17], self.crossing[18], self.rep16_zero, self.no_dist_blocks, self.one_dist_blocks, self.copies, len(self.overlaps),
                 self.max_out))


class _Bits:
    def __init__(self, data):
        self.data, self.ip, self.acc, self.n = data, 0, 0, 0

    def fill(self):
        data, ip, acc, n = self.data, self.ip, self.acc, self.n
        while n <= 48 and ip < len(data):
            acc |= data[ip] << n
            n += 8
            ip += 1
        self.ip, self.acc, self.n = ip, acc, n

    def take(self, k):
        if self.n < k:
            self.fill()
            if self.n < k:
                raise ValueError("the stream ends early")
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def decode(self, tab):
        """(symbol, bits of its code): the canonical walk by length"""
        cnt, syms = tab
        if self.n < 15:
            self.fill()
        v, code, first, index = self.acc, 0, 0, 0
        for l in range(1, 16):
            code |= v & 1
            v >>= 1
            c = cnt[l]
            if code - c < first:
                if l > self.n:
                    raise ValueError("the stream ends inside a code")
                self.acc >>= l
                self.n -= l
                return syms[index + code - first], l
            index += c
            first = (first + c) << 1
            code <<= 1
        raise ValueError("invalid code" if self.n >= 15 else "the stream ends inside a code")


def _table(lens, strict=False):
    """zlib's rule (inflate_table): never over-subscribed; incomplete only as a single code of length 1, and never for the code-length code"""
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - cnt[l]
        if left < 0:
            raise ValueError("over-subscribed code lengths")
    total = sum(cnt)
    if left > 0 and not (total == 0 or (not strict and total == 1 and cnt[1] == 1)):
        raise ValueError("incomplete code lengths")
    return cnt, [s for l in range(1, 16) for s, x in enumerate(lens) if x == l]


_FIXED_TABLES = None


def walk(stream):
    """(bytes, Record) of a raw deflate stream; ValueError where the stream is not valid"""
    global _FIXED_TABLES
    if _FIXED_TABLES is None:
        _FIXED_TABLES = (_table(FIXED_LIT), _table(FIXED_DIST))
    rec, out, b = Record(), bytearray(), _Bits(stream)
    rec.streams, blocks, last = 1, 0, 0
    while not last:
        last, btype = b.take(1), b.take(2)
        blocks += 1
        rec.block_types[btype] += 1
        if btype == 3:
            raise ValueError("block type 3")
        if btype == 0:
            b.take(b.n & 7)
            ln, nlen = b.take(16), b.take(16)
            if ln ^ 0xffff != nlen:
                raise ValueError("stored lengths do not match")
            at = b.ip - b.n // 8
            if at + ln > len(stream):
                raise ValueError("the stream ends inside a stored block")
            out += stream[at:at + ln]
            b.ip, b.acc, b.n = at + ln, 0, 0
            continue
        if btype == 1:
            tl, td = _FIXED_TABLES
        else:
            hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            rec.hlit.add(hlit), rec.hdist.add(hdist), rec.hclen.add(hclen)
            if hlit > 286 or hdist > 30:
                raise ValueError("too many length or distance symbols")
            cl = [0] * 19
            for s in CLEN_ORDER[:hclen]:
                cl[s] = b.take(3)
            tc = _table(cl, strict=True)
            lens, n = [], hlit + hdist
            while len(lens) < n:
                s, bits = b.decode(tc)
                rec.clen_bits[bits] += 1
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise ValueError("a repeat with nothing before it")
                    val, rep = lens[-1], 3 + b.take(2)
                    rec.rep16_zero += val == 0
                else:
                    val, rep = 0, (3 + b.take(3) if s == 17 else 11 + b.take(7))
                rec.reps[s] += 1
                if len(lens) + rep > n:
                    raise ValueError("a repeat runs past the code lengths")
                if len(lens) < hlit < len(lens) + rep:
                    rec.crossing[s] += 1
                lens += [val] * rep
            if lens[256] == 0:
                raise ValueError("no end-of-block code")
            tl, td = _table(lens[:hlit]), _table(lens[hlit:])
            nd = sum(1 for l in lens[hlit:] if l)
            rec.no_dist_blocks += nd == 0
            rec.one_dist_blocks += nd == 1
        while True:
            s, bits = b.decode(tl)
            rec.lit_bits[bits] += 1
            if s < 256:
                out.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise ValueError("invalid length symbol")
            rec.len_syms.add(s)
            ln = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
            ds, bits = b.decode(td)
            rec.dist_bits[bits] += 1
            if ds > 29:
                raise ValueError("invalid distance symbol")
            rec.dist_syms.add(ds)
            dist = DIST_BASE[ds] + b.take(DIST_EXTRA[ds])
            if dist > len(out):
                raise ValueError("distance too far back")
            rec.copies += 1
            rec.reach_first += dist == len(out)
            if dist < ln:
                rec.overlaps.add((dist, ln))
                piece = bytes(out[-dist:])
                out += (piece * (ln // dist + 1))[:ln]
            else:
                at = len(out) - dist
                out += out[at:at + ln]
    rec.max_blocks, rec.max_out = blocks, len(out)
    return bytes(out), rec


# ---- the writer ---------------------------------------------------------------------------------------------------------------------
def bitpos(w):
    return 8 * len(w.out) + w.n


def canonical(lens):
    """{symbol: (code, bits)} of the canonical code with these lengths"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


def kraft(lens):
    return sum(Fraction(1, 1 << l) for l in lens if l)


def expand_ops(ops):
    """the code lengths a run-length plan states"""
    out = []
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            out += [out[-1] if op[0] == 16 else 0] * op[1]
    return out


def write_stored(w, data, final=0, nlen=None, declared=None):
    """a stored block; nlen, declared: a NLEN that does not match, a LEN other than the bytes that follow"""
    w.bits(final, 1), w.bits(0, 2), w.align()
    ln = len(data) if declared is None else declared
    w.bits(ln, 16), w.bits(ln ^ 0xffff if nlen is None else nlen, 16)
    assert w.n == 0
    w.out += data


def write_header(w, lit_lens, dist_lens, plan):
    """HLIT, HDIST, HCLEN, the code-length code and the plan's symbols.  plan: "clen" {symbol of the code-length code: bits}, "ops" the
    code lengths as a list of 0..15 and (16 | 17 | 18, count); optional "hclen", "hlit_field" and "hdist_field" (the raw fields), and
    "check": False where the plan is meant not to state lit_lens + dist_lens"""
    clen, ops = plan["clen"], plan["ops"]
    hclen = plan.get("hclen") or max(4, 1 + max(i for i, s in enumerate(CLEN_ORDER) if clen.get(s, 0)))
    w.bits(plan.get("hlit_field", len(lit_lens) - 257), 5), w.bits(plan.get("hdist_field", len(dist_lens) - 1), 5), w.bits(hclen - 4, 4)
    for s in CLEN_ORDER[:hclen]:
        w.bits(clen.get(s, 0), 3)
    if plan.get("check", True):
        assert expand_ops(ops) == list(lit_lens) + list(dist_lens), "the plan states other lengths"
        assert not any(clen.get(s, 0) for s in CLEN_ORDER[hclen:])
    cc = canonical([clen.get(s, 0) for s in range(19)])
    for op in ops:
        if isinstance(op, int):
            w.code(*cc[op])
        else:
            s, count = op
            assert (3, 3, 11)[s - 16] <= count <= (6, 10, 138)[s - 16]
            w.code(*cc[s]), w.bits(count - (3, 3, 11)[s - 16], (2, 3, 7)[s - 16])


def len_sym(length):
    s = bisect.bisect_right(LEN_BASE, length) - 1
    return 257 + s, length - LEN_BASE[s]


def dist_sym(dist):
    s = bisect.bisect_right(DIST_BASE, dist) - 1
    return s, dist - DIST_BASE[s]


def explicit(tokens):
    """the tokens with every copy (length, dist) as ("sym", length symbol, extra, distance symbol, extra)"""
    return [t if isinstance(t, int) or isinstance(t[0], str) else ("sym",) + len_sym(t[0]) + dist_sym(t[1]) for t in tokens]


def write_block(w, tokens, lit_lens=None, dist_lens=None, header_plan=None, final=0, eob=True):
    """one compressed block: fixed where lit_lens is None, else dynamic with exactly these lengths and this header plan.  A token is a
    literal byte, a copy (length, dist), ("sym", length symbol, extra bits, distance symbol, extra bits), ("lit", any symbol of the
    literal/length code) or ("bits", value, n), raw"""
    w.bits(final, 1)
    if lit_lens is None:
        w.bits(1, 2)
        lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
    else:
        w.bits(2, 2)
        write_header(w, lit_lens, dist_lens, header_plan)
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in explicit(tokens):
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        elif t[0] == "lit":
            w.code(*lit[t[1]])
        else:
            _, ls, le, ds, de = t
            assert 0 <= le < 1 << LEN_EXTRA[ls - 257] and 0 <= de < 1 << DIST_EXTRA[ds]
            w.code(*lit[ls]), w.bits(le, LEN_EXTRA[ls - 257]), w.code(*dist[ds]), w.bits(de, DIST_EXTRA[ds])
    if eob:
        w.code(*lit[256])


def apply(out, tokens):
    """what the tokens append to the bytearray out"""
    for t in explicit(tokens):
        if isinstance(t, int):
            out.append(t)
        elif t[0] == "sym":
            ln, dist = LEN_BASE[t[1] - 257] + t[2], DIST_BASE[t[3]] + t[4]
            assert 1 <= dist <= len(out), (dist, len(out))
            for _ in range(ln):
                out.append(out[-dist])
    return out


# ---- helpers of the families: they choose, the writer does not -------------------------------------------------------------------
def balanced(n):
    """complete code lengths for n symbols, as even as they come"""
    if n == 1:
        return [1]
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def random_tree(n, cap, rng):
    """complete code lengths for n symbols from random splits of leaves, half the time of the deepest one, none deeper than cap"""
    if n == 1:
        return [1]
    leaves = [1, 1]
    while len(leaves) < n:
        ok = [i for i, l in enumerate(leaves) if l < cap]
        i = max(ok, key=lambda j: leaves[j]) if rng.random() < 0.5 else ok[int(rng.integers(len(ok)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return [leaves[i] for i in rng.permutation(n)]


def spread(symbols, lens, n):
    """lengths lens[i] on symbols[i] in an alphabet of n symbols"""
    out = [0] * n
    for s, l in zip(symbols, lens):
        out[s] = l
    return out


def used_symbols(tokens):
    lit, dist = {256}, set()
    for t in explicit(tokens):
        if isinstance(t, int):
            lit.add(t)
        elif t[0] == "lit":
            lit.add(t[1])
        elif t[0] == "sym":
            lit.add(t[1]), dist.add(t[3])
    return sorted(lit), sorted(dist)


def plan_rle(seq, rng=None):
    """a run-length plan for seq.  Without rng the longest run code wherever one fits, 18 before 17 before 16; with rng a random choice
    among the codes that fit, literal lengths included, with the count at its smallest, its largest or in between"""
    ops, i, n = [], 0, len(seq)
    while i < n:
        run = 1
        while i + run < n and seq[i + run] == seq[i]:
            run += 1
        choices = []
        if seq[i] == 0 and run >= 11:
            choices.append((18, 11, min(run, 138)))
        if seq[i] == 0 and run >= 3:
            choices.append((17, 3, min(run, 10)))
        if i > 0 and seq[i] == seq[i - 1] and run >= 3:
            choices.append((16, 3, min(run, 6)))
        if rng is not None:
            choices = [choices[int(rng.integers(len(choices)))]] if choices and rng.random() < 0.8 else []
        if not choices:
            ops.append(seq[i])
            i += 1
            continue
        s, lo, hi = choices[0]
        count = hi if rng is None else (lo, hi, int(rng.integers(lo, hi + 1)))[int(rng.integers(3))]
        ops.append((s, count))
        i += count
    return ops


def clen_for(ops, lens_of=balanced):
    """a complete code-length code over the symbols the plan uses (and one more where it uses one alone: zlib wants the code complete)"""
    used = sorted({op if isinstance(op, int) else op[0] for op in ops})
    if len(used) == 1:
        used.append(1 if used[0] == 0 else 0)
    return dict(zip(used, lens_of(len(used))))


def plan(lit_lens, dist_lens, ops=None, clen=None, **kw):
    ops = plan_rle(list(lit_lens) + list(dist_lens)) if ops is None else ops
    return dict(kw, ops=ops, clen=clen_for(ops) if clen is None else clen)


def dynamic(w, tokens, final=0, lit_lens=None, dist_lens=None, header_plan=None):
    """a dynamic block; where no lengths are given, balanced ones over the symbols the tokens use"""
    if lit_lens is None:
        lit, dist = used_symbols(tokens)
        lit_lens = spread(lit, balanced(len(lit)), max(257, lit[-1] + 1))
        dist_lens = spread(dist, balanced(len(dist)), dist[-1] + 1) if dist else [0]
    write_block(w, tokens, lit_lens, dist_lens, header_plan or plan(lit_lens, dist_lens), final)


def rnd_bytes(rng, n, lo=0, hi=256):
    return [int(x) for x in rng.integers(lo, hi, size=n)]


def grow(rng, out, target, first=300, lo=0, hi=256):
    """tokens that take the bytearray out to exactly target bytes: `first` random literals where it is empty, then copies of up to 258
    bytes from random distances"""
    tokens = []
    if not out:
        tokens += rnd_bytes(rng, min(first, target), lo, hi)
        apply(out, tokens)
    while len(out) < target:
        ln = min(258, target - len(out))
        t = [(ln, int(rng.integers(1, min(len(out), 32768) + 1)))] if ln >= 3 else rnd_bytes(rng, ln, lo, hi)
        apply(out, t)
        tokens += t
    return tokens


class Family(list):
    """[(name, stream, expected bytes)]"""

    def add(self, name, w, out):
        stream = w.done() if isinstance(w, BitWriter) else w
        assert len(stream) <= MAX_STREAM and len(out) <= MAX_OUT, (name, len(stream), len(out))
        self.append((name, stream, bytes(out)))


# ---- the designed families ----------------------------------------------------------------------------------------------------------
def symbols():
    """every length symbol and every distance symbol with its extra bits all zero and all one, in a fixed and in a dynamic block; one copy
    reaches exactly the member's first byte"""
    fam = Family()
    rng = np.random.default_rng(101)
    out = bytearray()
    tokens = grow(rng, out, 259)
    tokens.append((40, 259))  # dist == bytes so far: the first byte of the member
    apply(out, tokens[-1:])
    for s in range(29):
        for extra in (0, (1 << LEN_EXTRA[s]) - 1):
            ds, de = dist_sym(int(rng.integers(1, len(out) + 1)))
            tokens.append(("sym", 257 + s, extra, ds, de))
            apply(out, tokens[-1:])
    for ds in range(30):
        for extra in (0, (1 << DIST_EXTRA[ds]) - 1):
            tokens += grow(rng, out, max(len(out), DIST_BASE[ds] + extra))
            tokens.append(("sym", 257 + int(rng.integers(0, 8)), 0, ds, extra))
            apply(out, tokens[-1:])
    for name, block in (("fixed", write_block), ("dynamic", dynamic)):
        w = BitWriter()
        block(w, tokens, final=1)
        fam.add("symbols-" + name, w, out)
    return fam


OVERLAP_DIST = [1, 2, 3, 63, 64, 65, 127, 128, 129]
OVERLAP_LEN = [3, 63, 64, 65, 128, 129, 258]


def overlap():
    """the copies of the k % dist path around the 64-lane step, each behind two fresh literals"""
    fam = Family()
    rng = np.random.default_rng(102)
    out = bytearray()
    tokens = grow(rng, out, 200)
    for d in OVERLAP_DIST:
        for ln in OVERLAP_LEN:
            t = rnd_bytes(rng, 2) + [(ln, d)]
            tokens += t
            apply(out, t)
    for name, block in (("fixed", write_block), ("dynamic", dynamic)):
        w = BitWriter()
        block(w, tokens, final=1)
        fam.add("overlap-pairs-" + name, w, out)
    for name, tokens in (("literal-then-3-1", [ord("x"), (3, 1)]),
                         ("copy-of-a-copy", rnd_bytes(rng, 7) + [(10, 5), (10, 10), (70, 20), (258, 90), (130, 258), (64, 64), (65, 64)])):
        for kind, block in (("fixed", write_block), ("dynamic", dynamic)):
            w = BitWriter()
            block(w, tokens, final=1)
            fam.add("overlap-%s-%s" % (name, kind), w, apply(bytearray(), tokens))
    return fam


LADDER = list(range(1, 16)) + [15]  # 1, 2, ..., 14, 15, 15: complete, and as deep as the format goes
LADDER_LIT = [65, 67, 71, 84, 78, 97, 99, 103, 116, 110, 256, 257, 258, 283, 284, 285]
LADDER_DIST = list(range(14)) + [28, 29]


def _ladder_tokens(rng, out, lits, lsyms, dsyms, n=400):
    """n random tokens over these literals, length symbols and distance symbols (those whose distances are there yet)"""
    tokens = []
    for _ in range(n):
        ok = [d for d in dsyms if DIST_BASE[d] <= len(out)]
        if not ok or rng.random() < 0.5:
            t = lits[int(rng.integers(len(lits)))]
        else:
            ls, ds = lsyms[int(rng.integers(len(lsyms)))], ok[int(rng.integers(len(ok)))]
            de = min(int(rng.integers(1 << DIST_EXTRA[ds])), len(out) - DIST_BASE[ds])
            t = ("sym", ls, int(rng.integers(1 << LEN_EXTRA[ls - 257])), ds, de)
        if len(out) + 258 > MAX_OUT:
            break
        tokens.append(t)
        apply(out, [t])
    return tokens


def long_codes():
    fam = Family()
    rng = np.random.default_rng(103)
    # 1, 2, ..., 14, 15, 15 in both alphabets, up the symbols and down them: every symbol is used, the end-of-block code at 11 bits and at 6
    w, out = BitWriter(), bytearray()
    write_block(w, grow(rng, out, 33000, lo=65, hi=91), final=0)  # (so that the distance symbols 28 and 29 can be used)
    for k, order in enumerate((LADDER, LADDER[::-1])):
        lit_lens, dist_lens = spread(LADDER_LIT, order, 286), spread(LADDER_DIST, order, 30)
        tokens = _ladder_tokens(rng, out, LADDER_LIT[:10], LADDER_LIT[11:], LADDER_DIST, 120)
        tokens += [t for t in LADDER_LIT[:10]] + [("sym", ls, 0, ds, 0) for ls, ds in zip(LADDER_LIT[11:] * 4, LADDER_DIST)]
        apply(out, tokens[-26:])
        write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens), final=k)
    fam.add("long-ladder-15", w, out)
    # the two sides of the lookup tables' index: 7, 10 and 11 bits over all 286 symbols (110 + 112 + 64), and 1..5, 8, 9 bits on 17 distance symbols
    lit_lens = [7] * 110 + [10] * 112 + [11] * 64
    dsyms = [0, 1, 2, 3, 4] + [5, 7, 9, 11] + [6, 8, 10, 12, 13, 14, 15, 16]
    dist_lens = spread(dsyms, [1, 2, 3, 4, 5] + [8] * 4 + [9] * 8, 17)
    assert kraft(lit_lens) == 1 and kraft(dist_lens) == 1
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, list(range(256)), list(range(257, 286)), dsyms, 1500)
    write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens), final=1)
    fam.add("long-table-edges", w, out)
    # ... and ladders that end at 10, 11, 11 (literal/length) and 8, 9, 9 (distance)
    lsyms, dsyms = [65, 66, 67, 68, 69, 70, 256, 257, 258, 259, 97, 98], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    lit_lens, dist_lens = spread(lsyms, list(range(1, 11)) + [11, 11], 260), spread(dsyms, list(range(1, 9)) + [9, 9], 10)
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, [65, 66, 67, 68, 69, 70, 97, 98], [257, 258, 259], dsyms, 600)
    write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens), final=1)
    fam.add("long-ladder-to-the-index", w, out)
    # a code-length code of 1, 2, ..., 6, 7, 7 over the eight symbols 0, 3, 4, 5, 6, 16, 17, 18, all of them used by the plan
    lit_lens = spread(list(range(65, 73)) + list(range(97, 101)) + list(range(256, 264)), [3] * 4 + [4] * 4 + [5] * 4 + [6] * 8, 264)
    dist_lens = [3, 3, 3, 3, 0, 0, 0, 3, 3, 3, 0, 3]
    ops = plan_rle(lit_lens + dist_lens)
    assert {op if isinstance(op, int) else op[0] for op in ops} == {0, 3, 4, 5, 6, 16, 17, 18}
    for k, order in enumerate(([18, 0, 16, 3, 4, 5, 6, 17], [6, 5, 4, 17, 3, 16, 0, 18])):
        w, out = BitWriter(), bytearray()
        tokens = _ladder_tokens(rng, out, list(range(65, 73)) + list(range(97, 101)), list(range(257, 264)), [0, 1, 2, 3, 7, 8, 9, 11], 300)
        write_block(w, tokens, lit_lens, dist_lens, dict(ops=ops, clen=dict(zip(order, list(range(1, 8)) + [7]))), final=1)
        fam.add("long-clen-ladder-%d" % k, w, out)
    return fam


def header():
    fam = Family()
    rng = np.random.default_rng(104)
    # HLIT 257, HDIST 1, HCLEN 5 (16 17 18 0 8), no distance code: 8 bits for 0..254 and 256
    lit_lens = [8] * 255 + [0, 8]
    ops = [8] + [(16, 6)] * 42 + [8, 8, 0, 8, 0]
    w, tokens = BitWriter(), rnd_bytes(rng, 300, 0, 255)
    write_block(w, tokens, lit_lens, [0], dict(ops=ops, clen={8: 1, 0: 2, 16: 2}), final=1)
    fam.add("header-smallest", w, tokens)
    # HLIT 286, HDIST 30, HCLEN 19 (the last of the order is 15, so a 15-bit code has to be stated), every length written out
    lit_lens, dist_lens = spread(LADDER_LIT, LADDER, 286), [4, 4] + [5] * 28
    for name, ops in (("plain", lit_lens + dist_lens), ("runs", None)):
        w, out = BitWriter(), bytearray()
        tokens = _ladder_tokens(rng, out, LADDER_LIT[:10], LADDER_LIT[11:], list(range(30)), 400)
        p = plan(lit_lens, dist_lens, ops)
        write_block(w, tokens, lit_lens, dist_lens, p, final=1)
        assert max(i for i, s in enumerate(CLEN_ORDER) if p["clen"].get(s, 0)) == 18
        fam.add("header-largest-" + name, w, out)
    # every run code at its smallest and its largest count: 18 x 138 and 11, 16 x 3 and 6, 17 x 3 and 10; one distance code of length 1
    ops = [(18, 138), 5, (16, 3), (18, 11), 5, (16, 6), (17, 3), 5, (17, 10), 5, (18, 81), 5, 4, (16, 6), 4, 4, 1]
    lens = expand_ops(ops)
    lit_lens, dist_lens = lens[:266], lens[266:]
    assert kraft(lit_lens) == 1 and dist_lens == [1]
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, [i for i in range(256) if lit_lens[i]], list(range(257, 266)), [0], 200)
    write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens, ops), final=1)
    fam.add("header-run-counts", w, out)
    # a 16 behind an 18 and behind a 17: it repeats zero
    ops = [(18, 20), (16, 5), 3, 3, (17, 4), (16, 3), 3, 3, (18, 138), (18, 82), 3, 3, 3, 4, 4, 2, 2, 2, 2]
    lens = expand_ops(ops)
    lit_lens, dist_lens = lens[:261], lens[261:]
    assert kraft(lit_lens) == 1 and kraft(dist_lens) == 1
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, [25, 26, 34, 35], [257, 258, 259, 260], [0, 1, 2, 3], 200)
    write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens, ops), final=1)
    fam.add("header-16-repeats-zero", w, out)
    # a 16 across the boundary: the 4 of the symbols 257..259 runs on into the first three distance lengths
    lit_lens = spread([65, 66, 67, 68, 97, 98, 99, 100, 256, 257, 258, 259], [3] * 4 + [4] * 8, 260)
    dist_lens = [4] * 16
    ops = lit_lens[:257] + [(16, 6)] + [4] * 13
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, [65, 66, 67, 68, 97, 98, 99, 100], [257, 258, 259], list(range(16)), 300)
    write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens, ops), final=1)
    fam.add("header-16-across", w, out)
    # a 17 across: two zero lengths at the end of the literal/length code (HLIT is larger than it need be) and three at the start of the other
    lit_lens, dist_lens = lit_lens + [0, 0], [0, 0, 0] + [3] * 8
    ops = lit_lens[:260] + [(17, 5)] + [3] * 8
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, [65, 66, 67, 68, 97, 98, 99, 100], [257, 258, 259], list(range(3, 11)), 300)
    write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens, ops), final=1)
    fam.add("header-17-across", w, out)
    # an 18 across: ten and eight
    lit_lens, dist_lens = lit_lens[:260] + [0] * 10, [0] * 8 + [3] * 8
    ops = lit_lens[:260] + [(18, 18)] + [3] * 8
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, [65, 66, 67, 68, 97, 98, 99, 100], [257, 258, 259], list(range(8, 16)), 300)
    write_block(w, tokens, lit_lens, dist_lens, plan(lit_lens, dist_lens, ops), final=1)
    fam.add("header-18-across", w, out)
    # no distance code at all with HDIST 30, and a single distance code of length 1 that is not symbol 0
    lits = list(range(48, 58))
    lit_lens = spread(lits + [256, 257], balanced(12), 258)
    w, tokens = BitWriter(), [lits[i % 10] for i in rnd_bytes(rng, 100)]
    write_block(w, tokens, lit_lens, [0] * 30, plan(lit_lens, [0] * 30), final=1)
    fam.add("header-no-distance-code", w, tokens)
    w, out = BitWriter(), bytearray()
    tokens = _ladder_tokens(rng, out, lits, [257], [5], 100)
    write_block(w, tokens, lit_lens, [0, 0, 0, 0, 0, 1], plan(lit_lens, [0, 0, 0, 0, 0, 1]), final=1)
    fam.add("header-one-distance-code", w, out)
    return fam


def blocks():
    fam = Family()
    rng = np.random.default_rng(105)
    # 300 dynamic blocks of one to five symbols, the end-of-block code among them
    w, out = BitWriter(), bytearray()
    for k in range(300):
        tokens = [(int(rng.integers(3, 12)), int(rng.integers(1, len(out) + 1))) if out and rng.random() < 0.3 else int(rng.integers(256)) for _ in range(k % 5)]
        apply(out, tokens)
        dynamic(w, tokens, final=k == 299)
    fam.add("blocks-300-dynamic", w, out)
    # fixed, dynamic, fixed: the fixed tables are built again behind a dynamic block
    w, out = BitWriter(), bytearray()
    for k, block in enumerate((write_block, dynamic, write_block)):
        tokens = rnd_bytes(rng, 40) + [(20, 7), (258, 33)]
        apply(out, tokens)
        block(w, tokens, final=k == 2)
    fam.add("blocks-fixed-dynamic-fixed", w, out)
    # a stored block behind a compressed one that ends at each of the eight bit positions (3 + 9 j + 7 bits: j literals above 143)
    w, out, seen = BitWriter(), bytearray(), set()
    for j in range(8):
        tokens = rnd_bytes(rng, j, 144, 256)
        write_block(w, tokens, final=0)
        seen.add(bitpos(w) % 8)
        data = rnd_bytes(rng, 5 + j)
        write_stored(w, bytes(data), final=j == 7)
        apply(out, tokens + data)
    assert seen == set(range(8))
    fam.add("blocks-stored-at-every-bit", w, out)
    # stored blocks of no bytes and of one, between compressed ones
    w, out = BitWriter(), bytearray(b"ab?cd")
    write_block(w, [97, 98], final=0), write_stored(w, b""), write_stored(w, b"?"), write_stored(w, b""), write_block(w, [99, 100], final=1)
    fam.add("blocks-stored-0-and-1", w, out)
    # a stored block that ends one byte before, at, and one behind an input boundary of the ring, and a compressed block behind it
    for boundary in (1024, 2048):
        for end in (boundary - 1, boundary, boundary + 1):
            w, out = BitWriter(), bytearray()
            tokens = rnd_bytes(rng, 3)
            write_block(w, tokens, final=0)
            data = rnd_bytes(rng, end - (len(w.out) + 1 + 4))
            write_stored(w, bytes(data))
            assert len(w.out) == end and w.n == 0
            tail = rnd_bytes(rng, 30) + [(100, 1000), (258, 3)]
            dynamic(w, tail, final=1)
            fam.add("blocks-stored-ends-at-%d" % end, w, apply(out, tokens + data + tail))
    # a final block that is empty
    w, out = BitWriter(), bytearray()
    tokens = rnd_bytes(rng, 20)
    dynamic(w, tokens), write_block(w, [], final=1)
    fam.add("blocks-final-empty-fixed", w, apply(out, tokens))
    return fam


RING_LIT = spread([65, 67, 71, 84, 78, 256, 257, 258, 97, 99, 103, 116, 285, 110, 284, 283], LADDER, 286)  # 'A' 1 bit ... 284, 283: 15 bits
RING_DIST = spread(list(range(14)) + [28, 29], LADDER, 30)


def _straddle(rng, boundary, back, dist_code, skew):
    """a stream in which the 15-bit code of length symbol 284 (dist_code: of distance symbol 29), with its 5 (13) extra bits behind it,
    starts `back` bits in front of byte `boundary` of the input.  A stored block of 297 + skew bytes comes first: behind it the decoder
    takes its input from byte 302 + skew on, four at a time, so the refills meet the ring at every offset modulo 4"""
    w, out = BitWriter(), bytearray(rnd_bytes(rng, 297 + skew))
    write_stored(w, bytes(out))
    write_block(w, grow(rng, out, 32768), final=0)
    assert len(w.out) < 1000
    w.bits(1, 1), w.bits(2, 2)
    write_header(w, RING_LIT, RING_DIST, plan(RING_LIT, RING_DIST))
    lit = canonical(RING_LIT)
    target = 8 * boundary - back - (20 if dist_code else 0)
    fill = [65, 67, 71, 84, 78, 97, 99]
    while bitpos(w) < target:
        left = target - bitpos(w)
        s = fill[int(rng.integers(len(fill)))] if left > 24 else 65  # ('A' is one bit: any position can be reached)
        w.code(*lit[s])
        out.append(s)
    assert bitpos(w) == target
    tokens = [("sym", 284, 31, 29, 8191), 67, ("sym", 284, 0, 29, 0), 71, ("sym", 283, 17, 28, 4242), 84]
    dist = canonical(RING_DIST)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        else:
            w.code(*lit[t[1]]), w.bits(t[2], 5), w.code(*dist[t[3]]), w.bits(t[4], 13)
    w.code(*lit[256])
    return w, apply(out, tokens)


def ring():
    fam = Family()
    rng = np.random.default_rng(106)
    # streams of exactly n input bytes: random tokens in a fixed block, then 8-bit literals, a byte each, up to the length
    for n in (1023, 1024, 1025, 2047, 2048, 2049):
        out = bytearray()
        tokens = grow(rng, out, 300)
        bits = 3 + 9 * len(tokens) + 7  # (an upper bound: 9 for a literal, 48 for a copy)
        while bits + 8 * 60 < 8 * n:
            t = [int(rng.integers(256))] if rng.random() < 0.6 else [(int(rng.integers(3, 60)), int(rng.integers(1, len(out) + 1)))]
            bits += 9 if isinstance(t[0], int) else 48
            tokens += t
            apply(out, t)
        while True:  # (a literal below 144 is one byte more: all but the last of them at once)
            w = BitWriter()
            write_block(w, tokens, final=1)
            if len(w.done()) >= n:
                break
            tokens += rnd_bytes(rng, max(1, n - len(w.done()) - 1), 0, 144)
        assert len(w.done()) == n
        fam.add("ring-%d-bytes" % n, w, apply(bytearray(), tokens))
    # the longest things a refill must hold, across the edges of the ring's two slots: the boundary inside the code, between the code and
    # its extra bits, and inside the extra bits
    for boundary in (1024, 2048):
        for dist_code in (False, True):
            for back in (7, 15, 18):
                w, out = _straddle(rng, boundary, back, dist_code, len(fam) % 4)
                fam.add("ring-%s-code-%d-bits-before-%d" % ("distance" if dist_code else "length", back, boundary), w, out)
    # the last end-of-block code ends in each bit of the final byte (3 + 9 j + 7 bits)
    seen = set()
    for j in range(8):
        w, tokens = BitWriter(), rnd_bytes(rng, j, 144, 256)
        write_block(w, tokens, final=1)
        seen.add(bitpos(w) % 8)
        fam.add("ring-last-code-ends-at-bit-%d" % (bitpos(w) % 8), w, tokens)
    assert seen == set(range(8))
    return fam


def full():
    """a member of exactly 65536 bytes that ends in a copy of 258, sixteen times, each behind a stored member of k = 0..15 bytes: in a file
    of these members its output starts at every offset modulo 16 (k (k + 1) / 2 mod 16 is a permutation)"""
    fam = Family()
    rng = np.random.default_rng(107)
    out = bytearray()
    tokens = grow(rng, out, MAX_OUT - 258) + [(258, 12345)]
    apply(out, tokens[-1:])
    assert len(out) == MAX_OUT
    w = BitWriter()
    dynamic(w, tokens, final=1)
    stream = w.done()
    for k in range(16):
        data = bytes(rnd_bytes(rng, k))
        w = BitWriter()
        write_stored(w, data, final=1)
        fam.add("full-stored-%d" % k, w, data)
        fam.add("full-behind-%d" % k, stream, out)
    return fam


def random(seed, n):
    """n streams of one to five blocks: random complete codes up to 15 (7) bits deep, random header plans, random literals and copies with
    extra bits from {0, all ones, random}"""
    fam = Family()
    rng = np.random.default_rng(seed)
    pick = lambda xs, k: sorted(int(x) for x in rng.choice(xs, size=k, replace=False))
    extra = lambda bits: (0, (1 << bits) - 1, int(rng.integers(1 << bits)))[int(rng.integers(3))]
    for k in range(n):
        w, out = BitWriter(), bytearray()
        n_blocks = int(rng.integers(1, 6))
        cap = int(rng.integers(2000, 20000))
        for b in range(n_blocks):
            final, kind = b == n_blocks - 1, rng.random()
            if kind < 0.1:
                data = rnd_bytes(rng, int(rng.integers(0, 200)))
                write_stored(w, bytes(data), final)
                out += bytes(data)
                continue
            lits = pick(256, int(rng.integers(1, 60)))
            dsyms = [d for d in pick(30, int(rng.integers(0, 31))) if DIST_BASE[d] <= len(out) + 1]
            lsyms = [257 + s for s in pick(29, int(rng.integers(1, 30)))] if dsyms else []
            tokens = []
            for _ in range(int(rng.integers(0, 400))):
                ok = [d for d in dsyms if DIST_BASE[d] <= len(out)]
                if not ok or rng.random() < 0.5:
                    t = lits[int(rng.integers(len(lits)))]
                else:
                    ls, ds = lsyms[int(rng.integers(len(lsyms)))], ok[int(rng.integers(len(ok)))]
                    t = ("sym", ls, extra(LEN_EXTRA[ls - 257]), ds, min(extra(DIST_EXTRA[ds]), len(out) - DIST_BASE[ds]))
                if len(out) + 258 > cap:
                    break
                tokens.append(t)
                apply(out, [t])
            if kind < 0.3:
                write_block(w, tokens, final=final)
                continue
            lit_syms = lits + [256] + lsyms  # (the alphabet may be wider than what the tokens use)
            hlit = int(rng.integers(max(257, lit_syms[-1] + 1), 287))
            lit_lens = spread(lit_syms, random_tree(len(lit_syms), 15, rng), hlit)
            hdist = int(rng.integers(dsyms[-1] + 1 if dsyms else 1, 31))
            dist_lens = spread(dsyms, random_tree(len(dsyms), 15, rng), hdist) if dsyms else [0] * hdist
            ops = plan_rle(lit_lens + dist_lens, rng)
            clen = clen_for(ops, lambda m: random_tree(m, 7, rng))
            write_block(w, tokens, lit_lens, dist_lens, dict(ops=ops, clen=clen), final)
        fam.add("random-%d-%d" % (seed, k), w, out)
    return fam


FAMILIES = {"symbols": symbols, "overlap": overlap, "long_codes": long_codes, "header": header, "blocks": blocks, "ring": ring, "full": full,
            "random": lambda: random(1, 300)}
_cache = {}


def family(name):
    """the family, built once"""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


# ---- streams that must be refused ---------------------------------------------------------------------------------------------------
def invalid():
    """[(name, stream, ISIZE of the member's trailer, error class)]: one or two per class of gdz_strerror, each built with the writer"""
    out = []

    def add(name, w, isize, err):
        out.append((name, w.done() if isinstance(w, BitWriter) else w, isize, err))

    lit8 = [8] * 255 + [0, 8]  # a complete code that zlib and the decoder accept: 0..254 and 256 at 8 bits
    ok_plan = lambda lit, dist, **kw: plan(lit, dist, **kw)
    w = BitWriter()
    write_block(w, [97, 98], final=0), w.bits(1, 1), w.bits(3, 2), w.bits(0, 13)
    add("block-type-3", w, 2, E_BTYPE)
    w = BitWriter()
    write_stored(w, b"abcd", final=1, nlen=4)
    add("stored-nlen-mismatch", w, 4, E_STORED)
    w = BitWriter()
    write_block(w, [97], final=0), write_stored(w, b"abcd", final=1, nlen=0xfffb ^ 0x0100)
    add("stored-nlen-one-bit", w, 5, E_STORED)
    # code lengths
    lit = [8] * 255 + [7, 8]  # one 7 among 256 eights: over-subscribed
    w = BitWriter()
    write_block(w, [97, 98], lit, [0], ok_plan(lit, [0]), final=1)
    add("lens-over-subscribed-literal", w, 2, E_LENS)
    w = BitWriter()
    write_block(w, [97, 98], lit8, [1, 1, 1], ok_plan(lit8, [1, 1, 1]), final=1)
    add("lens-over-subscribed-distance", w, 2, E_LENS)
    lit = [8] * 254 + [0, 0, 8]
    w = BitWriter()
    write_block(w, [97, 98], lit, [0], ok_plan(lit, [0]), final=1)
    add("lens-incomplete-literal", w, 2, E_LENS)
    w = BitWriter()
    write_block(w, [97, 98], lit8, [2, 2, 2], ok_plan(lit8, [2, 2, 2]), final=1)
    add("lens-incomplete-distance", w, 2, E_LENS)
    w = BitWriter()
    write_block(w, [97, 98], lit8, [0], dict(ops=plan_rle(lit8 + [0]), clen={0: 2, 8: 2, 16: 2}), final=1)
    add("lens-incomplete-code-length-code", w, 2, E_LENS)
    w = BitWriter()
    write_block(w, [], lit8, [0], dict(ops=[], clen={0: 1, 8: 1, 16: 1}, check=False), final=1, eob=False)  # (nothing behind the code that is refused)
    add("lens-over-subscribed-code-length-code", w, 2, E_LENS)
    lit = [8] * 256 + [0]
    w = BitWriter()
    write_block(w, [97, 98], lit, [0], ok_plan(lit, [0]), final=1, eob=False)
    add("lens-no-end-of-block-code", w, 2, E_LENS)
    w = BitWriter()
    write_block(w, [], lit8, [0], dict(ops=[(16, 3)] + lit8[3:] + [0], clen={8: 1, 0: 2, 16: 2}, check=False), final=1, eob=False)
    add("lens-16-first", w, 0, E_LENS)
    w = BitWriter()
    write_block(w, [], lit8, [0], dict(ops=lit8 + [(18, 11)], clen={8: 1, 0: 2, 18: 2}, check=False), final=1, eob=False)
    add("lens-repeat-past-the-end", w, 0, E_LENS)
    w = BitWriter()
    write_block(w, [], lit8, [0], dict(ops=lit8 + [(16, 3)], clen={8: 1, 0: 2, 16: 2}, check=False), final=1, eob=False)
    add("lens-16-past-the-end", w, 0, E_LENS)
    for name, fields in (("hlit-287", dict(hlit_field=30)), ("hdist-31", dict(hdist_field=30))):
        w = BitWriter()
        write_block(w, [97, 98], lit8, [0], dict(ok_plan(lit8, [0]), check=False, **fields), final=1)
        add("lens-" + name, w, 2, E_LENS)
    # codes the fixed block has and the format does not
    w = BitWriter()
    write_block(w, [97, ("lit", 286)], final=1)
    add("code-fixed-symbol-286", w, 1, E_CODE)
    w = BitWriter()
    write_block(w, [97, 98, 99, ("lit", 257), ("bits", int("11110"[::-1], 2), 5)], final=1)  # (distance symbol 30: 11110, first bit first)
    add("code-fixed-distance-30", w, 6, E_CODE)
    # the window and the room
    w = BitWriter()
    write_block(w, [97, 98, 99, (3, 4)], final=1)
    add("distance-one-beyond-the-first-byte", w, 6, E_DIST)
    w = BitWriter()
    dynamic(w, [97] * 40 + [(3, 41)], final=1)
    add("distance-one-beyond-dynamic", w, 43, E_DIST)
    w = BitWriter()
    write_block(w, [97, 98, 99, 100], final=1)
    add("output-one-literal-more-than-isize", w, 3, E_OUTPUT)
    w = BitWriter()
    write_block(w, [97, 98, (10, 2)], final=1)
    add("output-a-copy-one-byte-more-than-isize", w, 11, E_OUTPUT)
    w = BitWriter()
    write_block(w, [97], final=0), write_stored(w, b"abcd", final=1)
    add("output-stored-one-byte-more-than-isize", w, 4, E_OUTPUT)
    # streams that end early: inside a 15-bit code (all ones: its first 9 bits end the last byte), inside the five extra bits of 284
    # (two of them there), inside a stored block
    lit, dist = RING_LIT, RING_DIST
    for name, last in (("inside-a-code", [("bits", 0x1ff, 9)]), ("inside-extra-bits", [("lit", 284), ("bits", 3, 2)])):
        w = BitWriter()
        w.bits(0, 1), w.bits(2, 2)
        write_header(w, lit, dist, plan(lit, dist))
        need = 9 if name == "inside-a-code" else 17
        while (bitpos(w) + need) % 8:
            w.code(*canonical(lit)[65])  # ('A', one bit)
        cl = canonical(lit)
        for t in last:
            if t[0] == "lit":
                w.code(*cl[t[1]])
            else:
                w.bits(t[1], t[2])
        assert w.n == 0
        add("cut-" + name, w, 1000, E_INPUT)
    w = BitWriter()
    write_stored(w, b"a" * 50, final=1, declared=100)
    add("cut-inside-a-stored-block", w, 100, E_INPUT)
    w = BitWriter()
    write_block(w, [97, 98], final=0)
    add("cut-no-final-block", w, 2, E_INPUT)
    return out


def member(stream, data):
    return bi.member_of_stream(stream, data)


def member_with_trailer(stream, isize, crc=0):
    """a member whose trailer says what the caller says"""
    m = bi.member_of_stream(stream, b"")
    return m[:-8] + struct.pack("<II", crc, isize)


def zlib_refuses(stream, isize):
    """whether zlib's raw inflate, given room for isize bytes, does not reach the end of the stream"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, isize + 1)
    except zlib.error:
        return True
    return not d.eof or len(out) > isize
