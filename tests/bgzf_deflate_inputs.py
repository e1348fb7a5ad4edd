"""inputs of the BGZF compression tests (tests/test_bgzf_deflate.py on the CPU emulator, tests/test_bgzf_deflate_gpu.py on the GPU): the
smallest inputs that reach each edge of csrc/bgzf_deflate.h, and the two golden SAM texts"""
import gzip
import os

import numpy as np

import bgzf_inputs as bi
from fixture_io import LR, SR

M = bi.MAX_MEMBER_BYTES
PATTERN = b"q7#Zk!pW"  # eight bytes that occur nowhere else in their inputs


def golden_text(which):
    path = os.path.join(SR, "sr.golden.sam.gz") if which == "sr" else os.path.join(LR, "hifi.golden.sam.gz")
    with gzip.open(path, "rb") as f:
        return f.read()


_cache = {}


def inputs():
    """[(name, bytes)], built once"""
    if "inputs" in _cache:
        return _cache["inputs"]
    rng = np.random.default_rng(11)
    rnd = lambda n: bytes(rng.integers(0, 256, size=n).astype("uint8").tolist())
    text = bi.fastq_text(rng, 1500)
    assert len(text) >= 3 * M + 17
    out = [("len%d" % n, b"ACGT"[:n]) for n in range(5)]                       # below and at the minimum match and the hash width
    out += [("run%d" % n, b"A" * n) for n in (257, 258, 259, 260, M)]          # the maximum length and its split
    out += [("dist32768", PATTERN + b"A" * (32768 - 8) + PATTERN),             # the farthest match there is: must be found
            ("dist32769", PATTERN + b"A" * (32769 - 8) + PATTERN),             # one further: must not be used
            ("dist32768_3", b"q7#" + b"A" * (32768 - 3) + b"q7#"), ("dist32769_3", b"q7#" + b"A" * (32769 - 3) + b"q7#"),
            ("bytes256x2", bytes(range(256)) * 2),                            # literal codes on both sides of 143 / 144 in a fixed block
            ("random", rnd(M)),                                               # the stored fallback
            ("one_value_1", b"A"), ("one_value_2", b"AA"),                    # one literal symbol, no distance code
            ("one_distance", b"AB" * 50),                                     # one match, one distance code (an incomplete code of one)
            ("text65279", text[:M - 1]), ("text65280", text[:M]), ("text65281", text[:M + 1]), ("text3m17", text[:3 * M + 17]),
            ("fastq", bi.fastq_text(np.random.default_rng(3), 40)), ("sr.sam", golden_text("sr")), ("hifi.sam", golden_text("hifi"))]
    _cache["inputs"] = out
    return out


def limiter_inputs():
    """[(name, bytes)]: inputs for which gdd_build_lengths has to cut a code to its limit inside a real block (the emulator counts the
    blocks: "cut A B C" of its report).

    clen_limit: 65280 bytes whose even positions are drawn from 60 values with p ~ 0.618^i and whose odd positions walk through 120 others,
    so that few matches form and the literal/length code has a long tail of lengths: in one of its blocks the plain Huffman code over the
    header's symbols is 8 deep, one more than the code-length code may be.

    The limit of 15 was looked for and not found: 4290 inputs of this kind (ratios 0.5 .. 0.72 over 20 .. 120 values, alone or interleaved
    with a walk through 3 .. 120 others; 60 s of emulator runs) gave plain Huffman codes at most 13 deep in both alphabets.  A block holds
    4096 tokens, depth 16 needs at least 2584 of them in near-Fibonacci proportions, and bytes that skewed turn into matches.  The limit
    of 15 stays with test_build_lengths (tests/test_bgzf_deflate.py), which calls the builder on frequencies directly."""
    rng = np.random.default_rng(5)
    p = 0.618 ** np.arange(60)
    a = np.zeros(M, dtype=np.uint8)
    a[0::2] = rng.choice(60, size=M // 2, p=p / p.sum())
    a[1::2] = (130 + 7 * np.arange(M // 2)) % 120
    return [("clen_limit", a.tobytes())]


def member_sizes(z):
    """[(member bytes, ISIZE)] of a BGZF file, walked by BSIZE"""
    out, at = [], 0
    while at < len(z):
        n = int.from_bytes(z[at + 16:at + 18], "little") + 1
        out.append((n, int.from_bytes(z[at + n - 4:at + n], "little")))
        at += n
    assert at == len(z)
    return out


def same_members(got, want, what):
    """two BGZF files are the same bytes; where they are not, the failure names the member"""
    if got != want:
        a, b = member_sizes(got), member_sizes(want)
        assert a == b, (what, [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:5])
        at = 0
        for k, (n, _) in enumerate(a):
            assert got[at:at + n] == want[at:at + n], (what, "member %d" % k)
            at += n
    assert got == want, what
