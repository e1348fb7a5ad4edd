"""inputs of the device-reader tests (tests/test_fastx_device.py on the CPU emulator, tests/test_fastx_device_gpu.py on the GPU)"""
import numpy as np


def sweep_file():
    """Strict four-line FASTQ that sweeps the geometry of the device passes (16-byte lanes, 1 KiB tiles): reads of every length 1..70 and
    1000..1100; header lengths varied, every tenth header padded so that its newline is the last byte of a tile or the first byte of the
    next one; quality lines that start with '@' and '+'; names followed by a space and a comment, a tab and a comment, nothing, or a
    space and nothing; U, u, lower case and N in sequences, U in qualities.  Returns (bytes, number of records)."""
    rng = np.random.default_rng(77)
    out, size, n = [], 0, 0
    edge = 0
    for i, ln in enumerate(list(range(1, 71)) + list(range(1000, 1101))):
        alphabet = b"ACGTacgtUuN" if i % 3 == 0 else b"ACGT"
        s = bytearray(rng.choice(list(alphabet), size=ln).tolist())
        if s[0] in b"@+>":  # (never, with these alphabets)
            s[0] = ord("A")
        q = bytearray(rng.integers(35, 74, size=ln, dtype=np.uint8).tolist())
        q[0] = (ord("@"), ord("+"), ord("U"), q[0])[i % 4]
        if ln > 2:
            q[ln // 2] = ord("U")
        name = b"s%d" % i + b"x" * (i * 7 % 23)
        tail = (b" c=%d more" % i, b"\tt%d" % i, b"", b" ")[i % 4]
        if i % 10 == 0:  # the header's newline on a tile edge: offset = 1023 or 0 (mod 1024), in turn
            want = (1023, 0)[edge % 2]
            edge += 1
            at = size + 1 + len(name) + len(tail)  # where the newline would fall
            name += b"y" * ((want - at) % 1024)
        rec = b"@" + name + tail + b"\n" + bytes(s) + b"\n+\n" + bytes(q) + b"\n"
        out.append(rec)
        size += len(rec)
        n += 1
    return b"".join(out), n


def newline_geometry(data):
    """(residues mod 16 of the newline offsets, residues mod 1024)"""
    pos = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    return set((pos % 16).tolist()), set((pos % 1024).tolist())


def mixed_file():
    """the mixed file of tests/test_fastx_reader.py::test_parallel_parse_equals_sequential_parse, by the same recipe: strict four-line
    FASTQ whose quality lines start with '@' and '+', with zones of multi-line FASTQ, Windows line ends and FASTA, and one malformed
    record.  6000 records, one batch closed early."""
    rng = np.random.default_rng(5)
    parts = []
    for i in range(6000):
        n = int(rng.integers(20, 300))
        s = bytes(rng.choice(list(b"ACGT"), size=n).tolist())
        q = bytearray(rng.integers(35, 74, size=n, dtype=np.uint8).tolist())
        if i % 3 == 0:
            q[0] = ord("@")
        if i % 5 == 0:
            q[0] = ord("+")
        zone = (i // 500) % 6
        if zone == 2 and n > 80:  # multi-line
            parts.append(b"@ml%d x\n" % i + s[:40] + b"\n" + s[40:] + b"\n+\n" + bytes(q[:40]) + b"\n" + bytes(q[40:]) + b"\n")
        elif zone == 3:
            parts.append(b"@cr%d\r\n" % i + s + b"\r\n+\r\n" + bytes(q) + b"\r\n")
        elif zone == 4:
            parts.append(b">fa%d some text\n" % i + s + b"\n")
        else:
            parts.append(b"@r%d c=%d\n" % (i, i) + s + b"\n+\n" + bytes(q) + b"\n")
        if i == 2750:
            parts.append(b"@broken\nACGTACGT\n+\nIII\n")
    return b"".join(parts)


def strict_prefix(data):
    """the line-based restatement of the strict-record predicate over a whole file: the number of leading strict records"""
    lines = data.split(b"\n")
    complete = len(lines) - 1  # (the piece behind the last newline is not a complete line)
    n = 0
    while 4 * n + 3 < complete:
        h, s, p, q = lines[4 * n:4 * n + 4]
        if not (h[:1] == b"@" and p[:1] == b"+" and len(s) == len(q) >= 1 and s[:1] not in (b"@", b"+", b">") and not any(b"\r" in x for x in (h, s, p, q))):
            break
        n += 1
    return n
