"""--eqx of the ShortReads variant: mm_update_cigar_eqx (SR/align.c:174-257) restated in Python, the readers of its fixtures
(tests/golden/eqx/, written by tools/make_eqx_golden.py from the reference's own output) and what the tests need around them: the two
windows of a record rebuilt from the read, the strand, the clips and the reference FASTA, the kinds of record a fixture must hold, and
the flat file tests/emul/eqx_emul.cpp reads.
The restatement is pinned by tests/test_eqx.py on every CIGAR the reference printed under --eqx."""
import gzip
import os

import numpy as np

from diffstr_ref import NT4, parse_cigar
from fixture_io import SETS, SR, golden_sam, read_fasta, read_fastq, reads_of

HERE = os.path.dirname(os.path.abspath(__file__))
EQX = os.path.join(HERE, "golden", "eqx")
F_EQX = 0x4000000
# the synthetic set lives under tests/golden/eqx/ with its own reference; it is mapped with sr.cmd
KINDS = ("sr_edge", "sr", "sr_var", "syn")
OPS = "MIDNSHP=X"
# what the fixtures must hold (tools/make_eqx_golden.py prints the counts per set, tests/test_eqx.py asserts them):
#   nn_for / nn_rev  a read N facing a reference N inside an M, on the forward / reverse strand (= there, X here: the reverse-complemented N is 7)
#   count_rule       every M of the record a single run and one of them a mismatch run: the reference labels it = (SR/align.c:212)
#   lead_x           an M of several runs that starts with a mismatch
#   exact            the whole read one = operation
#   diag_x           a single M over the whole read with mismatches in it (the alignment the main-diagonal pre-filter answers)
#   shift            query and target span differ in a square DP box: mm_fix_cigar removed a leading I or D and moved the sequences
KIND_NAMES = ("nn_for", "nn_rev", "count_rule", "lead_x", "exact", "diag_x", "shift")


def dir_of(kind):
    return EQX if kind == "syn" else SETS[kind][0]


def reference_of(kind):
    return read_fasta(os.path.join(EQX, "syn_ref.fa.gz") if kind == "syn" else os.path.join(SR, "ref.fa.gz"))


def reads_of_kind(kind):
    return read_fastq(os.path.join(EQX, "syn.fq.gz")) if kind == "syn" else reads_of(kind)


def plain_sam(kind):
    """the reference's SAM without --eqx: the committed golden (for the synthetic set: tests/golden/eqx/syn.golden.sam.gz)"""
    if kind == "syn":
        return [l.rstrip("\n") for l in gzip.open(os.path.join(EQX, "syn.golden.sam.gz"), "rt")]
    return golden_sam(kind)


def rows(name):
    """tests/golden/eqx/<name>.tsv.gz: one row per line of the reference's output under --eqx"""
    return [l.rstrip("\n").split("\t") for l in gzip.open(os.path.join(EQX, name + ".tsv.gz"), "rt")]


def eqx_sam(kind):
    """the SAM the reference prints under --eqx: the plain lines with column 6 from the fixture"""
    out = []
    plain, rws = plain_sam(kind), rows(kind + ".sam")
    assert len(plain) == len(rws)
    for line, r in zip(plain, rws):
        f = line.split("\t")
        assert (f[0], f[1], f[3]) == (r[0], r[1], r[2]), (kind, f[0])
        f[5] = r[3]
        out.append("\t".join(f))
    return out


def update_cigar_eqx(cigar, q, t):
    """mm_update_cigar_eqx on [(op, len)] and the two code arrays, statement by statement"""
    n_eqx = n_m = qoff = toff = 0
    for op, ln in cigar:
        if op == 0:
            while ln > 0:
                l = 0
                while l < ln and q[qoff + l] == t[toff + l]:
                    l += 1
                if l > 0:
                    n_eqx, ln, toff, qoff = n_eqx + 1, ln - l, toff + l, qoff + l
                l = 0
                while l < ln and q[qoff + l] != t[toff + l]:
                    l += 1
                if l > 0:
                    n_eqx, ln, toff, qoff = n_eqx + 1, ln - l, toff + l, qoff + l
            n_m += 1
        elif op == 1:
            qoff += ln
        elif op in (2, 3):
            toff += ln
    if n_eqx == n_m:  # "update in-place if we can"
        return [(7, ln) if op == 0 else (op, ln) for op, ln in cigar]
    out, qoff, toff = [], 0, 0
    for op, ln in cigar:
        if op == 0:
            while ln > 0:
                l = 0
                while l < ln and q[qoff + l] == t[toff + l]:
                    l += 1
                if l > 0:
                    out.append((7, l))
                ln, toff, qoff = ln - l, toff + l, qoff + l
                l = 0
                while l < ln and q[qoff + l] != t[toff + l]:
                    l += 1
                if l > 0:
                    out.append((8, l))
                ln, toff, qoff = ln - l, toff + l, qoff + l
            continue
        if op == 1:
            qoff += ln
        elif op in (2, 3):
            toff += ln
        out.append((op, ln))
    return out


def cigar_text(cigar):
    return "".join("%d%s" % (ln, OPS[op]) for op, ln in cigar)


def windows(fields, read, contig4):
    """(core CIGAR [(op, len)], clip text in front, clip text behind, query codes, target codes) of a mapped SAM line: the query is the read
    as the DP saw it -- on the reverse strand qs_rev[len - 1 - j] = code ^ 3 (SR/map.c:748,755), an N becomes 7 -- between the clips, the
    target the contig from POS on"""
    cg = parse_cigar(fields[5])
    clip0 = cg[0][1] if cg[0][0] in (4, 5) else 0
    clip1 = cg[-1][1] if len(cg) > 1 and cg[-1][0] in (4, 5) else 0
    core = [(o, n) for o, n in cg if o not in (4, 5)]
    head = "%d%s" % (clip0, OPS[cg[0][0]]) if clip0 else ""
    tail = "%d%s" % (clip1, OPS[cg[-1][0]]) if clip1 else ""
    codes = NT4[np.frombuffer(read.encode(), np.uint8)]
    if int(fields[1]) & 16:
        codes = codes[::-1] ^ 3
    qspan = sum(n for o, n in core if o in (0, 1, 7, 8))
    tspan = sum(n for o, n in core if o in (0, 2, 3, 7, 8))
    assert clip0 + qspan + clip1 == len(read), fields[0]
    pos = int(fields[3]) - 1
    return core, head, tail, codes[clip0:clip0 + qspan], contig4[pos:pos + tspan]


def triples(kind):
    """per mapped line of the kind's plain SAM: (line number, fields, core CIGAR, head, tail, q, t)"""
    names, seqs = reference_of(kind)
    contigs4 = [NT4[np.frombuffer(s.encode(), np.uint8)] for s in seqs]
    reads = {r[0]: r[1] for r in reads_of_kind(kind)}
    out = []
    for i, line in enumerate(plain_sam(kind)):
        f = line.split("\t")
        if f[5] == "*":
            continue
        out.append((i, f) + windows(f, reads[f[0]], contigs4[names.index(f[2])]))
    return out


def kinds_of(kind, eqx_rows):
    """{kind name: number of records}: the plain records of the set against the CIGARs the reference printed under --eqx (eqx_rows)"""
    got = dict.fromkeys(KIND_NAMES, 0)
    for i, f, core, head, tail, q, t in triples(kind):
        new = parse_cigar(eqx_rows[i][3])
        new = [(o, n) for o, n in new if o not in (4, 5)]
        rev = bool(int(f[1]) & 16)
        qo = to = 0
        nn = lead = only_x = False
        single = True
        for op, ln in core:
            if op == 0:
                d = q[qo:qo + ln] != t[to:to + ln]
                nn |= bool(np.any((q[qo:qo + ln] > 3) & (t[to:to + ln] > 3)))
                n_runs = 1 + int(np.count_nonzero(d[1:] != d[:-1]))
                single &= n_runs == 1
                only_x |= n_runs == 1 and bool(d[0])
                lead |= n_runs > 1 and bool(d[0])
                qo, to = qo + ln, to + ln
            elif op == 1:
                qo += ln
            else:
                to += ln
        got["nn_rev" if rev else "nn_for"] += nn
        got["count_rule"] += single and only_x and all(o != 8 for o, _ in new)
        got["lead_x"] += lead
        got["exact"] += len(new) == 1 and new[0][0] == 7 and not head and not tail
        got["diag_x"] += len(core) == 1 and not head and not tail and any(o == 8 for o, _ in new)
        got["shift"] += qo != to
    return got


def write_emul_input(path, trip):
    """the flat text tests/emul/eqx_emul.cpp reads: per record "n_cigar qlen tlen", the CIGAR words, the query codes, the target codes"""
    with open(path, "w") as fh:
        fh.write("%d\n" % len(trip))
        for _, _, core, _, _, q, t in trip:
            fh.write("%d %d %d\n" % (len(core), len(q), len(t)))
            fh.write(" ".join("%d" % (n << 4 | o) for o, n in core) + "\n")
            fh.write(" ".join("%d" % c for c in q) + "\n")
            fh.write(" ".join("%d" % c for c in t) + "\n")
