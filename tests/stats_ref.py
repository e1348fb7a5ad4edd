"""Read and alignment statistics from BAM records: an independent restatement, in Python, of the section "Alignment statistics" of
include/gdiet_hip.h.  Written from that text alone, one base at a time -- nothing here is taken from csrc/; reading a record's fields and
the bad-record reasons, which the section takes from "Coverage", are pile_ref's -- so that the 64-lane statements (csrc/stats.h through
tests/emul/stats_emul.cpp) and the kernel can be compared against it integer for integer.

  stats(data, ref_lens, ref_codes, excl_flags=0x700, min_mapq=0, cycles=512, max_len=65536, max_indel=64) -> Result
      .summary   dict of the 26 counters
      .tables    dict of numpy uint64 arrays, shaped as Stats.finish shapes them
      .bad       None, or (index of the first bad record, reason)
  sam_stats(lines, names, ref_seqs, ...) -> (summary subset, tables)     the second oracle: the columns of SAM text against FASTA letters"""
import re

import numpy as np

import pile_ref as pr

SUMMARY = ("records", "unmapped", "secondary", "supplementary", "primary_mapped", "reverse", "excluded_by_flag", "excluded_by_mapq", "counted", "bad", "duplicate", "qcfail", "reads",
           "read_bases", "aligned_bases", "matches", "mismatches", "other_bases", "ins_events", "ins_bases", "del_events", "del_bases", "soft_clipped", "hard_clipped", "no_seq", "no_identity")
TABLES = ("gc", "base_cycle", "qual_cycle", "base_qual", "mapq", "ins_len", "del_len", "subst", "cmp_cycle", "identity", "read_len")
_CODE = {1: 0, 2: 1, 4: 2, 8: 3}


class Result:
    pass


def empty_tables(cycles, max_len, max_indel):
    z = lambda *shape: np.zeros(shape, np.uint64)
    return dict(gc=z(101), base_cycle=z(cycles + 1, 5), qual_cycle=z(cycles + 1, 2), base_qual=z(96), mapq=z(256), ins_len=z(max_indel + 1), del_len=z(max_indel + 1), subst=z(5, 5),
                cmp_cycle=z(cycles + 1, 2), identity=z(101), read_len=z(max_len + 1))


def _cycle(flag, l_seq, lead, trail, qi):
    return trail + (l_seq - 1 - qi) if flag & 0x10 else lead + qi


def _hard_ends(ops):
    lead = ops[0][1] if ops and ops[0][0] == "H" else 0
    trail = ops[-1][1] if ops and ops[-1][0] == "H" else 0
    return lead, trail


def add_read(T, S, flag, codes, qual, lead, trail, cycles, max_len):
    """one READ: codes are the base codes as stored (0..4), qual the quality bytes or None"""
    l_seq = len(codes)
    S["reads"] += 1
    S["read_bases"] += l_seq
    T["read_len"][min(l_seq, max_len)] += 1
    a = sum(1 for c in codes if c < 4)
    g = sum(1 for c in codes if c in (1, 2))
    if l_seq > 0 and a > 0:
        T["gc"][(200 * g + a) // (2 * a)] += 1
    for qi, c in enumerate(codes):
        row = min(_cycle(flag, l_seq, lead, trail, qi), cycles)
        if flag & 0x10 and c < 4:
            c = 3 - c
        T["base_cycle"][row, c] += 1
        if qual is not None:
            T["qual_cycle"][row, 0] += 1
            T["qual_cycle"][row, 1] += qual[qi]
            T["base_qual"][min(qual[qi], 95)] += 1


def add_alignment(T, S, flag, mapq, pos, ops, codes, ref, lead, trail, cycles, max_indel):
    """one ALIGNMENT: ops = [(letter, length)], codes the base codes as stored, ref the codes of its contig"""
    l_seq = len(codes)
    T["mapq"][mapq] += 1
    r, q, m, x, i, d = pos, 0, 0, 0, 0, 0
    for o, n in ops:
        if o in "M=X":
            if l_seq > 0:
                for k in range(n):
                    rc, fc = codes[q + k], ref[r + k]
                    T["subst"][fc, rc] += 1
                    S["aligned_bases"] += 1
                    if rc < 4 and fc < 4:
                        row = min(_cycle(flag, l_seq, lead, trail, q + k), cycles)
                        T["cmp_cycle"][row, 0] += 1
                        if rc == fc:
                            m += 1
                        else:
                            x += 1
                            T["cmp_cycle"][row, 1] += 1
                    else:
                        S["other_bases"] += 1
            r, q = r + n, q + n
        elif o == "I":
            if n > 0:
                T["ins_len"][min(n, max_indel)] += 1
                S["ins_events"] += 1
                S["ins_bases"] += n
                i += 1
            q += n
        elif o == "D":
            if n > 0:
                T["del_len"][min(n, max_indel)] += 1
                S["del_events"] += 1
                S["del_bases"] += n
                d += 1
            r += n
        elif o == "N":
            r += n
        elif o == "S":
            S["soft_clipped"] += n
            q += n
        elif o == "H":
            S["hard_clipped"] += n
    S["matches"] += m
    S["mismatches"] += x
    den = m + x + i + d
    if den > 0:
        T["identity"][100 * m // den] += 1
    else:
        S["no_identity"] += 1
    if l_seq == 0:
        S["no_seq"] += 1


def stats(data, ref_lens, ref_codes, excl_flags=0x700, min_mapq=0, cycles=512, max_len=65536, max_indel=64):
    assert 1 <= cycles <= 1024 and 1 <= max_len <= 1 << 20 and 1 <= max_indel <= 4096
    T = empty_tables(cycles, max_len, max_indel)
    S = dict.fromkeys(SUMMARY, 0)
    bad = None
    for index, b in enumerate(pr.records(data)):
        f, why = pr._read(b, ref_lens)
        flag = f["flag"]
        S["records"] += 1
        S["unmapped"] += bool(flag & 4)
        S["secondary"] += bool(flag & 0x100)
        S["supplementary"] += bool(flag & 0x800)
        S["primary_mapped"] += not flag & 0x904
        S["reverse"] += bool(flag & 0x10) and not flag & 4
        if why:
            S["bad"] += 1
            bad = bad or (index, why)
            continue
        S["duplicate"] += bool(flag & 0x400)
        S["qcfail"] += bool(flag & 0x200)
        codes = [_CODE.get(n, 4) for n in f["seq"]]
        lead, trail = _hard_ends(f["ops"])
        if not flag & (excl_flags | 0x900):
            add_read(T, S, flag, codes, f["qual"], lead, trail, cycles, max_len)
        if flag & (excl_flags | 4):
            S["excluded_by_flag"] += 1
        elif f["mapq"] < min_mapq:
            S["excluded_by_mapq"] += 1
        elif f["rid"] >= 0:
            S["counted"] += 1
            add_alignment(T, S, flag, f["mapq"], f["pos"], f["ops"], codes, ref_codes[f["rid"]], lead, trail, cycles, max_indel)
    out = Result()
    out.summary, out.tables, out.bad = S, T, bad
    return out


# ---- the second oracle: SAM text against FASTA letters -------------------------------------------------------------------------------------
_OP = re.compile(r"(\d+)([MIDNSHP=X])")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
SAM_COUNTERS = ("reads", "read_bases", "counted", "aligned_bases", "matches", "mismatches", "other_bases", "ins_events", "ins_bases", "del_events", "del_bases", "soft_clipped",
                "hard_clipped", "no_seq", "no_identity")


def sam_stats(lines, names, ref_seqs, excl_flags=0x700, min_mapq=0, cycles=512, max_len=65536, max_indel=64):
    """(dict of SAM_COUNTERS, tables) from the FLAG, RNAME, POS, MAPQ, CIGAR, SEQ and QUAL columns of SAM lines and the letters of the
    reference: letters are compared as letters, the read's cycle is found by turning a reverse read round first"""
    T = empty_tables(cycles, max_len, max_indel)
    S = dict.fromkeys(SAM_COUNTERS, 0)
    letter = lambda ch: "ACGT".find(ch) if ch in "ACGT" else 4
    for l in lines:
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        flag, rname, pos, mapq, cigar, seq, qual = int(f[1]), f[2], int(f[3]) - 1, int(f[4]), f[5], f[9].upper(), f[10]
        seq = "" if seq == "*" else seq
        ops = [(int(n), o) for n, o in _OP.findall("" if cigar == "*" else cigar)]
        lead = ops[0][0] if ops and ops[0][1] == "H" else 0
        trail = ops[-1][0] if ops and ops[-1][1] == "H" else 0
        if not flag & (excl_flags | 0x900):  # a read: in its original orientation, base 0 first
            orig = "".join(_COMP.get(ch, ch) for ch in reversed(seq)) if flag & 16 else seq
            oq = None if qual == "*" or not seq else [ord(ch) - 33 for ch in (reversed(qual) if flag & 16 else qual)]
            first = trail if flag & 16 else lead
            S["reads"] += 1
            S["read_bases"] += len(seq)
            T["read_len"][min(len(seq), max_len)] += 1
            a, g = sum(seq.count(ch) for ch in "ACGT"), seq.count("C") + seq.count("G")
            if a:
                T["gc"][int(np.floor(100.0 * g / a + 0.5))] += 1  # (rounded, halves up: exact in double for these sizes)
            for k, ch in enumerate(orig):
                row = min(first + k, cycles)
                T["base_cycle"][row, letter(ch)] += 1
                if oq is not None:
                    T["qual_cycle"][row, 0] += 1
                    T["qual_cycle"][row, 1] += oq[k]
                    T["base_qual"][min(oq[k], 95)] += 1
        if flag & (excl_flags | 4) or mapq < min_mapq or rname == "*":
            continue
        S["counted"] += 1
        T["mapq"][mapq] += 1
        ref = ref_seqs[list(names).index(rname)].upper()
        r, q, m, x, i, d = pos, 0, 0, 0, 0, 0
        for n, o in ops:
            if o in "M=X":
                for k in range(n if seq else 0):
                    a, b = ref[r + k], seq[q + k]
                    T["subst"][letter(a), letter(b)] += 1
                    S["aligned_bases"] += 1
                    if a in "ACGT" and b in "ACGT":
                        cyc = trail + (len(seq) - 1 - (q + k)) if flag & 16 else lead + q + k
                        T["cmp_cycle"][min(cyc, cycles), 0] += 1
                        m += a == b
                        x += a != b
                        T["cmp_cycle"][min(cyc, cycles), 1] += a != b
                    else:
                        S["other_bases"] += 1
                r, q = r + n, q + n
            elif o in "ID" and n > 0:
                T["ins_len" if o == "I" else "del_len"][min(n, max_indel)] += 1
                S["ins_events" if o == "I" else "del_events"] += 1
                S["ins_bases" if o == "I" else "del_bases"] += n
                i, d = i + (o == "I"), d + (o == "D")
                r, q = r + (n if o == "D" else 0), q + (n if o == "I" else 0)
            elif o == "N":
                r += n
            elif o == "S":
                S["soft_clipped"] += n
                q += n
            elif o == "H":
                S["hard_clipped"] += n
        S["matches"] += m
        S["mismatches"] += x
        if m + x + i + d:
            T["identity"][100 * m // (m + x + i + d)] += 1
        else:
            S["no_identity"] += 1
        S["no_seq"] += not seq
    return S, T


def stats_tsv(summary, tables):
    """the text of <prefix>.stats.tsv, formed here from the integers"""
    ratio = lambda num, den, fmt="%.6g": fmt % (int(num) / int(den)) if int(den) else "0"
    out = ["# gdiet-hip alignment statistics.  Sections: SN summary, RL read lengths, GCF GC content, GCC base composition per cycle, QC quality per cycle, BQ base qualities,",
           "# MQ mapping qualities, IL / DL insertion / deletion lengths, SUB substitutions (reference base, read base), MPC mismatches per cycle, IDN identity per alignment.",
           "# A per-cycle table's last row takes every later cycle; the last bin of RL, IL and DL every longer length."]
    out += ["SN\t%s:\t%d" % (k, summary[k]) for k in SUMMARY]
    out.append("SN\terror_rate:\t" + ratio(summary["mismatches"], summary["matches"] + summary["mismatches"]))
    out.append("SN\taverage_length:\t" + ratio(summary["read_bases"], summary["reads"]))
    qc = tables["qual_cycle"]
    out.append("SN\taverage_quality:\t" + ratio(sum(int(v) for v in qc[:, 1]), sum(int(v) for v in qc[:, 0]), "%.4g"))
    for tag, name in (("RL", "read_len"), ("GCF", "gc")):
        out += ["%s\t%d\t%d" % (tag, k, int(v)) for k, v in enumerate(tables[name]) if int(v)]
    out += ["GCC\t%d\t%s" % (k + 1, "\t".join(str(int(v)) for v in row)) for k, row in enumerate(tables["base_cycle"]) if any(int(v) for v in row)]
    out += ["QC\t%d\t%s\t%d" % (k + 1, ratio(row[1], row[0], "%.4g"), int(row[0])) for k, row in enumerate(qc) if int(row[0])]
    for tag, name in (("BQ", "base_qual"), ("MQ", "mapq"), ("IL", "ins_len"), ("DL", "del_len")):
        out += ["%s\t%d\t%d" % (tag, k, int(v)) for k, v in enumerate(tables[name]) if int(v)]
    out += ["SUB\t%s\t%s\t%d" % ("ACGTN"[r], "ACGTN"[c], int(tables["subst"][r, c])) for r in range(5) for c in range(5)]
    out += ["MPC\t%d\t%d\t%d" % (k + 1, int(row[1]), int(row[0])) for k, row in enumerate(tables["cmp_cycle"]) if int(row[0])]
    out += ["IDN\t%d\t%d" % (k, int(v)) for k, v in enumerate(tables["identity"]) if int(v)]
    return "\n".join(out) + "\n"
