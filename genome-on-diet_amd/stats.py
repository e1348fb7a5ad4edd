"""Read and alignment statistics accumulated on the device: ``Stats`` over the library's accumulator (``gdiet_hip_stats_*``,
csrc/stats_driver.hip.h; what it shares with ``Coverage`` and ``Pileup`` is in accum.py).  The records of every batch are walked where
they are resident (csrc/stats.hip.h: one wavefront per record, the histograms summed per block in local memory and flushed with 64-bit
adds); ``finish`` only copies the tables down.  The rules are the section "Alignment statistics" of include/gdiet_hip.h.  The whole state
is a few tens of kilobytes (plus 8 bytes per read-length bin), so the accumulator can be on in every run.  The tables of disjoint sets of
records -- of several runs, or of several GPUs -- simply add."""
import ctypes as C

import numpy as np

from .accum import Accumulator
from .hip_abi import bind_stats, load_library

SUMMARY = ("records", "unmapped", "secondary", "supplementary", "primary_mapped", "reverse", "excluded_by_flag", "excluded_by_mapq", "counted", "bad", "duplicate", "qcfail", "reads",
           "read_bases", "aligned_bases", "matches", "mismatches", "other_bases", "ins_events", "ins_bases", "del_events", "del_bases", "soft_clipped", "hard_clipped", "no_seq", "no_identity")
TABLES = ("gc", "base_cycle", "qual_cycle", "base_qual", "mapq", "ins_len", "del_len", "subst", "cmp_cycle", "identity", "read_len")  # GDIET_STATS_*: the order of the header
SHAPES = dict(base_cycle=5, qual_cycle=2, subst=5, cmp_cycle=2)  # the row width of the tables that have rows
CODES = "ACGTN"


def tsv(summary, tables):
    """the text of ``<prefix>.stats.tsv`` from a summary dict and the tables: sections whose lines start with a tag, as `samtools stats`
    writes them.  Every integer is the device's; the ratios are formed here, in double."""
    ratio = lambda num, den, fmt="%.6g": fmt % (int(num) / int(den)) if int(den) else "0"
    out = ["# gdiet-hip alignment statistics.  Sections: SN summary, RL read lengths, GCF GC content, GCC base composition per cycle, QC quality per cycle, BQ base qualities,",
           "# MQ mapping qualities, IL / DL insertion / deletion lengths, SUB substitutions (reference base, read base), MPC mismatches per cycle, IDN identity per alignment.",
           "# A per-cycle table's last row takes every later cycle; the last bin of RL, IL and DL every longer length."]
    out += ["SN\t%s:\t%d" % (k, summary[k]) for k in SUMMARY]
    out.append("SN\terror_rate:\t" + ratio(summary["mismatches"], summary["matches"] + summary["mismatches"]))
    out.append("SN\taverage_length:\t" + ratio(summary["read_bases"], summary["reads"]))
    qc = tables["qual_cycle"]
    out.append("SN\taverage_quality:\t" + ratio(qc[:, 1].sum(dtype=np.uint64), qc[:, 0].sum(dtype=np.uint64), "%.4g"))
    hist = lambda tag, t: ["%s\t%d\t%d" % (tag, k, int(v)) for k, v in enumerate(t) if int(v)]
    out += hist("RL", tables["read_len"]) + hist("GCF", tables["gc"])
    out += ["GCC\t%d\t%s" % (k + 1, "\t".join(str(int(v)) for v in row)) for k, row in enumerate(tables["base_cycle"]) if row.any()]
    out += ["QC\t%d\t%s\t%d" % (k + 1, ratio(row[1], row[0], "%.4g"), int(row[0])) for k, row in enumerate(qc) if row[0]]
    out += hist("BQ", tables["base_qual"]) + hist("MQ", tables["mapq"]) + hist("IL", tables["ins_len"]) + hist("DL", tables["del_len"])
    out += ["SUB\t%s\t%s\t%d" % (CODES[r], CODES[c], int(tables["subst"][r, c])) for r in range(5) for c in range(5)]
    out += ["MPC\t%d\t%d\t%d" % (k + 1, int(row[1]), int(row[0])) for k, row in enumerate(tables["cmp_cycle"]) if row[0]]
    out += hist("IDN", tables["identity"])
    return "\n".join(out) + "\n"


class Stats(Accumulator):
    """``Stats(mapper, excl_flags=0x700, min_mapq=0, cycles=512, max_len=65536, max_indel=64)``.  Records come in through ``add`` (a mapped
    batch: the arguments of ``Mapper.bam_batch_raw``; encoded and scattered on the device, nothing comes down), ``add_bam`` (bytes of
    uncompressed BAM records) or an attached ``BgzfWriter`` / ``BamSorter`` (``set_stats``).  ``finish()`` returns (summary dict, tables
    dict of numpy uint64 arrays: gc[101], base_cycle[cycles + 1, 5], qual_cycle[cycles + 1, 2] (count, sum), base_qual[96], mapq[256],
    ins_len / del_len[max_indel + 1], subst[5, 5] (reference, read), cmp_cycle[cycles + 1, 2] (comparable, mismatches), identity[101],
    read_len[max_len + 1]); ``write(prefix)`` prints them.  A bad record raises ``GdietError`` and leaves the object refusing everything
    but ``close``.  Keep the mapper open while the object is used.  The tables of disjoint record sets simply add.  ``_bound`` is
    ``gdiet_hip_stats_open_bounded``'s: the weight a block holds in local memory between two flushes (0: the default); no result depends
    on it, tests lower it."""
    _prefix, _name = "stats", "Stats"

    def __init__(self, mapper, excl_flags=0x700, min_mapq=0, cycles=512, max_len=65536, max_indel=64, _bound=0):
        self.lib = load_library()
        bind_stats(self.lib)
        self.mapper = mapper
        self._h = C.c_void_p()
        self._result = None
        self._check(self.lib.gdiet_hip_stats_open_bounded(mapper.ctx._h, mapper._idx, int(excl_flags), int(min_mapq), int(cycles), int(max_len), int(max_indel), int(_bound),
                                                          C.byref(self._h)))

    def finish(self):
        """(summary, tables)"""
        self._open()
        summary = (C.c_uint64 * len(SUMMARY))()
        self._check(self.lib.gdiet_hip_stats_finish(self._h, summary))
        tables = {}
        for which, name in enumerate(TABLES):
            n = self._check(self.lib.gdiet_hip_stats_table(self._h, which, None, 0))
            t = np.zeros(n, np.uint64)
            self._check(self.lib.gdiet_hip_stats_table(self._h, which, t.ctypes.data, n))
            tables[name] = t.reshape(-1, SHAPES[name]) if name in SHAPES else t
        self._result = (dict(zip(SUMMARY, (int(x) for x in summary))), tables)
        return self._result

    def write(self, prefix):
        """``<prefix>.stats.tsv``: the sections SN RL GCF GCC QC BQ MQ IL DL SUB MPC IDN, every line starting with its tag"""
        summary, tables = self._result if self._result is not None else self.finish()
        with open(str(prefix) + ".stats.tsv", "w") as f:
            f.write(tsv(summary, tables))
