"""readers and shared definitions of the SAM / PAF output-option fixtures (tests/golden/samopts/, written by tools/make_samopts_golden.py
with the reference's own binaries): -Y, --sam-hit-only, -Q, -y, -R and all of them together on hifi_sv, ont_sv and sr; -y in PAF.

  <kind>.<mode>.sam.gz   the reference's whole standard output under the mode: header lines verbatim, body lines with SEQ and QUAL
                         stored as "#<length>:<sha1>" ("*" stays "*")
  <kind>.paf_y.paf.gz    its PAF under fixture_io.paf_cmd_of plus -y, verbatim
The reads are those of fixture_io.reads_of with a comment on two of every three (comment_of), the comment holding a tab as the MM / ML
methylation tags of a real FASTQ header do."""
import gzip
import hashlib
import os

from fixture_io import cmd_of, paf_cmd_of, reads_of

SAMOPTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samopts")
KINDS = ("hifi_sv", "ont_sv", "sr")
PAF_KINDS = ("hifi_sv", "sr")
# the -R argument as typed: backslash-t twice, a doubled backslash (one backslash), and backslash-q (both characters vanish)
RG_ARG = "@RG\\tID:grp1\\tSM:s\\\\x\\qz"
RG_LINE = "@RG\tID:grp1\tSM:s\\xz"  # what mm_escape makes of it
RG_ID = "grp1"
MODES = {"Y": ["-Y"], "hit": ["--sam-hit-only"], "Q": ["-Q"], "y": ["-y"], "R": ["-R", RG_ARG], "all": ["-Y", "-y", "-R", RG_ARG, "--sam-hit-only"]}
F_NO_QUAL, F_LONG_CIGAR, F_SOFTCLIP, F_COPY_COMMENT, F_SAM_HIT_ONLY = 0x10, 0x10000, 0x80000, 0x2000000, 0x40000000
MODE_FLAG = {"Y": F_SOFTCLIP, "hit": F_SAM_HIT_ONLY, "Q": F_NO_QUAL, "y": F_COPY_COMMENT, "R": 0, "all": F_SOFTCLIP | F_COPY_COMMENT | F_SAM_HIT_ONLY}
MODE_RG = {"R", "all"}
VERSION = "1.0-r1"  # MM_VERSION of both trees (LR/main.c:11)
THREADS = ["-t", "4"]


def comment_of(i):
    """the comment of read i of a set: none on every third read"""
    return None if i % 3 == 2 else "MM:Z:C+m,%d;\tML:B:C,%d" % (i, i % 256)


def reads_with_comments(kind):
    """[(qname, seq, qual, comment or None)]"""
    return [r + (comment_of(i),) for i, r in enumerate(reads_of(kind))]


def ref_argv(kind, mode):
    """the reference's argv under the mode (argv[0] is not printed); it runs in a directory that holds ref.fa and reads.fq"""
    extra = ["-y"] if mode == "paf_y" else MODES[mode]
    return ["minimap2"] + THREADS + (paf_cmd_of(kind) if mode == "paf_y" else cmd_of(kind)) + extra + ["ref.fa", "reads.fq"]


def digest(text):
    return text if text == "*" else "#%d:%s" % (len(text), hashlib.sha1(text.encode()).hexdigest())


def digest_line(line):
    """a SAM line as the fixtures hold it: header lines as they are, SEQ and QUAL of a record digested"""
    if line.startswith("@"):
        return line
    f = line.split("\t")
    f[9], f[10] = digest(f[9]), digest(f[10])
    return "\t".join(f)


def golden(kind, mode):
    """(header lines, digested body lines) of <kind>.<mode>.sam.gz"""
    lines = gzip.open(os.path.join(SAMOPTS, "%s.%s.sam.gz" % (kind, mode)), "rt").read().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    n_hdr = next((i for i, l in enumerate(lines) if not l.startswith("@")), len(lines))
    assert not any(l.startswith("@") for l in lines[n_hdr:])  # (no QNAME of these sets starts with @)
    return lines[:n_hdr], lines[n_hdr:]


def golden_paf_y(kind):
    return gzip.open(os.path.join(SAMOPTS, "%s.paf_y.paf.gz" % kind), "rt").read().split("\n")[:-1]
