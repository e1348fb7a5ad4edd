"""Steps 0-2 of the reference's worker_pipeline through the library: FASTA/FASTQ or unaligned BAM file -> mini-batches (gdiet_hip_fastx_read) ->
map with several batches in flight (gdiet_hip_map_submit / _wait) -> SAM records (gdiet_hip_sam_batch) -> output file.
No Python object is made per read: the C arrays of the reader go straight into the upload and the SAM formatter.

    python tools/map_file.py --preset sr ref.fa[.gz] | ref.mmi reads.fq[.gz] | reads.bam -o out.sam [-K 39321600] [--inflight 3] [--reader-threads 4] [--MD | --cs[=short|long]]
                             [-d out.mmi] [--header] [-R '@RG\tID:x\tSM:y'] [-Y] [-L] [-y] [-Q] [--sam-hit-only] [--device-reader]
                             [--bgzf {host,device}] [--bgzf-level N] [--bgzf-threads N] [--bam [--sort [--index] [--markdup] [--sort-mem BYTES] [--tmp-dir DIR]]] [--sam-device]
                             [--coverage PREFIX [--cov-window N] [--cov-min-mapq Q] [--cov-excl-flags F]]
                             [--pileup PREFIX [--pile-regions BED] [--pile-min-baseq Q] [--pile-min-mapq Q] [--pile-excl-flags F] [--pile-min-depth N] [--pile-min-alt N] [--pile-frac NUM/DEN]]
                             [--stats PREFIX [--stats-cycles N] [--stats-max-len N] [--stats-max-indel N] [--stats-min-mapq Q] [--stats-excl-flags F]]

`ref` is a FASTA / FASTQ file (plain, gzip or BGZF) or an .mmi index file, known by its magic, not its name (Mapper.from_file:
gdiet_hip_index_open -- FASTA blocks are parsed on the device); "synth:MBP" stands for bench.py's synthetic reference.  -d FILE dumps
the index to FILE after the build, as the reference's -d does; FILE can be the `ref` of a later run.  The JSON line gains ref_open.
Writes the SAM body (the records).  --header puts the header lines of the reference's CLI in front (gdiet_hip_sam_header: @SQ per
contig, the @RG line of -R, @PG with this tool's version and command line); it is opt-in, so that the default output stays the body alone.
-R, -Y, -L, -y, -Q and --sam-hit-only mean what they mean to the reference (LR/main.c): a read group on every record, soft clips and
whole reads on supplementary records, long CIGARs in the CG tag, the FASTQ comment as the last field (read with with_comment), no
qualities (not even read: with_qual off), no record for an unmapped read.
--device-reader attaches the reader to the context (gdiet_hip_fastx_attach): four-line FASTQ is parsed and encoded on the device, the
reader hands out resident batches, and the upload stage disappears; the output is the same, and the JSON line gains reader_stats.
A BAM file is read like FASTQ, with no option: the reader sees BAM\1 at the start of the decompressed stream (reads_format in the JSON
line says "bam").  Its records' aux fields are the comment -y copies; with --device-reader SEQ and QUAL are unpacked by the device.
--bgzf writes -o, the --header text included, as BGZF (BgzfWriter): `device` compresses every member of 65280 bytes on one wavefront of
the GPU, `host` with zlib at --bgzf-level on --bgzf-threads threads; the JSON line gains bgzf_out.  Without it nothing changes.
--bam writes -o as BAM: the header always (gdiet_hip_bam_header), then the records of every batch, encoded on the device
(gdiet_hip_bgzf_out_write_bam), in the BGZF container --bgzf picks (default `device`: the records are compressed where they were
encoded and only compressed members come back; `host`: they come back and go through zlib).  Every output option keeps its meaning;
a -y comment must be a list of SAM tags, or the run fails.  The JSON line gains bam_device_seconds.
--sam-device formats the SAM lines on the device (gdiet_hip_sam_batch_device_into; the same bytes as without it): to a plain -o the text
comes down and is written; with --bgzf device the lines are written behind the writer's tail and compressed where they are
(gdiet_hip_bgzf_out_write_sam), so only compressed members reach the host.  It does not go with --bam.
--bam --sort writes -o in coordinate order (BamSorter: every batch is encoded into a resident run buffer, a run of --sort-mem bytes is
sorted on the device and spooled to an unnamed file in --tmp-dir, default the output's directory, and the runs are merged on the device
at the end); the header then starts with @HD VN:1.6 SO:coordinate.  --index writes <out>.bai as well.  The JSON line gains bam_sort.
--markdup (with --bam --sort) marks duplicate reads in the sorted file: bit 0x400, decided on the device over the whole file before its
first chunk is written (include/gdiet_hip.h, "Duplicate marking"); bam_sort gains "dup".  An accumulator attached to the sorter (--coverage,
--pileup) reads the records before they are flagged and so still counts duplicates.  Without --sort nothing changes.
--coverage PREFIX accumulates per-contig coverage and depth on the device (Coverage: 4 bytes of device memory per reference base) and
writes PREFIX.coverage.tsv, and PREFIX.regions.bed with --cov-window N.  With --bam --sort, or --bam --bgzf device, the accumulator is
attached to the sorter or the writer and reads the records they have just encoded; otherwise (SAM output, or unsorted --bgzf host) the writer thread
calls Coverage.add on every batch, which encodes the batch's BAM records on the device for the accumulator alone.  The output file does
not change.  The JSON line gains coverage.  Without --coverage nothing changes.
--pileup PREFIX piles up base counts per position on the device (Pileup: 32 bytes of device memory per position) over the regions of
--pile-regions BED (contig, 0-based start, end; sorted as the contigs are and disjoint; default: every contig whole) and writes
PREFIX.pileup.tsv, the variant sites under --pile-min-depth / --pile-min-alt / --pile-frac, and PREFIX.consensus.fa.  It attaches exactly as
--coverage does and may be combined with it.  The JSON line gains pileup.  Without --pileup nothing changes.
--stats PREFIX collects read and alignment statistics on the device (Stats: a few tens of kilobytes of device memory, whatever the
reference) and writes PREFIX.stats.tsv, the summary and histograms of `samtools flagstat` / `samtools stats` in tagged sections (SN RL
GCF GCC QC BQ MQ IL DL SUB MPC IDN), with --stats-cycles rows per per-cycle table, read lengths up to --stats-max-len and indel lengths
up to --stats-max-indel.  It attaches exactly as --coverage does and may be combined with it and with --pileup; with --markdup it still
counts the duplicates (it reads the records before they are flagged).  The JSON line gains stats.  Without --stats nothing changes."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime for torch and libgdiet_hip.so)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import _load_pkg  # noqa: E402


VERSION = "gdiet-hip-map_file"  # the VN: field of --header's @PG line


def map_file(pkg, mapper, reads_path, out, chunk, inflight, reader_threads, with_qual=True, with_comment=False, device_reader=False, bam=False, sorter=None, sam_device=False,
             cov_add=None, pile_add=None, stats_add=None):
    """returns (reads, seconds).  Three stages on three threads, as the reference's kt_pipeline runs its three steps (LR/map.c:2094-2170):
    read -> upload + submit -> wait + format + write; the C calls release the interpreter lock, so the stages overlap.
    A failure in any stage stops all three: `stop` is set, the writer keeps draining q_done (every open ticket is still waited for and
    its permit, batch and reader arena released -- the lanes would otherwise keep running against the context), the reader and the
    submitting loop give up at their next queue operation, and the first error is raised once the threads have ended."""
    import queue
    import threading
    fx = pkg.FastxReader(reads_path, threads=reader_threads, ctx=mapper.ctx if device_reader else None)
    mapper.set_inflight(inflight)
    T = {"read": 0.0, "upload": 0.0, "submit": 0.0, "wait": 0.0, "sam+write": 0.0, "free": 0.0, **({"coverage": 0.0} if cov_add is not None else {}), **({"pileup": 0.0} if pile_add is not None else {}),
         **({"stats": 0.0} if stats_add is not None else {})}
    q_read, q_done = queue.Queue(maxsize=2), queue.Queue()
    open_tickets = threading.Semaphore(inflight)  # the library takes at most `inflight` tickets: one permit per open ticket
    errors, stop = [], threading.Event()
    t0 = time.perf_counter()

    def timed(key, f, *a, **k):
        t = time.perf_counter()
        r = f(*a, **k)
        T[key] += time.perf_counter() - t
        return r

    def fail(e):
        errors.append(e)
        stop.set()

    def put(q, item):
        """q.put that gives up once the pipeline is stopping; False = not queued"""
        while not stop.is_set():
            try:
                q.put(item, timeout=0.2)
                return True
            except queue.Full:
                pass
        return False

    def drop_item(item):
        """a batch of the reader that nobody is going to map"""
        if item[0]:
            if device_reader and item[7] is not None:
                mapper.free_batch(item[7])
            fx.release(item[6])

    def reader():
        try:
            while not stop.is_set():
                item = timed("read", fx.read_raw, chunk, with_qual=with_qual, with_comment=with_comment, detach=True, resident=device_reader)
                if not put(q_read, item):
                    drop_item(item)
                    return
                if item[0] == 0:
                    return
        except Exception as e:  # noqa: BLE001
            fail(e)

    def writer():
        while True:
            item = q_done.get()
            if item is None:
                return
            ticket, token, n, names, seqs, quals, lens, batch, comments = item
            res = None
            try:  # the ticket is waited for whatever happened before: only then is its lane idle
                res = timed("wait", mapper.wait, ticket)
            except Exception as e:  # noqa: BLE001
                fail(e)
            open_tickets.release()
            try:
                if res is not None and not stop.is_set() and sorter is not None:
                    timed("sam+write", sorter.add, res, n, names, seqs, quals, lens, comments if with_comment else None)
                elif res is not None and not stop.is_set():
                    timed("sam+write", mapper.bam_batch_raw if bam else mapper.sam_batch_raw, res, n, names, seqs, quals, lens, out, comments if with_comment else None,
                          *([True] if sam_device and not bam else []))
                if res is not None and not stop.is_set() and cov_add is not None:  # (an accumulator that is not attached to the writer or the sorter)
                    timed("coverage", cov_add.add, res, n, names, seqs, quals, lens, comments if with_comment else None)
                if res is not None and not stop.is_set() and pile_add is not None:
                    timed("pileup", pile_add.add, res, n, names, seqs, quals, lens, comments if with_comment else None)
                if res is not None and not stop.is_set() and stats_add is not None:
                    timed("stats", stats_add.add, res, n, names, seqs, quals, lens, comments if with_comment else None)
            except Exception as e:  # noqa: BLE001
                fail(e)
            try:
                def drop():
                    nonlocal res
                    res = None
                    mapper.free_batch(batch)
                    fx.release(token)
                timed("free", drop)
            except Exception as e:  # noqa: BLE001
                fail(e)

    th_r, th_w = threading.Thread(target=reader), threading.Thread(target=writer)
    th_r.start(), th_w.start()
    n_reads = 0
    try:
        while not stop.is_set():
            try:
                item = q_read.get(timeout=0.2)
                n, names, comments, seqs, quals, lens, token = item[:7]
            except queue.Empty:
                if not th_r.is_alive() and q_read.empty():
                    break  # the reader ended without its end-of-file item: it failed
                continue
            if n == 0:
                break
            n_reads += n
            batch = item[7] if device_reader else None  # (the reader's resident batch: nothing to encode or copy here)
            try:
                if not device_reader:
                    batch = timed("upload", mapper.upload_raw, n, seqs, lens)
                while not open_tickets.acquire(timeout=0.2):
                    if stop.is_set():
                        raise RuntimeError("pipeline stopped")
                try:
                    ticket = timed("submit", mapper.submit, batch)
                except Exception:
                    open_tickets.release()
                    raise
                q_done.put((ticket, token, n, names, seqs, quals, lens, batch, comments))
            except Exception as e:  # noqa: BLE001
                if batch is not None:
                    mapper.free_batch(batch)
                fx.release(token)
                if not stop.is_set() or not errors:
                    fail(e)
                break
    finally:
        stop_was_set = stop.is_set()
        q_done.put(None)  # the writer drains what is queued before it, then ends
        if stop_was_set:  # unblock a reader waiting on a full queue
            while True:
                try:
                    drop_item(q_read.get_nowait())
                except queue.Empty:
                    break
        th_w.join()
        stop.set()  # (nothing is left to do: a reader that has not reached the end of the file stops here)
        th_r.join()
        map_file.last_reader_stats = fx.stats()
        map_file.last_bgzf_stats = fx.bgzf_stats()
        map_file.last_format = fx.format()
        fx.close()
    if errors:
        raise errors[0]
    map_file.last_stage_seconds = {k: round(v, 3) for k, v in T.items()}
    return n_reads, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ref")
    ap.add_argument("reads")
    ap.add_argument("-o", "--out", default="/dev/null")
    ap.add_argument("--preset", default="hifi", choices=["hifi", "ont", "sr"])
    ap.add_argument("-K", type=int, default=0, help="bases per mini-batch (default: 39321600 for sr = 262144 reads of 150, 80e6 for long reads)")
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--reader-threads", type=int, default=4)
    ap.add_argument("--MD", action="store_true", help="MD:Z: tag on every record with a CIGAR (MM_F_OUT_MD)")
    ap.add_argument("--cs", nargs="?", const="short", choices=["short", "long"], help="cs:Z: tag (MM_F_OUT_CS; long: MM_F_OUT_CS_LONG as well); with --MD, MD is printed")
    ap.add_argument("--eqx", action="store_true", help="=/X in place of M in every CIGAR (MM_F_EQX); --preset sr only, as in the reference's ShortReads tree")
    ap.add_argument("--header", action="store_true", help="write the SAM header (@SQ, @RG, @PG) in front of the records")
    ap.add_argument("-R", dest="rg", metavar="LINE", help="read group line, tabs spelled \\t: '@RG\\tID:x\\tSM:y' (RG:Z: on every record; @RG under --header)")
    ap.add_argument("-Y", dest="softclip", action="store_true", help="soft clipping and whole-read SEQ/QUAL on supplementary and secondary records (MM_F_SOFTCLIP)")
    ap.add_argument("-L", dest="long_cigar", action="store_true", help="CIGARs of more than 65535 operations go to the CG:B:I tag (MM_F_LONG_CIGAR)")
    ap.add_argument("-y", dest="copy_comment", action="store_true", help="copy the FASTA/FASTQ comment to the end of each record (MM_F_COPY_COMMENT)")
    ap.add_argument("-Q", dest="no_qual", action="store_true", help="no base qualities: QUAL is * (MM_F_NO_QUAL)")
    ap.add_argument("--sam-hit-only", action="store_true", help="no record for a read without an alignment (MM_F_SAM_HIT_ONLY)")
    ap.add_argument("--bgzf", choices=["host", "device"], help="write -o as BGZF: members compressed by zlib on host threads, or on the device (one wavefront per member)")
    ap.add_argument("--bgzf-level", type=int, default=-1, help="zlib level of --bgzf host (-1: zlib's default)")
    ap.add_argument("--bgzf-threads", type=int, default=4, help="host threads of --bgzf host")
    ap.add_argument("--bam", action="store_true", help="write -o as BAM (header always; records encoded on the device); --bgzf picks the compressor, default device")
    ap.add_argument("--sam-device", action="store_true", help="format the SAM lines on the device (sam_encode_kernel); with --bgzf device they are compressed where they were written")
    ap.add_argument("--sort", action="store_true", help="with --bam: write the records in coordinate order (sorted and merged on the device; header with @HD SO:coordinate)")
    ap.add_argument("--index", action="store_true", help="with --bam --sort: write <out>.bai as well")
    ap.add_argument("--markdup", action="store_true", help="with --bam --sort: mark duplicate reads (bit 0x400), decided on the device over the whole sorted file")
    ap.add_argument("--sort-mem", type=int, default=1 << 29, metavar="BYTES", help="bytes of records per sorted run (default 512 MiB)")
    ap.add_argument("--tmp-dir", metavar="DIR", help="where the runs are spooled (unnamed files; default: the directory of -o)")
    ap.add_argument("--coverage", metavar="PREFIX", help="accumulate coverage and depth on the device; writes PREFIX.coverage.tsv (and PREFIX.regions.bed with --cov-window)")
    ap.add_argument("--cov-window", type=int, default=0, metavar="N", help="with --coverage: mean depth per window of N bases")
    ap.add_argument("--cov-min-mapq", type=int, default=0, metavar="Q", help="with --coverage: records with a lower MAPQ are not counted")
    ap.add_argument("--cov-excl-flags", type=lambda x: int(x, 0), default=0x704, metavar="F", help="with --coverage: records with one of these FLAG bits are not counted (default 0x704)")
    ap.add_argument("--pileup", metavar="PREFIX", help="pile up base counts per position on the device; writes PREFIX.pileup.tsv (the variant sites) and PREFIX.consensus.fa")
    ap.add_argument("--pile-regions", metavar="BED", help="with --pileup: the regions (contig, 0-based start, end), sorted and disjoint; default: every contig whole")
    ap.add_argument("--pile-min-baseq", type=int, default=0, metavar="Q", help="with --pileup: bases with a lower quality are not counted")
    ap.add_argument("--pile-min-mapq", type=int, default=0, metavar="Q", help="with --pileup: records with a lower MAPQ are not counted")
    ap.add_argument("--pile-excl-flags", type=lambda x: int(x, 0), default=0x704, metavar="F", help="with --pileup: records with one of these FLAG bits are not counted (default 0x704)")
    ap.add_argument("--pile-min-depth", type=int, default=8, metavar="N", help="with --pileup: a site and a consensus base need this depth (default 8)")
    ap.add_argument("--pile-min-alt", type=int, default=2, metavar="N", help="with --pileup: a site's allele needs this count (default 2)")
    ap.add_argument("--pile-frac", default="1/5", metavar="NUM/DEN", help="with --pileup: and this fraction of the depth (default 1/5)")
    ap.add_argument("--stats", metavar="PREFIX", help="collect read and alignment statistics on the device; writes PREFIX.stats.tsv")
    ap.add_argument("--stats-cycles", type=int, default=512, metavar="N", help="with --stats: rows of the per-cycle tables; later cycles share the last row (default 512, at most 1024)")
    ap.add_argument("--stats-max-len", type=int, default=65536, metavar="N", help="with --stats: the last read-length bin (default 65536)")
    ap.add_argument("--stats-max-indel", type=int, default=64, metavar="N", help="with --stats: the last indel-length bin (default 64)")
    ap.add_argument("--stats-min-mapq", type=int, default=0, metavar="Q", help="with --stats: records with a lower MAPQ are no alignments")
    ap.add_argument("--stats-excl-flags", type=lambda x: int(x, 0), default=0x700, metavar="F", help="with --stats: records with one of these FLAG bits are left out (default 0x700)")
    ap.add_argument("-d", dest="dump", metavar="FILE", help="dump the index to FILE (.mmi, as the reference's -d) after the build; FILE can be given as ref later")
    ap.add_argument("--device-reader", action="store_true", help="parse and encode four-line FASTQ on the device (gdiet_hip_fastx_attach); the reader hands out resident batches")
    a = ap.parse_args()
    if a.eqx and a.preset != "sr":
        ap.error("--eqx is interpreted for --preset sr only (the LongReads variant does not interpret MM_F_EQX)")
    if a.sam_device and a.bam:
        ap.error("--sam-device formats SAM text: it does not go with --bam")
    if a.bam and not a.bgzf:
        a.bgzf = "device"
    if (a.sort and not a.bam) or (a.index and not a.sort):
        ap.error("--sort goes with --bam, --index with --sort")
    if a.markdup and not (a.bam and a.sort):
        ap.error("--markdup needs --bam --sort: duplicates are decided over the whole sorted file, which only the sorter holds")
    pkg = _load_pkg()
    ctx = pkg.Context(0)
    tag_bits = (0x1000000 if a.MD else 0) | (0x40 if a.cs else 0) | (0x800 if a.cs == "long" else 0)
    try:
        if a.ref.startswith("synth:"):  # "synth:3088": bench.py's synthetic reference of that many Mbp, made in-process (no 3 GB FASTA file to write and parse)
            import bench
            names, seqs = bench.synth_reference(float(a.ref.split(":")[1]), seed=2)
            t0 = time.perf_counter()
            m = pkg.Mapper(ctx, names, seqs, preset=a.preset, n_threads=pkg.effective_cpus())
        else:  # a FASTA / FASTQ file (plain, gzip, BGZF) or an .mmi, known by its magic: gdiet_hip_index_open
            t0 = time.perf_counter()
            m = pkg.Mapper.from_file(ctx, a.ref, preset=a.preset, n_threads=pkg.effective_cpus())
        if a.dump:
            m.dump_mmi(a.dump)
    except pkg.GdietError as e:
        print("map_file: %s: %s" % (a.ref, e), file=sys.stderr)
        ctx.close()
        sys.exit(1)
    m.opt.flag |= tag_bits  # read by the SAM formatter alone (gdiet_hip_sam_batch); the mapping path does not interpret them
    if a.eqx:
        m.opt.flag |= 0x4000000  # MM_F_EQX: read by the mapping path (the CIGARs are rewritten on the device)
    # -Y / -L / -y / -Q / --sam-hit-only: read by the SAM formatter alone, like the tag bits
    m.opt.flag |= (0x80000 if a.softclip else 0) | (0x10000 if a.long_cigar else 0) | (0x2000000 if a.copy_comment else 0) | (0x10 if a.no_qual else 0) | \
        (0x40000000 if a.sam_hit_only else 0)
    if a.rg is not None:
        try:
            m.set_read_group(a.rg)
        except pkg.GdietError as e:
            print("map_file: -R: %s" % (e,), file=sys.stderr)
            m.close()
            ctx.close()
            sys.exit(1)
    m.set_host_threads(pkg.effective_cpus())
    t_idx = time.perf_counter() - t0
    chunk = a.K or (39321600 if a.preset == "sr" else 80_000_000)
    sort_stats = None
    cov, cov_report = None, None
    pile, pile_report = None, None
    stats, stats_report = None, None
    try:
        bgzf_out = None
        if a.coverage:
            cov = pkg.Coverage(m, excl_flags=a.cov_excl_flags, min_mapq=a.cov_min_mapq, window=a.cov_window)
        if a.pileup:
            regions = None
            if a.pile_regions:
                with open(a.pile_regions) as f:
                    regions = [(m.names.index(x[0]), int(x[1]), int(x[2])) for x in (l.split() for l in f if l.strip() and not l.startswith(("#", "track", "browser")))]
            num, den = (int(x) for x in a.pile_frac.split("/"))
            pile = pkg.Pileup(m, regions=regions, excl_flags=a.pile_excl_flags, min_mapq=a.pile_min_mapq, min_baseq=a.pile_min_baseq)
        if a.stats:
            stats = pkg.Stats(m, excl_flags=a.stats_excl_flags, min_mapq=a.stats_min_mapq, cycles=a.stats_cycles, max_len=a.stats_max_len, max_indel=a.stats_max_indel)
        resident = a.bam and (a.sort or a.bgzf == "device")  # the records are resident in the sorter's or the writer's hands
        attach, attach_pile, attach_stats = cov is not None and resident, pile is not None and resident, stats is not None and resident
        if a.sort:
            sorter = pkg.BamSorter(a.out, m, bgzf=a.bgzf, level=a.bgzf_level, threads=a.bgzf_threads, run_bytes=a.sort_mem, tmp_dir=a.tmp_dir, index=a.index, version=VERSION, argv=sys.argv,
                                   markdup=a.markdup)
            if attach:
                sorter.set_coverage(cov)
            if attach_pile:
                sorter.set_pileup(pile)
            if attach_stats:
                sorter.set_stats(stats)
            try:
                n, dt = map_file(pkg, m, a.reads, None, chunk, a.inflight, a.reader_threads, with_qual=not a.no_qual, with_comment=a.copy_comment, device_reader=a.device_reader,
                                 bam=True, sorter=sorter, cov_add=None if attach else cov, pile_add=None if attach_pile else pile, stats_add=None if attach_stats else stats)
                t_close = time.perf_counter()
                sort_stats = dict(sorter.close(), route=a.bgzf)
                sort_stats["close_seconds"] = round(time.perf_counter() - t_close, 3)
                dt += sort_stats["close_seconds"]
            finally:
                if sort_stats is None:
                    try:
                        sorter.close()
                    except pkg.GdietError:
                        pass
        else:
            with (pkg.BgzfWriter(a.out, ctx=ctx if a.bgzf == "device" else None, level=a.bgzf_level, threads=a.bgzf_threads) if a.bgzf else open(a.out, "wb")) as out:
                bgzf_out = out if a.bgzf else None
                if attach:
                    out.set_coverage(cov)
                if attach_pile:
                    out.set_pileup(pile)
                if attach_stats:
                    out.set_stats(stats)
                if a.bam:
                    out.write(m.bam_header(VERSION, sys.argv))
                elif a.header:
                    out.write(m.sam_header(VERSION, sys.argv).encode())
                n, dt = map_file(pkg, m, a.reads, out, chunk, a.inflight, a.reader_threads, with_qual=not a.no_qual, with_comment=a.copy_comment,
                                 device_reader=a.device_reader, bam=a.bam, sam_device=a.sam_device, cov_add=None if attach else cov, pile_add=None if attach_pile else pile,
                                 stats_add=None if attach_stats else stats)
        if cov is not None:
            t_cov = time.perf_counter()
            _, summary = cov.finish()
            cov.write(a.coverage)
            cov_report = dict(summary, prefix=a.coverage, window=a.cov_window, attached=attach, finish_write_seconds=round(time.perf_counter() - t_cov, 3))
            cov.close()
        if pile is not None:
            t_pile = time.perf_counter()
            summary = pile.finish()
            pile.write(a.pileup, min_depth=a.pile_min_depth, min_alt=a.pile_min_alt, frac=(num, den))
            pile_report = dict(summary, prefix=a.pileup, regions=len(pile.regions), attached=attach_pile, finish_write_seconds=round(time.perf_counter() - t_pile, 3))
            pile.close()
        if stats is not None:
            t_stats = time.perf_counter()
            summary, _ = stats.finish()
            stats.write(a.stats)
            stats_report = dict(summary, prefix=a.stats, attached=attach_stats, finish_write_seconds=round(time.perf_counter() - t_stats, 3))
            stats.close()
    except Exception as e:  # noqa: BLE001  (every ticket has been waited for by now: the context can be closed)
        print("map_file failed: %r" % (e,), file=sys.stderr)
        if cov is not None:
            cov.close()
        if pile is not None:
            pile.close()
        if stats is not None:
            stats.close()
        m.close()
        ctx.close()
        sys.exit(1)
    print(json.dumps({"reads": n, "seconds": round(dt, 3), "reads_per_s": round(n / dt), "index_s": round(t_idx, 2), **({} if a.ref.startswith("synth:") else {"ref_open": m.open_stats()}), "mini_batch_bases": chunk,
                      "inflight": a.inflight, "reader_threads": a.reader_threads, "tags": "MD" if a.MD else ("cs=" + a.cs if a.cs else None), "eqx": a.eqx, "out": a.out, "caller_seconds": map_file.last_stage_seconds,
                      **({"reader_stats": map_file.last_reader_stats} if a.device_reader else {}), "bgzf_stats": map_file.last_bgzf_stats, "reads_format": map_file.last_format,
                      **({"bgzf_out": dict(bgzf_out.stats(), route=a.bgzf, device_seconds=[round(x, 4) for x in ctx.bgzf_deflate_seconds()])} if bgzf_out is not None else {}),
                      **({"bam_sort": sort_stats} if sort_stats is not None else {}),
                      **({"coverage": cov_report} if cov_report is not None else {}),
                      **({"pileup": pile_report} if pile_report is not None else {}),
                      **({"stats": stats_report} if stats_report is not None else {}),
                      **({"bam": True, "bam_device_seconds": [round(x, 4) for x in m.bam_device_seconds()]} if a.bam else {}),
                      **({"sam_device": True, "sam_device_seconds": [round(x, 4) for x in m.bam_device_seconds()]} if a.sam_device else {})}))
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
