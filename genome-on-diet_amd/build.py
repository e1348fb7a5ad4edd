"""Compile the HIP C-ABI library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libgdiet_hip.so")
SRC = os.path.join(HERE, "csrc", "gdiet_hip.hip")
RES = os.path.join(HERE, "build_resources.txt")  # the compiler's per-kernel resource remarks of the last build

# Register budgets the design depends on (checked against the compiler's own resource report after every build):
#   * the 64-lane DP kernel: 96 VGPRs = 5 wavefronts per SIMD, and nothing of its row loops in scratch memory -- the full-band rows, the
#     half-block rows of the 495-wide band and the quarter-block rows of the 239-wide band it tries before them are one kernel
#     (ksw_wave.hip.h, "NARROW BAND FIRST" / "THE QUARTER RUNG"), so one budget covers all three row loops;
#   * the kernels that must be able to start BESIDE a full house of those DP wavefronts (5 x 96 of a SIMD's 512 registers are taken):
#     at most 32 VGPRs (map_kernels.hip.h: map_post_wave_kernel; map_diffstr.hip.h: the cs / MD tag pass of batch i runs beside the DP of batch i+1).
BUDGET = {"_Z21ksw_extd2_wave_kernelILi64ELi0ELb1E": dict(vgprs=96, scratch=0),
          "_Z21ksw_extd2_pipe_kernelILb1E": dict(vgprs=128, scratch=320),  # four wavefronts per SIMD; the spills sit in the once-per-alignment staging code, none in the steps
          "_Z20map_post_wave_kernel": dict(vgprs=32, scratch=0),
          "_Z21map_pack_cigar_kernel": dict(vgprs=32, scratch=0),
          # the wave seed kernel on the tile sketch (map_tile_sketch.h): 64 registers = two of its wavefronts in the room one retiring DP
          # wavefront leaves (96 + the 32 a full house leaves free); not the 32 that would start beside a full house.  Its scratch is
          # mm_seed_select's heap on lane 0 (1 KB) and a few spills outside the tile loop.
          "_Z20map_seed_wave_kernel": dict(vgprs=64, scratch=1152),
          # the rest of a HiFi batch's tail: with two batches in flight every kernel between a batch's main DP launch and its results runs
          # beside the other batch's DP launch (profiles/r13_batch_tail.md)
          "_Z25ksw_backtrack_wave_kernel": dict(vgprs=32, scratch=0),
          "_Z22ksw_exact_match_kernel": dict(vgprs=32, scratch=0),
          "_Z18map_diffstr_kernel": dict(vgprs=32, scratch=0),  # every instance: count / write pass x MD / cs / cs=long (map_diffstr.hip.h)
          # the reader's device mode (fastx_dev.hip.h) parses block i + 1 and encodes batch i + 1 beside the DP of batch i
          "_Z18fastx_count_kernel": dict(vgprs=32, scratch=0),
          "_Z18fastx_write_kernel": dict(vgprs=32, scratch=0),
          "_Z19fastx_record_kernel": dict(vgprs=32, scratch=0),
          "_Z19fastx_encode_kernel": dict(vgprs=32, scratch=0),
          # BGZF members inflated beside the DP of the batches in flight (bgzf_inflate.hip.h): nothing of the symbol loop in scratch memory
          "_Z19bgzf_inflate_kernel": dict(vgprs=64, scratch=0),
          # BGZF members written on the device (bgzf_deflate.hip.h): its local memory bounds it to one wavefront per SIMD at most, so
          # registers up to 128 cost no occupancy; nothing in scratch memory
          "_Z19bgzf_deflate_kernel": dict(vgprs=128, scratch=0),
          # BAM records encoded on the device (bam_encode.hip.h): batch i is encoded beside the DP of batch i + 1, like the difference strings
          "_Z17bam_encode_kernel": dict(vgprs=32, scratch=0),
          # SAM lines formatted on the device (sam_encode.hip.h): the same place in the pipeline as the BAM encoder
          "_Z17sam_encode_kernel": dict(vgprs=32, scratch=0),
          # BAM input unpacked on the device (bam_in.hip.h): block i + 1 is unpacked beside the DP of batch i, like the FASTQ passes
          "_Z17bam_unpack_kernel": dict(vgprs=32, scratch=0),
          # BAM records put into coordinate order (bam_sort.hip.h): a run is sorted, and a chunk of the merge gathered, beside the DP of the batches in flight
          "_Z14bam_key_kernel": dict(vgprs=32, scratch=0),
          "_Z17bam_gather_kernel": dict(vgprs=32, scratch=0),
          # duplicates marked in the sorter's resident runs and chunks (bam_markdup.hip.h): beside the DP wavefronts, like the rest of the sort
          "_Z14dup_key_kernel": dict(vgprs=32, scratch=0),
          "_Z17dup_decide_kernel": dict(vgprs=32, scratch=0),
          "_Z16dup_apply_kernel": dict(vgprs=32, scratch=0),
          # coverage accumulated from the resident BAM records (cov.hip.h): batch i is scattered beside the DP of batch i + 1, like the encoders
          "_Z18cov_scatter_kernel": dict(vgprs=32, scratch=0),
          "_Z17cov_window_kernel": dict(vgprs=32, scratch=0),
          # base counts per position piled up from the resident BAM records, and the calls after finish (pile.hip.h)
          "_Z19pile_scatter_kernel": dict(vgprs=32, scratch=0),
          "_Z16pile_call_kernel": dict(vgprs=32, scratch=0),
          "_Z16pile_site_kernel": dict(vgprs=32, scratch=0),
          # read and alignment statistics from the resident BAM records (stats.hip.h): the compiler's own figure
          "_Z20stats_scatter_kernel": dict(vgprs=64, scratch=0)}


def _newest_source():
    m = 0.0
    for root in (os.path.join(HERE, "csrc"), os.path.join(os.path.dirname(HERE), "include")):
        for f in os.listdir(root):
            m = max(m, os.path.getmtime(os.path.join(root, f)))
    return m


def check_resources(text):
    """{kernel prefix: (VGPRs, scratch bytes per lane)} for the kernels in BUDGET; raises if one is over its budget"""
    found = {}
    blocks = re.split(r"remark: Function Name: ", text)
    for b in blocks[1:]:
        name = b.split()[0]
        for prefix, lim in BUDGET.items():
            if name.startswith(prefix):
                v = re.search(r"remark:\s+VGPRs: (\d+)", b)
                sc = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
                if v and sc:
                    found[prefix] = (int(v.group(1)), int(sc.group(1)))
                    if int(v.group(1)) > lim["vgprs"] or int(sc.group(1)) > lim["scratch"]:
                        raise RuntimeError("%s: %d VGPRs / %d B scratch per lane, budget %d / %d (genome-on-diet_amd/build.py)"
                                           % (name, int(v.group(1)), int(sc.group(1)), lim["vgprs"], lim["scratch"]))
    missing = [p for p in BUDGET if p not in found]
    if missing:
        raise RuntimeError("no resource report for %s" % missing)
    return found


def build_hip(force=False, verbose=False):
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= _newest_source():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # max-ilp scheduling: the DP row loop is one long block of dependent packed-16 operations; the default scheduler leaves 40 hazard
    # s_nop in it (a VALU instruction reading the result of the VOP3P instruction right before it), this one 8: -1 % kernel time
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-mllvm", "-amdgpu-sched-strategy=max-ilp",
           "-Rpass-analysis=kernel-resource-usage", "-o", LIB, SRC, "-lz"]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    remarks = "\n".join(l for l in r.stderr.split("\n") if "-Rpass-analysis=kernel-resource-usage" in l)
    other = "\n".join(l for l in r.stderr.split("\n") if "-Rpass-analysis=kernel-resource-usage" not in l)
    if r.returncode:
        raise RuntimeError("hipcc failed:\n" + other[-4000:])
    open(RES, "w").write(remarks)
    found = check_resources(remarks)
    if verbose:
        print("register budgets:", found)
    return LIB


if __name__ == "__main__":
    print(build_hip(force=True, verbose=True))
