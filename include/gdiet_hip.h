/*
 * gdiet_hip.h -- C ABI of the MI355X (gfx950) implementation of Genome-on-Diet's per-read mapping hot path.
 *
 * Plain C, plain pointers and sizes: this is what the reference's C host (map.c's worker loop) binds.
 * Every entry point names the reference interface it replaces (paths relative to the reference tree;
 * SR/ = GDiet-ShortReads/, LR/ = GDiet-LongReads/; the two trees share every file cited here unless noted).
 *
 * Conventions
 *   - all functions return 0 on success, a negative GDIET_E_* code on failure; gdiet_hip_strerror() explains it.
 *     There is NO CPU fallback inside the library: if no gfx950 device / code object is usable the call fails.
 *   - "host" entry points take host pointers and do H2D/D2H themselves; "_dev" entry points take device
 *     pointers (e.g. torch tensors' data_ptr()) plus a hipStream_t passed as void*, and never synchronise.
 *   - sequences are nt4-encoded bytes 0..4 (A,C,G,T,N) exactly as the reference feeds ksw2 (LR/map.c:1622-1643,
 *     SR/index.c:183-196 mm_idx_getseq2).
 */
#ifndef GDIET_HIP_H
#define GDIET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDIET_OK            0
#define GDIET_E_NODEVICE   (-1) /* no HIP device / not gfx950 */
#define GDIET_E_HIP        (-2) /* a HIP runtime call failed */
#define GDIET_E_PARAM      (-3) /* invalid or unsupported argument (see gdiet_hip_strerror) */
#define GDIET_E_NOMEM      (-4) /* device workspace too small for the batch */
#define GDIET_E_CIGAR_CAP  (-5) /* a CIGAR did not fit the caller's capacity (n_cigar[i] holds the needed size) */

#define GDIET_KSW_NEG_INF (-0x40000000) /* KSW_NEG_INF, SR/ksw2.h:7 */

/* flag bits understood by the DP entry points; numeric values of SR/ksw2.h:9-18 */
#define GDIET_EZ_APPROX_MAX 0x08 /* the only mode the live path uses: LR/map.c:1742, SR/map.c:867 */

typedef struct gdiet_ctx gdiet_ctx; /* one per (process, GPU); owns the stream(s) and the device workspace */

/* scoring of one DP batch: the scalar arguments of ksw_extd2_sse (SR/ksw2.h:68-69) with the 5x5 matrix reduced
 * to what the non-GENERIC_SC path reads (mat[0], mat[1], mat[24]; SR/ksw2_extd2_sse.c:85-87). */
typedef struct {
	int8_t match;      /* mat[0]   (> 0) */
	int8_t mismatch;   /* mat[1]   (< 0) */
	int8_t sc_ambi;    /* mat[24]  (0 on the live path => ambiguous bases score -e2) */
	int8_t q, e, q2, e2; /* gap open / extend of the two affine models, as passed by the caller (un-swapped) */
	int8_t reserved;
	int32_t flag;      /* GDIET_EZ_APPROX_MAX (global alignment with CIGAR, left-aligned gaps, no z-drop) */
} gdiet_ksw_score_t;

/* ---- life cycle --------------------------------------------------------------------------------------------- */
int gdiet_hip_init(gdiet_ctx **ctx, int device_ordinal);   /* replaces nothing: GPU context for one device */
void gdiet_hip_destroy(gdiet_ctx *ctx);
const char *gdiet_hip_strerror(const gdiet_ctx *ctx);       /* text of the last failure on this context */
/* (The difference-string pass -- gdiet_hip_diffstr_batch, and gdiet_hip_sam_batch[_into] / gdiet_hip_paf_batch_seqs under --cs / --MD -- may
 * refuse a record on a writer thread while map calls run on another: its text is kept apart, and gdiet_hip_strerror returns it to the thread
 * whose call failed, until that thread's next difference-string, upload or map call.) */
int gdiet_hip_device_name(const gdiet_ctx *ctx, char *buf, size_t len);
/* which kernel variants handled the last batch: bit0 = register-resident 64-lane wave kernel, bit1 = generic LDS kernel,
 * bit2 = register-resident short-alignment kernels (several alignments per wavefront), bit3 = two-blocks-per-lane kernel (wide bands),
 * bit4 = some of bit2's alignments (full matrices of one geometry: a short-read batch) ran as skewed pipelines (ksw_pipe.hip.h) */
int gdiet_hip_last_kernel_mask(const gdiet_ctx *ctx);

/* ---- B3: batched banded dual-affine global alignment -------------------------------------------------------
 * Replaces, for a whole batch, the per-candidate sequence of calls in mm_map_frag:
 *     [exact_match_sse]  ->  ksw_extd2_avx512 | ksw_extd2_sse  ->  ksw_backtrack        (LR/map.c:1748-1806,
 *     SR/map.c:873-929; kernels SR/ksw2_extd2_sse.c:34-401, SR/ksw2_extd2_avx.c:72-913, SR/ksw2.h:131-163,
 *     SR/exact_match_sse.c:23-91).
 *
 * For alignment i (0 <= i < n):
 *   query  = qseq[qoff[i] .. qoff[i+1])       target = tseq[toff[i] .. toff[i+1])
 *   w[i]   = band width argument of ksw_extd2 (w < 0: max(qlen,tlen) as in the reference)
 *   exact_score[i] (may be NULL): if non-NULL and exact_score[i] != GDIET_KSW_NEG_INF and qlen == tlen, the
 *            exact-match pre-filter runs first; on a match score[i] = exact_score[i] and the CIGAR is "<qlen>M"
 *            (the caller passes qlen_sum * a -- bug-compatibility item 5 of SURVEY 8; LR/map.c:1782).
 * Outputs
 *   score[i]   = ez.score (GDIET_KSW_NEG_INF if the band emptied or the corner was not reached)
 *   n_cigar[i] = ez.n_cigar; cigar ops (BAM encoding len<<4|op, op 0=M 1=I 2=D) at cigar[cigar_off[i] ..)
 *   the caller provides cigar_off[n+1]; capacity of alignment i is cigar_off[i+1]-cigar_off[i]
 *   (qlen+tlen always suffices).
 * How a result is obtained is the library's business, what it is is the reference's: short alignments (a target of at most 256 bases) whose
 * result can be proven without the DP -- an N-free pair of equal length with so few mismatches that no gapped path can reach the main
 * diagonal's score: m (a + b) <= a + 2 (q + e) -- are answered by the pre-filter kernel with exactly what ksw_extd2 + ksw_backtrack return
 * for them (tests/test_oracle_ksw2.py pins the property on the reference's own ksw_extd2_sse).  GDIET_DIAG_SHORTCUT=0 in
 * the environment sends every alignment through the DP kernels and the walk.
 */
int gdiet_hip_ksw_extd2_batch(gdiet_ctx *ctx, int n,
                              const uint8_t *qseq, const int64_t *qoff,
                              const uint8_t *tseq, const int64_t *toff,
                              const int32_t *w, const int32_t *exact_score,
                              const gdiet_ksw_score_t *sc,
                              int32_t *score, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off);

/* same, everything already resident in HBM (device pointers); asynchronous on `stream` (hipStream_t).
 * Workspace for the backtrace matrices comes from the context (gdiet_hip_reserve). */
int gdiet_hip_ksw_extd2_batch_dev(gdiet_ctx *ctx, int n,
                                  const uint8_t *d_qseq, const int64_t *d_qoff,
                                  const uint8_t *d_tseq, const int64_t *d_toff,
                                  const int32_t *d_w, const int32_t *d_exact_score,
                                  const gdiet_ksw_score_t *sc, /* host */
                                  int32_t *d_score, int32_t *d_n_cigar, uint32_t *d_cigar, const int64_t *d_cigar_off,
                                  const int64_t *h_qoff, const int64_t *h_toff, const int32_t *h_w, /* host copies for planning */
                                  void *stream);

/* ---- K3: batched banded SINGLE-affine global alignment -------------------------------------------------------------
 * Replaces ksw_extz2_sse + ksw_backtrack (SR/ksw2_extz2_sse.c:31-312, SR/ksw2.h:62; BASELINE config 2; not called by the live
 * mapping path).  Same batch layout and outputs as gdiet_hip_ksw_extd2_batch; sc->q / sc->e are the gap costs, sc->q2 / sc->e2
 * are ignored, sc->flag must be GDIET_EZ_APPROX_MAX (the only mode GDiet ever passes; the exact-maximum mode is
 * gdiet_hip_ksw_extz2_batch_ex below); sequence bytes must be 0..4 (the one
 * out-of-alphabet byte GDiet produces, 7 for a reverse-complemented N, only ever reaches ksw_extd2).  Implementation note: at the
 * scorings the register-resident kernels take (gd_wave_scoring_ok: a + 3(q+e) + max(b,|N|) <= 120 and q+e small enough for the
 * byte-wide S keys) ksw_extz2(q,e) and ksw_extd2(q,e,q,e) visit identical cells with identical values -- the unsigned bias of extz2
 * is then a re-labelling that never crosses 127, and a second gap model equal to the first never wins the priority chain -- so
 * those kernels run their single-affine form.  Elsewhere the identity does not hold (the biased bytes leave the signed range, e.g.
 * a + 2(q+e) >= 128 wraps, and smaller scorings such as (a,b,q,e) = (2,32,40,2) differ in CIGARs through the band-edge padding
 * cells), and the call runs ksw_extz2_sse's own recurrence (ksw_extz2_exact.hip.h, APPROX_MAX branch; last_kernel_mask 2).  Tests
 * pin both against ksw_extz2_sse's outputs (tests/golden/ksw2_extz2.npz, ksw2_scoring.npz). */
int gdiet_hip_ksw_extz2_batch(gdiet_ctx *ctx, int n,
                              const uint8_t *qseq, const int64_t *qoff,
                              const uint8_t *tseq, const int64_t *toff,
                              const int32_t *w, const gdiet_ksw_score_t *sc,
                              int32_t *score, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off);

/* K3, exact-maximum mode: ksw_extz2_sse called WITHOUT KSW_EZ_APPROX_MAX (SR/ksw2_extz2_sse.c:226-268: the per-cell H array, the
 * row maximum with z-drop, SR/ksw2.h:172-188), the second mode SURVEY 8d names for BASELINE config 2.  sc->flag = 0 or
 * GDIET_EZ_EXTZ_ONLY (SR/ksw2.h:15); zdrop / end_bonus as the reference's arguments (zdrop < 0: no z-drop).  ez[i] receives every
 * scalar of ksw_extz_t (SR/ksw2.h:31-40); the CIGAR is the walk from the last cell, from (mqe_t, qlen-1) when EXTZ_ONLY reaches
 * the query end, or from (max_t, max_q) after a z-drop, exactly as :296-305.  One wavefront per alignment, state in LDS. */
#define GDIET_EZ_EXTZ_ONLY 0x40
typedef struct {
	int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end;
} gdiet_ksw_extz_t;
int gdiet_hip_ksw_extz2_batch_ex(gdiet_ctx *ctx, int n,
                                 const uint8_t *qseq, const int64_t *qoff,
                                 const uint8_t *tseq, const int64_t *toff,
                                 const int32_t *w, const gdiet_ksw_score_t *sc, int32_t zdrop, int32_t end_bonus,
                                 gdiet_ksw_extz_t *ez, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off);

/* ---- SURVEY 8f rank 4 (kernel half): batched splice-aware extension alignment -------------------------------------------
 * Replaces ksw_exts2_sse + ksw_backtrack (SR/ksw2_exts2_sse.c:34-416, SR/ksw2.h:71-72,131-163).  GDiet keeps this kernel of
 * minimap2 in its tree (SR/align.c:363 is its only call site, under MM_F_SPLICE) but no GDiet preset reaches it; it is provided
 * for a minimap2-compatible splice mode.  Arguments as the reference's: mat = the 5 x 5 matrix (m = 5), q / e the short gap,
 * q2 the long-gap (intron) open cost (must exceed q + e), noncan the penalty of a non-canonical splice site, junc = one
 * annotation byte per target base laid out like tseq (NULL: none) with junc_bonus, flag = any of KSW_EZ_SCORE_ONLY 0x01,
 * RIGHT 0x02, GENERIC_SC 0x04, APPROX_MAX 0x08, APPROX_DROP 0x10, EXTZ_ONLY 0x40, REV_CIGAR 0x80, SPLICE_FOR 0x100,
 * SPLICE_REV 0x200, SPLICE_FLANK 0x400 (SR/ksw2.h:9-18).  No band (the reference has none).  ez[i]: every scalar of ksw_extz_t;
 * CIGAR in BAM ops incl. N (3) for long gaps of at least long_thres bases.  One wavefront per alignment, state in LDS:
 * min(qlen, tlen) is limited to ~8000. */
int gdiet_hip_ksw_exts2_batch(gdiet_ctx *ctx, int n,
                              const uint8_t *qseq, const int64_t *qoff,
                              const uint8_t *tseq, const int64_t *toff, const uint8_t *junc,
                              const int8_t *mat, int8_t q, int8_t e, int8_t q2, int8_t noncan, int32_t zdrop, int8_t junc_bonus, int32_t flag,
                              gdiet_ksw_extz_t *ez, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off);

/* ---- SURVEY 8f rank 4 (chaining half): batched anchor chaining ------------------------------------------------------------
 * Replaces mg_lchain_dp (SR/lchain.c:124-190, SR/mmpriv.h:102-104) for a batch of reads; like ksw_exts2 it is code of minimap2
 * that GDiet keeps and never calls (GDiet votes instead of chaining), provided for a minimap2-compatible mode.  a = the
 * anchors of all reads as (x, y) pairs of uint64 (x: rev<<63 | tid<<32 | tpos -- minimap2's layout, SR/hit.c:26; any layout whose
 * upper 32 bits name the target + strand and whose lower 32 bits are the position chains alike --, y: flags<<40 | q_span<<32 | q_pos; per read
 * sorted by x as minimap2 sorts them), read i = pairs aoff[i] .. aoff[i+1]; the scalar parameters are the reference's.
 * Outputs, per read at the read's own offset (a chain set never has more chains or anchors than the read has anchors):
 * n_u[i] chains, u[aoff[i] + k] = score<<32 | n_anchors of chain k, a_out (pairs, at 2 * aoff[i]) = the chains' anchors, n_v[i]
 * of them -- the very arrays mg_lchain_dp returns (same chain order, same anchor order).  The reference frees its input; here
 * `a` stays untouched.  The O(n * max_iter) fill runs on the GPU, one wavefront per read; the chains are cut on host threads. */
int gdiet_hip_lchain_dp_batch(gdiet_ctx *ctx, int n_reads, const uint64_t *a, const int64_t *aoff,
                              int32_t max_dist_x, int32_t max_dist_y, int32_t bw, int32_t max_skip, int32_t max_iter, int32_t min_cnt, int32_t min_sc,
                              float chn_pen_gap, float chn_pen_skip, int32_t is_cdna, int32_t n_seg,
                              int32_t *n_u, int64_t *n_v, uint64_t *u, uint64_t *a_out);

/* make sure the context owns at least `bytes` of device workspace (backtrace arena); returns GDIET_E_NOMEM
 * if the device cannot provide it.  gdiet_hip_ksw_extd2_batch() grows the arena by itself. */
int gdiet_hip_reserve(gdiet_ctx *ctx, size_t bytes);
/* bytes of backtrace arena the batch (host-side lengths) needs */
size_t gdiet_hip_ksw_workspace_bytes(int n, const int64_t *qoff, const int64_t *toff, const int32_t *w);
/* restrict dispatch: 0 = automatic (default), 1 = force the generic LDS kernel, 2 = wave kernel only (fails
 * with GDIET_E_PARAM for alignments it cannot take).  For tests and A/B measurements. */
int gdiet_hip_set_kernel_mode(gdiet_ctx *ctx, int mode);
/* Wavefronts per SIMD the 64-lane DP kernel (long reads) is launched for: 5 (default: 96 VGPRs, the best throughput of a full pipeline)
 * or 4 (a fifth of every SIMD's registers stays free, so the seeding / voting kernels of the NEXT batch run beside the
 * DP kernel instead of trickling through as its wavefronts retire -- two batches in flight then keep the DP kernels back to back, at
 * two instead of three step times of latency; bench.py latency_mode).  Same arithmetic, same results. */
int gdiet_hip_set_dp_waves(gdiet_ctx *ctx, int waves_per_simd);
/* average device time (ms, HIP events on the launch stream) of the DP kernel(s) and of the backtrack kernel of the
 * most recent *_dev / host batch; only valid after the stream has been synchronised. */
int gdiet_hip_last_kernel_ms(gdiet_ctx *ctx, float *dp_ms, float *backtrack_ms);
/* The shader clock the 64-lane DP kernel sustained, from its own wavefronts: each stamps s_memtime (shader clock) and s_memrealtime
 * (constant 100 MHz) around its DP rows.  Median and minimum over the wavefronts of the most recent launches of the process, and the
 * median duration of one wavefront's rows.  (Says whether the kernel ran throttled: profiles/r03_clock.md.) */
int gdiet_hip_last_dp_clock(gdiet_ctx *ctx, double *sclk_mhz_median, double *sclk_mhz_min, double *wavefront_ms_median);
/* work of the most recent DP launch: DP cells = sum (qlen+tlen-1)*min(w+1,qlen,tlen), and the algorithmic bytes of
 * SURVEY.md 8d = cells + (qlen+tlen) + qlen + ceil(tlen/2) per alignment (what bench.py's roofline divides by the kernel time) */
int gdiet_hip_last_dp_work(const gdiet_ctx *ctx, uint64_t *cells, uint64_t *alg_bytes);
/* The 64-lane DP kernel aligns a box whose band is wider than 495 in a band of 495 first (half the arithmetic per row) and keeps the
 * result when a bound on every path outside that band proves it to be the full band's; otherwise the same wavefront runs the full
 * band.  Counters of the most recent DP launch: boxes that tried the narrow band, boxes whose certificate held.  Call after the
 * batch has completed.  GDIET_NARROW_BAND=0 (read at gdiet_hip_init) switches the narrow band off. */
int gdiet_hip_last_narrow_band(gdiet_ctx *ctx, uint64_t *tried, uint64_t *certified);
/* The same per rung of the ladder the kernel climbs: before the 495-wide band a box tries the quarter-block rows in a 239-wide band with the
 * same certificate (D = 239).  out[0] / out[1]: boxes that evaluated the certificate at 239 / for which it held; out[2] / out[3]: the
 * same at 495.  GDIET_NARROW_QUARTER (read at gdiet_hip_init): 0 never offers the 239 rung, 1 always does; unset, a context stops
 * offering it for 15 launches after one in which fewer than four fifths of at least 64 boxes certified there.  Results never depend on it. */
int gdiet_hip_last_narrow_rungs(gdiet_ctx *ctx, uint64_t out[4]);
/* The backtrace arena of the most recent DP launch.  Where the narrow band is offered, the slot of a box that tries it holds the 512-byte
 * rows only; a box whose certificate fails at both rungs claims its full-band rows from an overflow pool behind the slots (default: a
 * sixteenth of them, at least 64 MiB; GDIET_BT_OVERFLOW_MB), and one that finds the pool used up is served by a drain launch of the same kernel behind
 * the main one, from the start of the arena.  out[0]: boxes that claimed from the pool; out[1]: boxes served by a drain launch; out[2]:
 * bytes of arena the batch was planned with.  GDIET_BT_COMPACT=0 (read when the library is loaded): every slot is sized for the full-band
 * rows.  Results never depend on either.  GDIET_E_HIP if a box was left without rows (a planner bug, never a wrong alignment). */
int gdiet_hip_last_arena(gdiet_ctx *ctx, uint64_t out[3]);
/* Drain launches the most recent DP launch enqueued.  A box that finds the pool used up appends its id to a pending list on the device.
 * Where the call waits for its stream anyway (gdiet_hip_ksw_extd2_batch, the mapping path in an arena of its own) the host reads the
 * list's length when the main launch has ended: 0 launches for an empty list, else as many as the pending boxes need, one wavefront per
 * box.  gdiet_hip_ksw_extd2_batch_dev never waits, and lanes that take turns in a shared arena must not: there the planner's worst case
 * for the whole batch is enqueued up front, and the wavefronts past the list's end return at once. */
int gdiet_hip_last_drain_launches(gdiet_ctx *ctx, int *enqueued);

/* ---- B1: the per-read mapping path for a whole batch of reads (LongReads variant; ShortReads variant with MM_F_SR) ----
 * Replaces step 1 of worker_pipeline -- kt_for(n_threads, worker_for, ...) -> mm_map_frag() per read
 * (LR/map.c:2132-2137 -> :1975-2022 -> :1273-1940): sketch2/get_shift/sketch3, seed filter + collect, hit sort,
 * vote/vote_2, candidate geometry, exact-match / ksw_extd2 / backtrack, mm_update_extra, concatenate_cigars,
 * mm_set_sam_params.  The seeding/voting stages and the DP run on the GPU; geometry and CIGAR post-processing
 * run on host threads inside this library (they need the float/double comparisons and the bug-compatible
 * control flow of the reference).
 */

/* device-resident index: the flat mirror of mm_idx_t (LR/minimap.h:79-96, LR/index.c:29-34,84-100) */
typedef struct gdiet_index gdiet_index;

/* Build the index from nt ASCII sequences with this library's own builder (same minimizers, same position order
 * as mm_idx_gen of GDiet_avx: LR/index.c:306-412, LR/sketch.c:156/1577) and upload it.  pattern/pattern_len = -Z/-W.
 * Limits, refused with GDIET_E_PARAM: 1 <= k <= 28 as in the reference (LR/main.c), and 1 <= w <= 64 -- the reference accepts
 * w < 256; the winnowing windows of the sketch kernels live in registers / LDS sized for 64 (every preset uses w <= 19).  For
 * every w from 2 to 7 the reference's own scalar (GDiet) and AVX-512 (GDiet_avx) sketches disagree; at w = 1 and w >= 8 they agree.
 * This library follows the scalar one: its pattern phases and seed hits equal GDiet's at w = 1 .. 12 on the reads DESIGN.md names
 * ("Known divergence"), and two rows of tests/golden/opts/grid.json written by scalar GDiet at w = 4 pin that
 * (tests/test_map_host.py on the CPU, tests/test_option_grid_gpu.py on the GPU). */
int gdiet_hip_index_build(gdiet_ctx *ctx, gdiet_index **idx, int n_seq, const char *const *names,
                          const char *const *seqs, const uint32_t *lens, int k, int w, const char *pattern,
                          int pattern_len, int n_threads);
/* Upload an index that the caller already holds in flat form -- what a reference-side stub produces by walking
 * mm_idx_t::B[]: keys[i] = minimizer hash (x>>8), cnt[i] its number of occurrences, pos = the
 * occurrence lists (y values, each list sorted ascending) concatenated in key order; S = mm_idx_t::S. */
int gdiet_hip_index_import(gdiet_ctx *ctx, gdiet_index **idx, int k, int w, const char *pattern, int pattern_len,
                           int n_seq, const char *const *names, const uint32_t *lens, const uint64_t *offsets,
                           const uint32_t *S, uint64_t n_keys, const uint64_t *keys, const uint32_t *cnt,
                           const uint64_t *pos);
/* the inverse of gdiet_hip_index_import: sizes first (array arguments NULL), then the arrays (caller-allocated: n_keys keys and
 * counts, n_pos positions, n_S_words words of S, n_seq offsets).  What a maintainer needs to write the index back into an
 * mm_idx_t / .mmi (LR/index.c:428-470 mm_idx_dump) or to check it against mm_idx_get. */
int gdiet_hip_index_export(const gdiet_index *idx, uint64_t *n_keys, uint64_t *n_pos, uint64_t *n_S_words, uint64_t *keys,
                           uint32_t *cnt, uint64_t *pos, uint32_t *S, uint64_t *offsets);
/* Read an .mmi file written by the reference (mm_idx_dump, LR/index.c:480-517; `GDiet -d`) and upload it.  The file does not store
 * the pattern, so -Z / -W are given again, exactly as on the reference's command line. */
int gdiet_hip_index_load_mmi(gdiet_ctx *ctx, gdiet_index **idx, const char *path, const char *pattern, int pattern_len);
/* Write the .mmi file mm_idx_dump (LR/index.c:480-517) writes for this index, byte for byte: the position arrays in the order
 * worker_post fills them and every bucket's entries in the slot order of the reference's khash table (its resize / put sequence is
 * emulated: LR/index.c:216-264, LR/khash.h:199-330).  bucket_bits = mm_idxopt_t::bucket_bits (14 by default). */
int gdiet_hip_index_dump_mmi(gdiet_ctx *ctx, const gdiet_index *idx, const char *path, int bucket_bits);
void gdiet_hip_index_destroy(gdiet_ctx *ctx, gdiet_index *idx);
/* mm_idx_cal_max_occ (LR/index.c:190-210) */
int32_t gdiet_hip_index_cal_max_occ(const gdiet_index *idx, float frac);
uint64_t gdiet_hip_index_n_keys(const gdiet_index *idx);

/* ---- Reference input: an index from a file -----------------------------------------------------------------------------------------
 * gdiet_hip_index_open takes the reference as the reference's command line does (mm_idx_reader_open, LR/index.c:595-613): a FASTA or
 * FASTQ file -- plain, gzip, BGZF, or "-" for stdin -- or an .mmi index file.
 *   WHAT IT RETURNS.  For a sequence file: the index gdiet_hip_index_build makes of the names and sequences that this library's sequential
 *     reader grammar (kseq_read, LR/kseq.h:191-232, without qualities) returns for the file, in file order.  Nothing else defines it:
 *     neither the route (device or host), nor the block size, nor the compression of the input changes a byte of it.
 *   .mmi.  An index file is known by its magic alone, as mm_idx_is_idx knows it (LR/index.c:573-593: a regular file of four bytes or
 *     more that starts with "MMI\2"); the file name is not looked at.  k and w are then the file's: other values in the arguments are
 *     not an error (the reference overrides them with a warning); gdiet_hip_index_info reports the values in use.  pattern / pattern_len
 *     are always the arguments' (the file does not store them, see gdiet_hip_index_load_mmi).
 *   LIMITS.  Those of gdiet_hip_index_build, refused with the same texts.  One part only: the file is never split as -I splits it.  A
 *     file without any sequence is GDIET_E_PARAM, as n_seq = 0 is there.
 *   ERRORS.  A file that cannot be opened or read: GDIET_E_PARAM, and gdiet_hip_strerror names the file.
 *   ROUTES.  By default the blocks of the file go to the device as the reader reads them (inflated, where compressed, on n_threads host
 *     threads): three passes per block place the nt4 code of every base and find the header lines (csrc/ref_fasta.h says which blocks
 *     the device claims, and why its result is kseq_read's there; every other block goes through that grammar on the host), a last pass
 *     packs S, and sketch, sorts and table are gdiet_hip_index_build's.  GDIET_INDEX_BUILD=host keeps everything on the host: the reader
 *     collects the records and the host builder runs.  GDIET_FASTX_BLOCK sizes the blocks, as for reads.
 *   n_threads <= 0: the CPUs the process may use. */
int gdiet_hip_index_open(gdiet_ctx *ctx, gdiet_index **idx, const char *path, int k, int w, const char *pattern, int pattern_len,
                         int n_threads);
/* The sequence table of any index, however it was made; every pointer may be NULL.  *names and *lens point at n_seq entries that stay
 * valid while the index lives. */
int gdiet_hip_index_info(const gdiet_index *idx, int *k, int *w, int *n_seq, const char *const **names, const uint32_t **lens);
/* The counters of the gdiet_hip_index_open that made this index (all zero for an index made otherwise).
 *   counts6:  file bytes | decompressed bytes | blocks | blocks handed to the host grammar | bases placed by the device | bases placed
 *             by the host
 *   seconds5: read | inflate (both on the reading thread, beside the passes; a gzip stream inflates inside its reads and reports them
 *             here) | device passes (copy up, kernels, tables down) | host grammar | the rest of the build (pack, sketch, sorts, table)
 *   device_peak_bytes: the most device memory the block passes, the bases and S held at one time (0 on the host route). */
int gdiet_hip_index_open_stats(const gdiet_index *idx, int64_t *counts6, double *seconds5, uint64_t *device_peak_bytes);
/* The kernel-level boundary, for tests: the three block passes on text[0, n) with the parser in state_in at byte 0 -- 0: at the start
 * of a line, 1: inside a header line, 2: inside a sequence line.  *claimed is n where the device claims the block and 0 where it does
 * not (then nothing else is returned and *state_out is -1).  For a claimed block: nt4[0, *n_bases) are the codes of its bases;
 * rows[3 r ..] = {offset of the '>', offset of its '\n' or 0xffffffff where the header line does not end in the block, bases in front
 * of it} for every header line that starts in the block (*n_rows of them); *run_nl is the offset of the '\n' that ends the header line
 * running into the block (state_in == 1), or 0xffffffff; *state_out is the state behind the last byte.  nt4 / rows may be NULL to ask
 * for the sizes only; too little room is GDIET_E_PARAM. */
int gdiet_hip_ref_block(gdiet_ctx *ctx, const char *text, size_t n, int state_in, uint8_t *nt4, size_t nt4_cap, size_t *n_bases,
                        uint32_t *rows, size_t row_cap, size_t *n_rows, size_t *claimed, int *state_out, uint32_t *run_nl);

/* The kernel-level boundary of P1 (mm_fix_cigar + mm_update_extra, LR/align.c:93-172,259-318), for tests: the kernels the mapping path
 * launches behind its backtrack, on n alignments given as raw arrays.
 *   qseq / tseq   nt4 codes of all query / target windows; alignment b's begin at qoff[b] / toff[b] (n + 1 offsets each)
 *   cigar         in/out: the CIGAR pool of coff[n] words; alignment b owns the slot [coff[b], coff[b + 1]) and its raw CIGAR starts the slot
 *   n_cigar       in/out: operations per alignment
 *   score         a slot whose score is -0x40000000, whose n_cigar is <= 0 or larger than its slot is dead: its GdPostOut is all zero
 *                 and its slot and n_cigar are left alone
 *   mat           the 5 x 5 scoring matrix mat[target * 5 + query]; q, e, log_gap as in mm_update_extra
 *   form          0: one alignment per thread (map_post_kernel)   1: one alignment per wavefront (map_post_wave_kernel)
 *   exported      1: the kernel itself stores score, n_cigar and the results to page-locked host memory (what the mapping path does when
 *                 the results must not wait for a copy); the returned n_cigar and post are then those stores, and the score stored
 *                 must equal the one given (GDIET_E_HIP otherwise)
 *   post          n records of six int32: qshift, tshift, mlen, blen, dp_max, n_ambi
 * The --eqx rewrite is not reachable from here. */
int gdiet_hip_post_batch(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff, const uint8_t *tseq, const int64_t *toff,
                         uint32_t *cigar, const int64_t *coff, int32_t *n_cigar, const int32_t *score, const int8_t *mat, int8_t q, int8_t e,
                         int log_gap, int form, int exported, int32_t *post);

/* the fields of mm_mapopt_t (LR/minimap.h:145-214) this path reads; fill them from the reference's struct */
typedef struct {
	int64_t flag;                 /* MM_F_* bits; only NO_PRINT_2ND, SR (selects the variant), FRAG_MODE, FOR_ONLY, REV_ONLY and, with SR, EQX are
	                               * interpreted.  MM_F_EQX (0x4000000, --eqx) with MM_F_SR: every entry point that maps (gdiet_hip_map_batch, _map_uploaded,
	                               * _map_submit / _map_wait, _map_batch_multi, _map_frag) returns CIGARs with = (7) and X (8) in place of M, as
	                               * mm_update_cigar_eqx writes them (SR/align.c:174-257, its count-based shortcut included); n_cigar is the rewritten length,
	                               * no other field of a record changes.  Without MM_F_SR the bit is NOT interpreted: the LongReads tree rewrites before
	                               * concatenate_cigars, which knows no = / X, and aborts under --eqx --MD. */
	int32_t a, b, q, e, q2, e2;
	uint32_t bw;
	int32_t min_dp_max, best_n;
	float q_occ_frac;
	int32_t mid_occ, max_max_occ, occ_dist, max_frag_len;
	uint32_t vt_dis, vt_nb_loc;
	float vt_cov, vt_f, vt_df1, vt_df2;
	uint32_t max_max_gap, max_min_gap;
	float max_seeds;
	/* read only when flag has MM_F_SR: the ShortReads variant of mm_map_frag (SR/map.c:586-984; SR/minimap.h:149-150,196-197) */
	float min_cnt, rec_threshold_frac;  /* -n FLOAT1,FLOAT2 */
	float bw_frac;                      /* -r FLOAT,INT,INT: band = vote distance = clamp(qlen*bw_frac, bw_min, bw_max) */
	int32_t bw_min, bw_max;
	int32_t AF_max_loc;                 /* --AF_max_loc */
} gdiet_mapopt_t;

/* one alignment record: mm_reg1_t + mm_extra_t (LR/minimap.h:105-131) flattened */
typedef struct {
	int32_t id, cnt, rid, score, qs, qe, rs, re, parent, subsc, mlen, blen;
	uint32_t mapq, rev, sam_pri;
	int32_t dp_score, dp_max;
	uint32_t n_ambi, n_cigar;
	uint32_t *cigar;              /* points into the allocation the record belongs to */
} gdiet_reg_t;

/* Map n_reads single-segment reads (ASCII sequences).  On return regs[i] is a malloc'd array of n_regs[i] records
 * (NULL when n_regs[i] == 0, as LR/map.c:1915), in the order mm_map_frag leaves them.  The records and CIGARs of a batch share
 * a few large allocations: release them with ONE gdiet_hip_free_regs call on the same n_reads / n_regs / regs arrays, never with
 * free() on a single regs[i]. */
int gdiet_hip_map_batch(gdiet_ctx *ctx, const gdiet_index *idx, const gdiet_mapopt_t *opt, int n_reads,
                        const char *const *seqs, const int32_t *lens, int32_t *n_regs, gdiet_reg_t **regs);
void gdiet_hip_free_regs(int n_reads, int32_t *n_regs, gdiet_reg_t **regs);

/* B2, the per-read level of the boundary: mm_map_frag's call shape (LR/minimap.h:390, LR/map.c:1273-1940) for ONE fragment of n_segs
 * segments.  As in the reference only segment 0 is sketched and aligned (qlen_sum aside: paired-end input is effectively unsupported
 * there, SURVEY bug-compatibility item 7): n_regs[0] / regs[0] receive its records, the other segments none.  Release with
 * gdiet_hip_free_regs(n_segs, n_regs, regs).  A wavefront-per-alignment device path gains nothing from one read at a time: this entry
 * exists for callers that are written against mm_map_frag; throughput lives in gdiet_hip_map_batch / _submit. */
int gdiet_hip_map_frag(gdiet_ctx *ctx, const gdiet_index *idx, const gdiet_mapopt_t *opt, int n_segs, const int32_t *qlens,
                       const char *const *seqs, int32_t *n_regs, gdiet_reg_t **regs);

/* B4, the sketch / seed level of the boundary (LR/mmpriv.h:65-76), for a batch of reads: what mm_sketch2 + mm_get_shift (the pattern phase
 * shift[i]), mm_sketch3 (tmp_extracted_len[i]), mm_seed_mz_flt (n_mv[i]: minimizers left after the query-side filter) and
 * mm_collect_matches2 (the kept seeds: mm_seed_t reduced to n = occurrences in the index and q_pos = lastPos<<1 | strand, in sketch
 * order; their occurrence lists = the y values mm_idx_get returns, rid<<32 | lastPos<<1 | strand) produce for every read -- the output of
 * the seeding kernel (LR/map.c:1296-1325).  Read i owns seeds[seed_off[i] .. seed_off[i+1]) and occ[occ_off[i] .. occ_off[i+1]) (the
 * lists of its seeds back to back).  *seeds and *occ are malloc'd: free() them. */
typedef struct { uint32_t n, q_pos; } gdiet_seed_t;
int gdiet_hip_seed_batch(gdiet_ctx *ctx, const gdiet_index *idx, const gdiet_mapopt_t *opt, int n_reads, const char *const *seqs,
                         const int32_t *lens, int32_t *shift, uint32_t *tmp_extracted_len, uint32_t *n_mv, int64_t *seed_off,
                         int64_t *occ_off, gdiet_seed_t **seeds, uint64_t **occ);

/* Reads of the most recent map call on this context that were given up on and came back unmapped (n_regs = 0) while the rest of their
 * batch was mapped: a candidate's DP box lay outside its read / contig or had wrapped to an absurd size -- input on which the
 * reference reads stale heap memory (LR/map.c:1654-1806 with mm_idx_getseq2 returning short / -1), i.e. has no defined result.
 * last_call / total (since gdiet_hip_init) / what (a one-line description of the last one; valid until the next map call) may be NULL. */
int gdiet_hip_map_failed_reads(const gdiet_ctx *ctx, int64_t *last_call, int64_t *total, const char **what);

/* ---- single-process multi-GPU fan-out of one mini-batch -----------------------------------------------------------
 * What step 1 of worker_pipeline calls when the process owns several GPUs (LR/map.c:2132-2137: kt_for over the fragments of the
 * mini-batch; step 2 prints in input order, LR/kthread.c:97-121): the mini-batch is cut into n_ctx CONTIGUOUS read ranges of equal DP
 * cost (gdiet_hip_read_ranges_by_cost), range k is mapped by ctxs[k] against idxs[k] (the index replicated per device: build / import
 * / load it once per context) on a caller thread of its own, and every range writes its records straight into n_regs / regs at its
 * offset -- the arrays come back exactly as gdiet_hip_map_batch on one context would fill them (same records, same order; release
 * them with ONE gdiet_hip_free_regs call).  No collective: reads are independent.  Give every context its share of the host's CPUs
 * first (gdiet_hip_set_host_threads(ctx, gdiet_hip_effective_cpus() / n_ctx)).  Errors are joined: the code of the first failing
 * range is returned, its text (with device and read range) is gdiet_hip_strerror(ctxs[0]), and no records are handed back. */
int gdiet_hip_map_batch_multi(int n_ctx, gdiet_ctx *const *ctxs, const gdiet_index *const *idxs, const gdiet_mapopt_t *opt,
                              int n_reads, const char *const *seqs, const int32_t *lens, int32_t *n_regs, gdiet_reg_t **regs);
/* bounds[0..n_parts]: contiguous ranges of equal DP cost, a read costing (2 len - 1) * min(band + 1, len) cells (balance by
 * "sum l_seq^2-ish DP cost, not read count").  Host arithmetic only. */
int gdiet_hip_read_ranges_by_cost(int n_reads, const int32_t *lens, int n_parts, int32_t band, int32_t *bounds);

/* Two-step form for measurements: stage a batch in HBM once, then map it (repeatedly).  Only the second call belongs
 * to a timed region whose inputs are "already resident in HBM". */
typedef struct gdiet_read_batch gdiet_read_batch;
int gdiet_hip_batch_upload(gdiet_ctx *ctx, gdiet_read_batch **batch, int n_reads, const char *const *seqs, const int32_t *lens);
int gdiet_hip_map_uploaded(gdiet_ctx *ctx, const gdiet_index *idx, const gdiet_mapopt_t *opt, gdiet_read_batch *batch,
                           int32_t *n_regs, gdiet_reg_t **regs);
void gdiet_hip_batch_destroy(gdiet_ctx *ctx, gdiet_read_batch *batch);
/* Several batches in flight: _submit starts the whole path for a resident batch on a lane of its own (stream, scratch) and
 * returns a ticket, _wait joins it (results in the n_regs / regs arrays given to _submit).  Up to
 * gdiet_hip_set_inflight() tickets (default 2, at most 8) may be open; wait for them in submission order.  The latency-bound
 * stages of one batch overlap the DP kernel of another, exactly as the reference's kt_pipeline overlaps the steps of consecutive
 * mini-batches (LR/map.c:2094-2170); results are those of gdiet_hip_map_uploaded.  The lanes share one backtrace arena (~34 MB
 * per 15 kbp alignment: two whole-batch arenas would not fit in HBM), so their DP stages take turns -- unless a batch's backtrace
 * is small enough for every lane to hold one of its own (gdiet_hip_set_inflight sets the limit: 70 % of HBM / n, or
 * GDIET_LANE_ARENA_GB), in which case the DP kernels of the batches in flight overlap as well. */
typedef struct gdiet_map_ticket gdiet_map_ticket;
int gdiet_hip_set_inflight(gdiet_ctx *ctx, int n);
int gdiet_hip_map_submit(gdiet_ctx *ctx, const gdiet_index *idx, const gdiet_mapopt_t *opt, gdiet_read_batch *batch,
                         int32_t *n_regs, gdiet_reg_t **regs, gdiet_map_ticket **ticket);
int gdiet_hip_map_wait(gdiet_ctx *ctx, gdiet_map_ticket *ticket);
/* seconds spent in the stages of the most recent map call: [0] seed kernel, [1] vote kernel, [2] host geometry,
 * [3] gather + DP + backtrack kernels, [4] host post-processing, [5] transfers/other */
int gdiet_hip_map_stage_seconds(const gdiet_ctx *ctx, double out[6]);
/* How many batches of this process had to run their seeding stage a second time because a read produced more minimizers than the first
 * per-read scratch estimate holds (tiny windows, dense or long patterns).  The retry is exact; the count is for tests and tuning. */
int64_t gdiet_hip_map_scratch_retries(void);
/* software-pipeline depth of gdiet_hip_map_uploaded / gdiet_hip_map_batch: the batch is cut into slices that run the whole
 * chain on `n` independent lanes (stream + workspace + host threads each), overlapping the latency-bound stages of one slice
 * with the DP kernel of the others.  1 (default) = no pipelining.  Results do not depend on it. */
int gdiet_hip_set_map_lanes(gdiet_ctx *ctx, int n);
/* number of host threads used for geometry / CIGAR post-processing (default: gdiet_hip_effective_cpus(), at most 64) */
int gdiet_hip_set_host_threads(gdiet_ctx *ctx, int n);
/* CPUs the process may really use: min(hardware threads, affinity mask, cgroup CPU quota).  The reference sizes its worker pool
 * with -t (LR/main.c:85 n_threads); a caller that derives -t from the machine should use this figure. */
int gdiet_hip_effective_cpus(void);

/* ---- the per-base difference strings of --cs[=short|long] and --MD -------------------------------------------------------------------
 * Replaces mm_gen_cs_or_MD (LR/format.c:270-281; mm_gen_cs / mm_gen_MD :283-290; write_cs_core / write_MD_core / write_cs_or_MD
 * :150-268) for every record of a mini-batch, on the GPU: one wavefront per record walks the CIGAR over the encoded read and the 4-bit
 * reference, both already in HBM.  Bits of opt_flag that are read: MM_F_OUT_MD (0x1000000) selects MD, else MM_F_OUT_CS (0x40) selects
 * cs, in its long form with MM_F_OUT_CS_LONG (0x800) -- both MD and cs set mean MD, as in the reference --, and MM_F_QSTRAND
 * (0x100000000: the forward read against mm_idx_getseq2's reverse target, what mm_write_paf3 passes).  With neither 0x40 nor 0x1000000
 * every string is empty and nothing is launched.
 * batch: the resident reads of gdiet_hip_batch_upload (seqs / lens are then ignored), or NULL: seqs / lens (ASCII) are encoded and
 * uploaded by the call.  Output: *text (NUL-terminated) and *off, both malloc'd (free() them): record k's string is
 * text[off[k] .. off[k + 1]), records counted read-major in the order of regs[i]; off has one entry per record plus one.  The strings
 * carry no "cs:Z:" / "MD:Z:" prefix.  A record without a CIGAR (n_cigar == 0: mm_reg1_t::p == NULL) gets the empty string.
 * The reference's assertions (LR/format.c:156,199,232) are errors here, checked on the host before anything is launched: a record
 * whose CIGAR lengths do not sum to qe - qs and re - rs, with an operation other than M I D N = X, with rid out of range, re past its
 * contig or qe past its read, or (cs only) with an N operation shorter than 2 fails the whole call with GDIET_E_PARAM and a one-line
 * gdiet_hip_strerror.  The call works on a stream and buffers of its own: it may run on another caller thread while map tickets
 * (gdiet_hip_map_submit) are open on the context. */
#define GDIET_F_OUT_CS      0x40
#define GDIET_F_OUT_CS_LONG 0x800
#define GDIET_F_OUT_MD      0x1000000
int gdiet_hip_diffstr_batch(gdiet_ctx *ctx, const gdiet_index *idx, const gdiet_read_batch *batch /* or NULL */, int n_reads,
                            const char *const *seqs, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                            int64_t opt_flag, char **text, int64_t **off);

/* One SAM record exactly as mm_write_sam3 prints it for a single-segment read (LR/format.c:412-599); reg_idx < 0 writes
 * the unmapped record.  Returns the number of bytes needed (excluding the terminating NUL); writes at most cap bytes.
 * This call has no context, hence no device: the cs:Z: / MD:Z: difference tags exist in the batch calls below only, and
 * MM_F_OUT_CS / MM_F_OUT_MD in opt_flag are ignored here.  For the same reason it prints no RG:Z: tag (the read group lives in a
 * context) and, having no comment argument, no comment: MM_F_COPY_COMMENT is ignored.  MM_F_SOFTCLIP, MM_F_LONG_CIGAR and MM_F_NO_QUAL
 * are honoured as in the batch calls. */
size_t gdiet_hip_sam_record(const gdiet_index *idx, const char *qname, const char *seq, const char *qual, int32_t l_seq,
                            const gdiet_reg_t *regs, int32_t n_regs, int32_t reg_idx, int64_t opt_flag, char *buf, size_t cap);

/* All records of a batch, in input order, one per line (the body of a SAM file without the header), formatted on the context's
 * host threads -- step 2 of worker_pipeline (LR/map.c:2139-2170) for a whole mini-batch.  *out is malloc'd (free() it); returns
 * its length.  quals may be NULL, and so may its entries.
 * MM_F_OUT_CS / MM_F_OUT_CS_LONG / MM_F_OUT_MD in opt_flag (--cs[=long] / --MD) add "\tcs:Z:..." or "\tMD:Z:..." to every record with a
 * CIGAR, behind its SA:Z: tag, if any, and in front of rl:i:0 (LR/format.c:593-597): one gdiet_hip_diffstr_batch pass over the batch on
 * the GPU before the records are formatted.  Without those bits nothing is launched and the text is what it always was.  A record
 * that pass refuses makes the call return 0 with *out == NULL; gdiet_hip_strerror says why.
 * The other output bits of mm_mapopt_t::flag that are read (all host work, LR/format.c:387-602, LR/map.c:2166-2185):
 *   MM_F_NO_PRINT_2ND   (0x4000, --secondary=no) no record with 0x100
 *   MM_F_SAM_HIT_ONLY   (0x40000000, --sam-hit-only) no record for a read without alignments
 *   MM_F_NO_QUAL        (0x10, -Q)  QUAL is "*" whatever quals holds
 *   MM_F_SOFTCLIP       (0x80000, -Y) supplementary records clip with S instead of H, and supplementary and secondary records carry
 *                       the whole read as SEQ / QUAL
 *   MM_F_LONG_CIGAR     (0x10000, -L) a CIGAR of more than 65 535 operations, clips included, is printed as "<l>S<ref span>N" with
 *                       the operations in a CG:B:I tag behind the cs / MD tag
 *   MM_F_COPY_COMMENT   (0x2000000, -y) the read's comment is the last field; only the calls that take `comments` have one to print
 * and, with a read group set on the context (gdiet_hip_set_read_group), RG:Z:<id> is the first tag of every record, unmapped ones
 * included.  Paired-end fields of mm_write_sam3 (n_seg > 1) are not written: every read is a segment of its own. */
#define GDIET_F_NO_QUAL       0x10
#define GDIET_F_LONG_CIGAR    0x10000
#define GDIET_F_SOFTCLIP      0x80000
#define GDIET_F_COPY_COMMENT  0x2000000
#define GDIET_F_SAM_HIT_ONLY  0x40000000
size_t gdiet_hip_sam_batch(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                           const char *const *quals, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                           int64_t opt_flag, char **out);

/* The same into a buffer the caller keeps from mini-batch to mini-batch: *buf / *cap start as NULL / 0, are realloc'd when too small, and
 * are free()d by the caller at the end.  (The SAM text of a long-read mini-batch is ~150 MB; a fresh allocation of that size costs its
 * page faults every time.)  Returns the length of the text. */
size_t gdiet_hip_sam_batch_into(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                                const char *const *quals, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                                int64_t opt_flag, char **buf, size_t *cap);
/* gdiet_hip_sam_batch_into with the reads' comments (the array gdiet_hip_fastx_read hands out with with_comment; NULL, or NULL entries,
 * where a read has none).  A comment is printed only with MM_F_COPY_COMMENT set, behind rl:i:0, on unmapped records too
 * (LR/format.c:599).  gdiet_hip_sam_batch and gdiet_hip_sam_batch_into are this call with comments == NULL. */
size_t gdiet_hip_sam_batch_comments_into(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                                         const char *const *quals, const char *const *comments, const int32_t *lens, const int32_t *n_regs,
                                         gdiet_reg_t *const *regs, int64_t opt_flag, char **buf, size_t *cap);

/* -R: the read group (sam_write_rg_line, LR/format.c:90-126).  rg_line is the option's argument, "@RG\tID:x\tSM:y" with every tab
 * spelled as backslash-t; mm_escape turns backslash-t into a tab and two backslashes into one, and drops a backslash together with any
 * other character behind it.  GDIET_E_PARAM, with the reference's message in gdiet_hip_strerror, when the line does not start with
 * @RG, holds a literal tab, has no "	ID:" after escaping, or has an ID of more than 255 bytes -- and when it ends in a lone backslash,
 * where the reference reads past the terminator.  After a failure, and with rg_line == NULL, no read group is set.
 * The escaped line and the ID are kept in the context and read by gdiet_hip_sam_header and the SAM batch formatters: set it before
 * formatting starts, not while a formatter call runs on another thread. */
int gdiet_hip_set_read_group(gdiet_ctx *ctx, const char *rg_line);
/* The SAM header, mm_write_sam_hdr (LR/format.c:128-148): "@SQ	SN:<name>	LN:<length>" per index sequence, the context's @RG line
 * if one is set, then "@PG	ID:minimap2	PN:minimap2", "	VN:<version>" unless version is NULL, "	CL:minimap2 argv[1] ... argv[argc-1]"
 * when argc > 1, and the final newline.  *out is malloc'd (free() it); returns its length, 0 with *out == NULL on failure. */
size_t gdiet_hip_sam_header(gdiet_ctx *ctx, const gdiet_index *idx, const char *version, int argc, const char *const *argv, char **out);

/* The same for PAF output: mm_write_paf3 (LR/format.c:326-367) as step 2 prints it when MM_F_OUT_SAM is off (LR/map.c:2163-2185).
 * opt_flag: MM_F_OUT_CG (0x20, `-c`) adds the cg:Z: tag, MM_F_PAF_NO_HIT (0x8000000, --paf-no-hit) the lines of unmapped reads,
 * MM_F_NO_PRINT_2ND drops secondary records, MM_F_QSTRAND is honoured.  *out is malloc'd; returns its length.
 * This call is not given the reads, so MM_F_OUT_CS / MM_F_OUT_MD stay ignored here: gdiet_hip_paf_batch_seqs prints the tags. */
size_t gdiet_hip_paf_batch(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const int32_t *lens,
                           const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **out);
/* gdiet_hip_paf_batch plus the reads (ASCII): mm_write_paf3 with MM_F_OUT_CS / MM_F_OUT_CS_LONG / MM_F_OUT_MD, which add the cs:Z: /
 * MD:Z: tag behind cg:Z: (LR/format.c:354-356); MM_F_QSTRAND reaches the tag as it does there.  One gdiet_hip_diffstr_batch pass
 * per call; failure as in gdiet_hip_sam_batch. */
size_t gdiet_hip_paf_batch_seqs(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                                const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **out);
/* ... and with the reads' comments (as gdiet_hip_sam_batch_comments_into): under MM_F_COPY_COMMENT the comment is the last field of
 * every MAPPED line (LR/format.c:357); the lines of --paf-no-hit carry none (:329-333).  gdiet_hip_paf_batch_seqs is this call with
 * comments == NULL. */
size_t gdiet_hip_paf_batch_comments(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                                    const char *const *comments, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                                    int64_t opt_flag, char **out);

/* Read input, step 0 of worker_pipeline (LR/map.c:2095-2131): FASTA / FASTQ, plain, gzip or BGZF ("-" = stdin), one mini-batch per
 * call.  Replaces mm_bseq_open / mm_bseq_read3 / mm_bseq_close (LR/bseq.c:38-58, 80-121) with the same record grammar
 * (kseq_read, LR/kseq.h:191-232: multi-line records, names up to the first white space, the rest of the header as comment,
 * "\r\n" line ends, U -> T) and the same batching rule (records until their lengths sum to chunk_size; in fragment mode the mates
 * of the last read as well).  The arrays and strings belong to the reader and stay valid until the next call on it; comments[i]
 * and quals[i] are NULL where the reference would store none; with_qual / with_comment of the FIRST call hold for the whole file
 * (the reader parses ahead).  *n_reads == 0: end of input.  Returns GDIET_OK, or
 * GDIET_W_TRUNCATED when the input ended in a malformed record (the batch holds the records before it; the reference prints a
 * warning and goes on likewise), or GDIET_E_PARAM (cannot open / read error). */
#define GDIET_W_TRUNCATED 1
typedef struct gdiet_fastx gdiet_fastx;
int gdiet_hip_fastx_open(gdiet_fastx **fx, const char *path);
int gdiet_hip_fastx_read(gdiet_fastx *fx, int64_t chunk_size, int with_qual, int with_comment, int frag_mode, int32_t *n_reads,
                         const char *const **names, const char *const **comments, const char *const **seqs,
                         const char *const **quals, const int32_t **lens);
/* Several mini-batches in flight: take the batch the last gdiet_hip_fastx_read returned out of the reader.  Its arrays and strings
 * (the pointers that call handed out) then stay valid until gdiet_hip_fastx_batch_free, whatever is read in the meantime. */
typedef struct gdiet_fastx_batch gdiet_fastx_batch;
gdiet_fastx_batch *gdiet_hip_fastx_detach(gdiet_fastx *fx);
void gdiet_hip_fastx_batch_free(gdiet_fastx_batch *b);
/* parser threads (default 1).  Blocks of the file are cut at places that look like the start of a four-line FASTQ record and the
 * stretches parsed side by side; a stretch that does not end exactly where the next one began proves the cut wrong, and the rest of
 * the block is parsed again in sequence -- so the records are those of the sequential grammar whatever the input looks like. */
int gdiet_hip_fastx_set_threads(gdiet_fastx *fx, int n);
void gdiet_hip_fastx_close(gdiet_fastx *fx);

/* Device mode of the reader.  From the next block of the file on, the strict four-line FASTQ records at the front of every block are
 * found on ctx's device (newline ballot, scan, one thread per record) in place of kseq_read (LR/kseq.h:191-232): a record is strict
 * when its four lines are complete, start with '@' / not '@', '+', '>' / '+' / anything, hold no '\r', and sequence and quality are
 * equally long and not empty -- for such a record kseq_read consumes exactly these lines.  The first record of a block that is not
 * strict, and everything behind it, goes through the sequential grammar as before, so the records, batches (LR/bseq.c:80-121) and
 * truncation flags are those of an unattached reader on every input.  ctx == NULL detaches.  Close the reader, and free the batches
 * taken out of it, before ctx is destroyed.  Any thread may read while map tickets are open on ctx. */
int gdiet_hip_fastx_attach(gdiet_fastx *fx, gdiet_ctx *ctx);
/* gdiet_hip_fastx_read plus the resident batch of exactly those reads: *batch is what gdiet_hip_batch_upload(ctx, ..., n, seqs, lens)
 * would have built (seq_nt4_table, LR/sketch.c:11-18), NULL when no read is returned.  Reads of device-parsed chunks are encoded on the
 * device from the block that is already there -- their U / u becomes T / t in the host strings (LR/bseq.c:71-73) by a flag the encode
 * kernel sets -- and reads the host parsed are encoded and copied as gdiet_hip_batch_upload does; one batch may hold both kinds.
 * Release with gdiet_hip_batch_destroy.  Requires an attached reader (GDIET_E_PARAM otherwise).  gdiet_hip_fastx_detach and
 * gdiet_hip_fastx_batch_free work on the host arrays as before. */
int gdiet_hip_fastx_read_resident(gdiet_fastx *fx, int64_t chunk_size, int with_qual, int with_comment, int frag_mode, int32_t *n_reads,
                                  const char *const **names, const char *const **comments, const char *const **seqs,
                                  const char *const **quals, const int32_t **lens, gdiet_read_batch **batch);
/* Who parsed what since the reader was opened: records found on the device, records the host grammar returned, blocks parsed, and
 * blocks of an attached reader whose rest gave the host grammar at least one record (or a malformed one).  Any pointer may be NULL. */
int gdiet_hip_fastx_stats(const gdiet_fastx *fx, int64_t *records_device, int64_t *records_host, int64_t *blocks, int64_t *blocks_handed_over);
/* A resident batch as arrays, for tests and for a maintainer checking one: *n reads, roff[n + 1], and the roff[n] encoded bytes of the
 * host copy (enc_host) and of the device copy, downloaded (enc_device).  Sizes first: every array argument may be NULL. */
int gdiet_hip_batch_export(gdiet_ctx *ctx, const gdiet_read_batch *b, int32_t *n, int64_t *roff, uint8_t *enc_host, uint8_t *enc_device);

/* BGZF input (the blocked gzip of htslib's bgzip).  No call selects it: gdiet_hip_fastx_open reads a file raw, member by member, when it
 * is a regular file whose first gzip member carries the BC extra subfield and whose last 28 bytes are the BGZF end-of-file member, and
 * GDIET_BGZF is not 0 in the environment at that time.  The members of one read are then inflated side by side: by zlib's raw inflate on
 * the reader's threads (gdiet_hip_fastx_set_threads), or, once the reader is attached, on the device, one wavefront per member
 * (csrc/bgzf_inflate.hip.h).  The records, batches and truncation flags are those of the same bytes uncompressed.  After inflation every
 * member's length must be its ISIZE and its CRC32 its trailer's, on either route: otherwise the read fails with GDIET_E_PARAM
 * (GDIET_E_HIP when the device itself failed; nothing continues on the host for that file), and gdiet_hip_fastx_strerror, or
 * gdiet_hip_strerror of the attached context, says which member.  How many reads of earlier blocks were handed out before such an
 * error is not what gzread's stream would have given.
 * Still read through zlib's gzread, as before: single-stream gzip, stdin, and a BGZF file without its end marker.  A member without a BC
 * subfield inside a file that took the BGZF route is a read error whose message names GDIET_BGZF=0; mixed streams are not read.
 * Out of scope: the reader's CRC on the device, keeping the inflated block resident for the device's parse pass (it is uploaded again),
 * and the reference FASTA of the index build. */
/* members inflated on the device and by zlib, compressed bytes taken and bytes produced since the reader was opened: all zero for a file
 * that did not take the BGZF route.  Any pointer may be NULL. */
int gdiet_hip_fastx_bgzf_stats(const gdiet_fastx *fx, int64_t *members_device, int64_t *members_host, int64_t *bytes_in, int64_t *bytes_out);
/* the text of the reader's last read error ("" if there was none); valid until the reader is closed */
const char *gdiet_hip_fastx_strerror(const gdiet_fastx *fx);
/* The kernel-level boundary of the inflater: raw[0, raw_len) must be whole BGZF members; they are located (no inflating), inflated on the
 * device, and checked (length against ISIZE, CRC32 against the trailer, on the host).  *out_len is the sum of ISIZE; with out == NULL
 * only that is computed.  GDIET_E_PARAM with a message in gdiet_hip_strerror for a malformed range, a range that ends inside a member,
 * out_cap too small, or a member's error; the context stays usable. */
int gdiet_hip_bgzf_inflate(gdiet_ctx *ctx, const uint8_t *raw, size_t raw_len, uint8_t *out, size_t out_cap, size_t *out_len);

/* BAM input.  No call selects it and no switch: a source whose first four bytes, after decompression, are "BAM\1" is BAM -- on the BGZF
 * route, through gzread (BGZF without its end marker, stdin) and as a raw uncompressed stream alike; GDIET_BGZF=0 still only selects the
 * inflater.  The reads are DEFINED as the records gdiet_hip_fastx_read returns for the FASTQ equivalent of the file:
 *   header    consumed, not returned: l_text, the text, n_ref, and l_name, name, l_ref per reference; it may be longer than a reader block.
 *   records   every alignment record is one read, in file order, except records with FLAG 0x100 or 0x800 (secondary, supplementary),
 *             which are skipped as `samtools fastq` skips them.  CIGAR and reference fields are passed over.
 *   name      read_name up to its NUL.      len   l_seq; 0 gives an empty string.
 *   seq       the l_seq letters of "=ACMGRSVTWYHKDBN".
 *   qual      (qual[i] + 33) mod 256 per base; NULL when the first quality byte is 0xFF, when l_seq is 0 and when the reader was opened
 *             with with_qual == 0.
 *   FLAG 0x10 the sequence is reverse-complemented and the quality reversed: the read is the one the instrument produced.  The complement
 *             is the BAM writer's (csrc/bam_record.h), which is the 4-bit reversal of the code (csrc/bam_in.h proves it at compile time),
 *             so this library's own BAM output, read back, gives the reads that went in.
 *   comment   only with with_comment: the record's aux fields as SAM text, in record order, joined by tabs; NULL when there are none.
 *             Every integer type prints as i; f as the shortest decimal text, without exponent, whose float32 it is ("nan", "inf",
 *             "-inf"); A, Z, H verbatim; B as its subtype and comma-separated values.  A comment is thus a list of SAM tags, which is
 *             what -y into SAM or BAM output needs.  Made on host threads.
 * Batching is that of FASTQ input (mates in fragment mode are consecutive records with equal names).  Input that ends inside the header
 * or inside a record gives GDIET_W_TRUNCATED with the records before it.  A record that contradicts itself is a read error
 * (GDIET_E_PARAM) that surfaces behind the reads in front of it: a block_size below 32; fields that do not fit their record
 * (32 + l_read_name + 4 n_cigar_op + ceil(l_seq / 2) + l_seq > block_size); l_read_name == 0; a name without its NUL; a negative l_seq;
 * a negative count in the header; and, only when comments are asked for, an aux field that runs past the record or has no known type.
 * A record is judged once all of its block_size bytes are there.  gdiet_hip_fastx_strerror then reads "BAM record <k> at offset <o>: ..."
 * with k counting every record of the file from 0 and o the offset of its block_size field in the decompressed stream.
 * Unattached, SEQ and QUAL are unpacked on the reader's threads, records side by side; attached, by bam_unpack_kernel, one wavefront per
 * record (csrc/bam_in.hip.h), and gdiet_hip_fastx_read_resident builds the resident batch from the text that is already on the device.
 * gdiet_hip_fastx_stats counts the records of either route as records_device / records_host.  Out of scope: CRAM, SAM text input,
 * index-driven region reads, and keeping the inflated block resident between inflate and unpack. */
/* 0: the reader reads FASTA / FASTQ; 1: BAM.  Valid after the first read. */
int gdiet_hip_fastx_format(const gdiet_fastx *fx);
/* The kernel-level boundary of the unpack step: recs[0, len) must be whole uncompressed alignment records (no header).  They are walked
 * on the host, unpacked on the device and copied back: text holds seq NUL [qual NUL] per kept record, off four offsets per kept record
 * -- name and aux fields in recs (-1: no aux field), seq and qual in text (-1: no quality) -- and lens its l_seq.  *text_len and *n_reads
 * are always set; with text, off and lens all NULL nothing else happens (sizes first).  GDIET_E_PARAM with a message in
 * gdiet_hip_strerror for a malformed record, a range that ends inside a record or text_cap too small; GDIET_E_HIP if the device fails. */
int gdiet_hip_bam_in_unpack(gdiet_ctx *ctx, const uint8_t *recs, size_t len, int with_qual, char *text, size_t text_cap, size_t *text_len, int64_t *off, int32_t *lens,
                            int32_t *n_reads);

/* BGZF output.  The kernel-level boundary of the compressor: in[0, in_len) is cut into members of 65280 input bytes (the last one
 * shorter), every member is compressed by one wavefront of the device (csrc/bgzf_deflate.hip.h: LZ77 match search, dynamic, fixed or
 * stored DEFLATE blocks, CRC32) and the complete members -- header with BC subfield and BSIZE, stream, CRC32, ISIZE -- are written one
 * behind the other to out; flags & 1 appends the 28-byte end-of-file member.  A member's bytes depend on its input bytes alone.
 * *out_len is what was written; with out == NULL it is the bound ceil(in_len / 65280) * 65536 + 28 that out_cap must reach, and nothing
 * runs.  in_len == 0 writes nothing but the optional end-of-file member.  GDIET_E_PARAM, before any launch and with a message in
 * gdiet_hip_strerror, for in == NULL with a length or out_cap below the bound; GDIET_E_HIP if the device fails. */
int gdiet_hip_bgzf_deflate(gdiet_ctx *ctx, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, size_t *out_len, int flags);

/* A BGZF stream writer: path is created or truncated.  With a context the members of a write go through the kernel above (on a stream
 * and behind a lock of the context's own: a writer thread may compress while other threads map and read); with ctx == NULL they go
 * through zlib's raw deflate at `level` (-1: zlib's default, 0..9) on `threads` host threads, plus zlib's crc32.  level and threads
 * mean nothing with a context. */
typedef struct gdiet_bgzf_out gdiet_bgzf_out;
int gdiet_hip_bgzf_out_open(gdiet_ctx *ctx_or_null, const char *path, int level, int threads, gdiet_bgzf_out **out);
/* n bytes more.  Whole members of 65280 bytes are compressed and written; what is left below that waits for the next call, so members
 * are full except where a flush or the close ends one.  An error of the device (GDIET_E_HIP), of zlib or of write() -- a short write
 * is one -- (GDIET_E_PARAM) leaves its message in gdiet_hip_strerror(ctx_or_null) for the calling thread; the writer then refuses
 * everything but its close. */
int gdiet_hip_bgzf_out_write(gdiet_bgzf_out *h, const void *bytes, size_t n);
/* what is waiting becomes a (shorter) member now */
int gdiet_hip_bgzf_out_flush(gdiet_bgzf_out *h);
/* flushes, writes the end-of-file member, closes the file and frees the writer, whatever it returns */
int gdiet_hip_bgzf_out_close(gdiet_bgzf_out *h);
/* members compressed by the device and by zlib, bytes taken and bytes written to the file so far.  Any pointer may be NULL. */
int gdiet_hip_bgzf_out_stats(const gdiet_bgzf_out *h, int64_t *members_device, int64_t *members_host, int64_t *bytes_in, int64_t *bytes_out);

/* ---- BAM output ----------------------------------------------------------------------------------------------------------------------
 * The reference writes no BAM.  A BAM alignment record (SAM specification 4.2; all integers little-endian) is defined here as a fixed
 * function of the SAM line gdiet_hip_sam_batch_comments_into prints for the same arguments, so the SAM text, which is pinned to the
 * reference, stays the oracle (tests/bam_ref.py restates the function):
 *   RNAME -> refID (its index in the index; -1 for "*"), POS - 1 -> pos, MAPQ, FLAG; next_refID = next_pos = -1, tlen = 0;
 *   CIGAR -> n_cigar_op words len << 4 | op (MIDNSHP=X = 0..8), clips included, "*" -> none.  More than 65 535 operations, clips
 *            included: the two operations <l_seq>S<reference length>N and the real ones in a CG:B:I tag, placed where MM_F_LONG_CIGAR
 *            puts it in the SAM line (behind cs / MD, in front of rl) -- whether or not that bit is set: BAM has no other way;
 *   bin    = reg2bin(pos, pos + reference length of the real CIGAR, or pos + 1 if that is 0); 4680 for an unmapped record;
 *   SEQ    -> 4-bit codes, the index of the upper-cased letter in "=ACMGRSVTWYHKDBN", 15 for any other byte; high nibble first.  SEQ is
 *            taken from the read's text (seqs[i]), so IUPAC letters keep their codes.  "*" -> l_seq = 0 and no qualities;
 *   QUAL   -> byte - 33; "*" -> l_seq bytes of 0xff;
 *   tags in the order of the line: integers as the smallest type that holds the value (c s i for negative values, C S I otherwise),
 *            A one byte, Z / H text and NUL, de:f: the float32 nearest to the decimal text printed, B:I the CG array;
 *   the comment (MM_F_COPY_COMMENT): every tab-separated field must itself be a tag XX:T:value, T in A i f Z H B (B subtypes cCsSiIf),
 *            and is stored as that tag.  A comment that is no list of tags cannot be stored: the batch call fails with GDIET_E_PARAM
 *            and a message that names the read.  So does a read name of more than 254 bytes.
 * Which records exist is decided exactly as in the SAM batch calls (MM_F_NO_PRINT_2ND, MM_F_SAM_HIT_ONLY, MM_F_SOFTCLIP, MM_F_NO_QUAL,
 * MM_F_COPY_COMMENT, the cs / MD bits with their pass on the GPU, the context's read group, = / X operations as they come in regs).
 * The records are written on the GPU, one wavefront per record (csrc/bam_encode.hip.h), from a table the context's host threads
 * flatten; a stream and a lock of the context's own, so a writer thread may encode while other threads map.  Failures of these calls
 * leave their text in gdiet_hip_strerror(ctx) for the calling thread.  Paired-end fields are out of scope; coordinate order and the index: "Sorted BAM output" below. */

/* The BAM header: "BAM\1", l_text and the text gdiet_hip_sam_header returns for the same arguments (no NUL), n_ref, and per index sequence
 * l_name (with NUL), the name and its NUL, l_ref.  *out is malloc'd (free() it); returns its length, 0 with *out == NULL on failure. */
size_t gdiet_hip_bam_header(gdiet_ctx *ctx, const gdiet_index *idx, const char *version, int argc, const char *const *argv, char **out);
/* The uncompressed BAM records of a batch, in input order, one behind the other (each with its block_size), into a buffer the caller
 * keeps from mini-batch to mini-batch: the argument shape of gdiet_hip_sam_batch_comments_into (*buf / *cap start as NULL / 0, are
 * realloc'd when too small, and are free()d by the caller; quals, comments and their entries may be NULL).  This is the kernel-level
 * boundary of the encoder: the records are encoded on the device and copied back.  Returns the number of bytes -- 0 for a batch that
 * yields no record, which is no failure --, or a negative GDIET_E_* code: GDIET_E_PARAM for a comment that is no tag list, a name of
 * more than 254 bytes, a record whose rid / qs / qe lie outside the index or the read, or a record the difference-string pass refuses;
 * GDIET_E_HIP if the device fails. */
int64_t gdiet_hip_bam_batch_into(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                                 const char *const *quals, const char *const *comments, const int32_t *lens, const int32_t *n_regs,
                                 gdiet_reg_t *const *regs, int64_t opt_flag, char **buf, size_t *cap);
/* The same records appended to a BGZF stream writer (write the header with gdiet_hip_bgzf_out_write first).  On a writer opened with a
 * context -- it must be ctx -- the uncompressed records never reach the host: the writer's waiting tail (under 65280 bytes) is uploaded
 * in front of a resident buffer, the records are encoded behind it, every whole member of 65280 bytes is compressed from that buffer by
 * the deflate kernel, the members come down and are written, and what is left below a member comes down as the next tail.  The file's
 * bytes are those of gdiet_hip_bam_batch_into followed by gdiet_hip_bgzf_out_write, which is what the call does on a writer without a
 * context (the records are still encoded on ctx's device).  gdiet_hip_bgzf_out_stats counts these members like any others.  Returns
 * GDIET_OK or the codes of gdiet_hip_bam_batch_into and gdiet_hip_bgzf_out_write. */
int gdiet_hip_bgzf_out_write_bam(gdiet_bgzf_out *h, gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames,
                                 const char *const *seqs, const char *const *quals, const char *const *comments, const int32_t *lens,
                                 const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag);

/* ---- SAM text on the device --------------------------------------------------------------------------------------------------------------
 * The SAM lines of a batch written by the GPU, one wavefront per line (csrc/sam_encode.hip.h, the statements of csrc/sam_record.h), from
 * a table the context's host threads flatten (csrc/sam_flatten.h).  The bytes are exactly those of gdiet_hip_sam_batch_comments_into
 * for the same arguments and flags -- gd_write_sam's rules, not BAM's: a name of any length, a comment of any text, the CIGAR in a
 * CG:B:I tag only under MM_F_LONG_CIGAR (behind the cs / MD tag), MM_F_NO_QUAL, MM_F_SOFTCLIP, MM_F_COPY_COMMENT, MM_F_SAM_HIT_ONLY and
 * MM_F_NO_PRINT_2ND as in the host formatter, the cs / MD strings from the same pass on the GPU, the context's read group.  The host
 * lays out what only it holds as ready text (RG:Z:, SA:Z:, the difference tag, the comment, the text of de:f:); every number, the CIGAR
 * column, SEQ (reversed and complemented on the reverse strand) and QUAL are formatted on the device.  Line sizes are arithmetic on the
 * rows, so one kernel writes every line at its final offset.  The route is opt-in: no other call changes.  The calls run on the BAM
 * encoder's stream and lock.  Out of scope: PAF, gdiet_hip_sam_record, the header (gdiet_hip_sam_header), SEQ / QUAL taken from the
 * device reader's resident block, difference strings kept resident between their pass and this kernel, paired-end fields. */

/* The kernel-level boundary: the text comes down into a buffer the caller keeps (*buf / *cap as in gdiet_hip_sam_batch_comments_into;
 * NUL-terminated).  Returns its length -- 0 for a batch that yields no line, which is no failure --, or a negative GDIET_E_* code:
 * GDIET_E_PARAM for a record whose rid / qs / qe lie outside the index or the read, or with a clip of 2^28 bases or more (a clip travels
 * as a CIGAR operation, so the limit is BAM's; gdiet_hip_strerror(ctx) names the read), or one the difference-string pass refuses, GDIET_E_NOMEM, GDIET_E_HIP if the device fails. */
int64_t gdiet_hip_sam_batch_device_into(gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                                        const char *const *quals, const char *const *comments, const int32_t *lens, const int32_t *n_regs,
                                        gdiet_reg_t *const *regs, int64_t opt_flag, char **buf, size_t *cap);
/* The same lines appended to a BGZF stream writer (write the header with gdiet_hip_bgzf_out_write first).  On a writer opened with a
 * context -- it must be ctx -- the route of gdiet_hip_bgzf_out_write_bam: the writer's waiting tail goes up in front of a resident
 * buffer, the lines are written behind it, every whole member of 65280 bytes is compressed from that buffer, the members come down and
 * are written, and what is left below a member comes down as the next tail; the uncompressed text never reaches the host.  On a writer
 * without a context the text is formatted on ctx's device, comes down and goes through gdiet_hip_bgzf_out_write.  Either way the
 * file's bytes are those of that second route.  Returns GDIET_OK or the codes of gdiet_hip_sam_batch_device_into and
 * gdiet_hip_bgzf_out_write. */
int gdiet_hip_bgzf_out_write_sam(gdiet_bgzf_out *h, gdiet_ctx *ctx, const gdiet_index *idx, int n_reads, const char *const *qnames,
                                 const char *const *seqs, const char *const *quals, const char *const *comments, const int32_t *lens,
                                 const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag);

/* ---- Sorted BAM output ---------------------------------------------------------------------------------------------------------------
 * Coordinate order, and the BAI index of a file in that order.  Definitions (tests/bam_sort_ref.py restates them):
 *   ORDER   records are sorted by key = (uint32)refID << 32 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1), the low word computed in 32 bits.
 *           refID -1 becomes 0xFFFFFFFF: unplaced records come last.  pos -1 comes first within its contig.  On equal position the
 *           forward strand comes before the reverse strand.  Records with equal keys keep their input order: the sort is stable, so the
 *           output is a function of the input records alone.
 *   HEADER  gdiet_hip_bam_header_so: gdiet_hip_bam_header with "@HD\tVN:1.6\tSO:<sort_order>\n" as the first line of the text.
 *   INDEX   <path>.bai, SAM specification 5.2: "BAI\1", n_ref, per reference the bins with their chunks and the linear index, n_no_coor.
 *           - A record covers [pos, pos + max(ref_len, 1)); ref_len is the sum of the M / D / N / = / X operations of the record's own
 *             CIGAR field (a record with the <l_seq>S<ref_len>N placeholder is covered by this rule without reading CG).  The windows
 *             of the linear index run from max(pos, 0) >> 14 to (max(pos + max(ref_len, 1), 1) - 1) >> 14.
 *           - The record's bin is the bin field it carries.
 *           - A chunk is a maximal stretch of consecutive records of one reference with one bin; it runs from the first record's start
 *             virtual offset to the last record's end virtual offset.  Bins are written in ascending bin number, a bin's chunks in file
 *             order.
 *           - Pseudo-bin 37450 comes last for every reference that has a record: {first start, last end}, {mapped, unmapped-but-placed}.
 *             A reference without a record has n_bin = 0 and n_intv = 0.
 *           - ioffset[w] is the start virtual offset of the first record covering the 16 kbp window w; n_intv is the last covered
 *             window + 1; an uncovered window takes the value of the next covered one to its right.
 *           - Virtual offset = member_file_offset << 16 | offset_in_member.  A stream offset lies in the first member that ends behind
 *             it; the end of the stream is the file offset of the end-of-file member << 16.
 *           - n_no_coor counts the records whose refID is outside [0, n_ref).
 *           No claim is made that the bytes equal those of `samtools index`.  A contig longer than 2^29 cannot be indexed (CSI is out of
 *           scope).
 * The device pass (csrc/bam_sort.hip.h) reads nothing but the records' own bytes, so it sorts any BAM records: bam_key_kernel (one thread
 * per record: key and size from refID, pos, flag and block_size, assembled from byte loads), hipCUB's stable radix sort and exclusive
 * scan, and bam_gather_kernel (one wavefront per output record: the copy to the sorted offset, the reference length of the CIGAR field, and
 * one 32-byte index row).  It runs on a lane of the context's own.  The host side of the merge of several sorted runs (csrc/bam_sorter.h:
 * gdq_plan_chunks) and of the index (csrc/bam_index.h: gdx_bai_build) is host-only code.  Out of scope: CSI / tabix indexes, name sort,
 * merging existing BAM files, compressed spools, paired-end fields, sorted SAM text. */

/* gdiet_hip_bam_header with "@HD\tVN:1.6\tSO:<sort_order>\n" in front of the text ("coordinate" for a sorted file; letters only, or the
 * call fails).  *out is malloc'd (free() it); returns its length, 0 with *out == NULL on failure. */
size_t gdiet_hip_bam_header_so(gdiet_ctx *ctx, const gdiet_index *idx, const char *version, int argc, const char *const *argv, const char *sort_order, char **out);

/* One 32-byte row per record of a sorted buffer, in sorted order: what the index needs of a record.  end = pos + max(ref_len, 1). */
typedef struct {
	uint64_t key, out_offset;
	int32_t refID, pos, end;
	uint16_t bin, flag;
} gdiet_bam_row_t;
/* The kernel-level boundary of the sort pass: recs[0, len) holds whole uncompressed BAM records (any records, each with its block_size;
 * under 2 GiB).  The host walks them for their starts, the device sorts them into out[0, len) and writes rows[k] for the record at place
 * k (rows_cap: bytes rows holds; 32 per record are needed); both are copied back.  *n_rec takes the number of records.  With out and
 * rows both NULL only *n_rec is set.  Returns len, or a negative code: GDIET_E_PARAM for a malformed record (the text of
 * gdiet_hip_strerror(ctx) names it as the BAM reader does) or too small a rows, GDIET_E_HIP if the device fails. */
int64_t gdiet_hip_bam_sort_records(gdiet_ctx *ctx, const void *recs, size_t len, void *out, void *rows, size_t rows_cap, int64_t *n_rec);

/* The sorter: a coordinate-sorted BAM file, and its index, from mapped batches in any order.  open takes the uncompressed header
 * (gdiet_hip_bam_header_so(..., "coordinate", ...)) and writes it; add encodes a batch -- the batch arguments of
 * gdiet_hip_bam_batch_into -- into a resident run buffer; a run that would exceed run_bytes (0: 512 MiB) is sorted on the device and
 * spooled, uncompressed, to a file in tmp_dir (NULL: the output's directory) that is created and unlinked at once; close merges the
 * runs in chunks of at most chunk_bytes (0: 256 MiB) on the device -- or, if one run was all, writes its sorted buffer as it is --,
 * ends the file and writes <path>.bai if want_index.  bgzf_device: the stream is compressed from the resident buffer by the deflate
 * kernel; otherwise by zlib at `level` on `threads` host threads.  The output is a function of the input records alone.
 * open fails with GDIET_E_PARAM for a header that is none, a tmp_dir that cannot be written (the text names it), an output that cannot
 * be created, and, with want_index, a contig longer than 2^29 (the text names it).  *out still takes a handle then -- unless an
 * argument was NULL --: it refuses add, and its close frees it and returns GDIET_OK, having created nothing.  After a failed add --
 * GDIET_E_PARAM as gdiet_hip_bam_batch_into, or for the 2^31st record of a file (the merge sorts all keys in one call that counts them in
 * an int; 2^32 is not reached); GDIET_E_HIP for the device, a short spool or output write -- the sorter refuses everything but close,
 * which always frees the handle and the spools, removes a partial .bai, and returns the failure's code.  Texts are
 * gdiet_hip_strerror(ctx)'s, for the calling thread.  One thread at a time per sorter. */
typedef struct gdiet_bam_sorter gdiet_bam_sorter;
typedef struct {
	int64_t records, runs, spooled_bytes, chunks, members, n_no_coor;
	double seconds[5]; /* device: key + sort, gather; wall: spool write, spool read, compress + write */
} gdiet_bam_sort_stats_t;
int gdiet_hip_bam_sort_open(gdiet_ctx *ctx, const char *path, const void *header, size_t header_len, int bgzf_device, int level, int threads,
                            uint64_t run_bytes, uint64_t chunk_bytes, const char *tmp_dir, int want_index, gdiet_bam_sorter **out);
int gdiet_hip_bam_sort_add(gdiet_bam_sorter *h, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs,
                           const char *const *quals, const char *const *comments, const int32_t *lens, const int32_t *n_regs,
                           gdiet_reg_t *const *regs, int64_t opt_flag);
int gdiet_hip_bam_sort_close(gdiet_bam_sorter *h, gdiet_bam_sort_stats_t *stats);

/* ---- Duplicate marking ---------------------------------------------------------------------------------------------------------------
 * Bit 0x400 of BAM alignment records, decided on the device: the step between sort and index of a post-mapping toolchain (samtools
 * markdup, Picard MarkDuplicates).  The reference writes no duplicate flags: these rules are the definition (tests/markdup_ref.py
 * restates them).  Single-end only.
 *   ELIGIBLE  a record with (flag & 0xB04) == 0 (not unmapped, secondary, QC-fail or supplementary), refID >= 0 and pos >= 0.  An
 *             ineligible record is written exactly as it came; a 0x400 it carries stays.
 *   THE REAL CIGAR  as for Coverage: the record's n_cigar_op words, or the CG:B:I array of a placeholder record.
 *   U         the unclipped 5' coordinate, from the real CIGAR, the sums taken in 64 bits:
 *             forward strand:          u = pos - (sum of the S and H lengths in front of the first other operation)
 *             reverse strand (0x10):   u = pos + (sum of the M D N = X lengths) - 1 + (sum of the S and H lengths behind the last other
 *                                      operation)
 *             A CIGAR of S and H alone (or none) has all of its lengths in both clip sums.
 *   GROUP     the eligible records with equal (refID, u, strand).  The group key is refID << 34 | (u + 2^32) << 1 | strand; the all-ones
 *             word marks an ineligible record, so -2^32 <= u <= 2^32 - 2 and refID < 2^30 are required: on these the key is injective.
 *   SCORE     the sum, as uint32, of the QUAL bytes q with 15 <= q and q != 0xFF (Picard's sum of base qualities): missing qualities
 *             score 0.
 *   WINNER    the highest score of the group; among equal scores the record that comes first in the output order (the file's order for
 *             the sorter, the buffer's for gdiet_hip_bam_markdup_records).  Bit 0x400 of every eligible record is cleared and then set
 *             on every member of a group but its winner.  Nothing else of a record changes: not its size, its bin or its place -- the
 *             sort key does not read the bit --, so the marked file, like the sorted one, is a function of the input records alone.
 *   BAD       a record is bad if its fixed fields, name, CIGAR, SEQ and QUAL do not fit its block_size, it is a placeholder without a
 *             well-formed CG:B:I tag or the aux walk to that tag leaves the record (every record: the reasons of Coverage's record
 *             head); or, eligible, an operation code of its real CIGAR is above 8, or u or refID leave the range of the key.  A bad
 *             record fails the call with GDIET_E_PARAM, the text names the first one and its reason, and nothing is written; the
 *             sorter then takes nothing but its close.
 *   STATS     examined (records seen), eligible, duplicates (bits set), max_group (members of the largest group; 0 without an eligible
 *             record).
 * The device passes (csrc/bam_markdup.hip.h): dup_key_kernel (one wavefront per record: u and the score, one entry {key, score} per
 * record), two stable hipCUB radix sorts of the entries -- by descending score, then by key --, dup_decide_kernel (one thread per sorted
 * entry: an entry whose key equals its predecessor's sets the bit of its place) and dup_apply_kernel (one thread per record: the bit
 * rewritten where the record is resident).  In the sorter the entries of a spooled run stay on the host (12 bytes per record), and one
 * decision covers the whole file before its first chunk is streamed: groups span runs and chunks.  A Coverage or Pileup attached to
 * the sorter scatters at add, before any flag exists, and so still counts duplicates: feed it the finished records (add_bam) to
 * leave them out.  Out of scope: removing duplicates, optical duplicates, UMI / barcode-aware grouping, marking the secondary and
 * supplementary records of a duplicate, paired-end rules, a library-size estimate, an @PG line, unsorted BAM output. */
typedef struct {
	int64_t examined, eligible, duplicates, max_group;
} gdiet_dup_stats_t;
/* The kernel-level boundary: recs[0, len) holds whole uncompressed BAM records in any order (under 2 GiB); out[0, len) takes them with
 * bit 0x400 rewritten under the rule, the buffer's order breaking ties.  Returns len, or a negative code: GDIET_E_PARAM for a range that
 * ends inside a record or a bad record (out is then not written), GDIET_E_HIP if the device fails. */
int64_t gdiet_hip_bam_markdup_records(gdiet_ctx *ctx, const void *recs, size_t len, void *out, gdiet_dup_stats_t *dup_stats);
/* Duplicate marking of a sorter's file, off by default: chosen before the first gdiet_hip_bam_sort_add (GDIET_E_PARAM afterwards).  With
 * it off the sorter launches exactly what it launches without this call. */
int gdiet_hip_bam_sort_set_markdup(gdiet_bam_sorter *h, int on);
/* gdiet_hip_bam_sort_close that also hands out the duplicate counts (all 0 with marking off); either pointer may be NULL. */
int gdiet_hip_bam_sort_close_dup(gdiet_bam_sorter *h, gdiet_bam_sort_stats_t *stats, gdiet_dup_stats_t *dup_stats);

/* ---- Coverage ------------------------------------------------------------------------------------------------------------------------
 * Per-contig coverage and depth, a flag summary, mean depth per fixed window and the depth of any interval, accumulated on the device
 * from uncompressed BAM alignment records (SAM specification 4.2) while they are resident there.  The reference prints SAM and stops:
 * these rules are the definition (tests/cov_ref.py restates them).  The reference dictionary is the index's contigs
 * (gdiet_hip_index_info): n_ref lengths.  Options: excl_flags (usual value 0x704: unmapped, secondary, QC-fail, duplicate; supplementary
 * records count), min_mapq (0) and window (0: no window table).
 *   THE REAL CIGAR  is the record's n_cigar_op words, unless they are the placeholder of specification 4.2.2 -- n_cigar_op == 2, word 0 ==
 *           l_seq << 4 | S, word 1 an N --: then it is the array of the first CG tag met by walking the aux fields (types A c C s S i I f
 *           Z H B), which must be CG:B:I.  The aux fields are walked for a placeholder only, and only up to that tag.
 *   BAD     a record is bad if: refID >= n_ref; refID >= 0 and pos < 0; an operation code of the real CIGAR is above 8; refID >= 0 and
 *           pos + (sum of the M D N = X lengths) lies past the contig; l_seq > 0 and the sum of the M I S = X lengths is above l_seq; it is
 *           a placeholder without a well-formed CG:B:I tag; the aux walk leaves the record or meets an unknown type; or its fixed fields,
 *           name, CIGAR, SEQ and QUAL do not fit its block_size (l_seq below 0 included).  A negative refID is never bad by itself.  A bad
 *           record adds to no array and to no contig's counters; it is counted in `bad`, and its flag bits still count in the summary.
 *           The add call that saw it returns GDIET_E_PARAM, the text names the call's first bad record (its index and the reason), and the
 *           accumulator then refuses every add and finish: only close is left.
 *   SUMMARY over every record seen: records; unmapped (0x4), secondary (0x100), supplementary (0x800); primary_mapped (none of the three);
 *           reverse (0x10 on a record without 0x4); then exactly one of bad, excluded_by_flag ((flag & excl_flags) != 0),
 *           excluded_by_mapq (mapq < min_mapq), counted (refID >= 0) -- tested in this order -- or none (an unplaced record that passes).
 *   COUNTED a counted record adds 1 to its contig's n_reads and its mapq to sum_mapq, and walks its real CIGAR with a reference cursor
 *           from pos and a query cursor from 0: M = X give every reference position of the run +1 depth, add the run's length to
 *           sum_depth and, if the record has qualities (l_seq > 0 and qual[0] != 0xff), the stored quality bytes of the run's query bases
 *           to sum_baseq and the run's length to n_baseq, and advance both cursors; D N advance the reference cursor, I S the query
 *           cursor, H P neither.  A counted record without operations adds to n_reads and sum_mapq only.
 *   RESULTS per contig n_reads, cov_bases (positions with depth > 0), sum_depth, sum_mapq, sum_baseq, n_baseq; with window > 0 per contig
 *           ceil(len / window) windows (the last one short), each with cov_bases and sum_depth; depth is uint32 per position.  Input that
 *           drives one position above 2^31 - 1 is out of contract.  Every result is an integer and a function of the multiset of input
 *           records alone: no float is formed on the device, and nothing depends on the order of atomic arrivals, on how the records were
 *           cut into calls, on the scan's chunk or on the route that delivered them.
 * The device side (csrc/cov.hip.h, statements in csrc/cov.h): cov_scatter_kernel, one wavefront per record, validates, then adds +1 / -1
 * per M = X run into an int32 difference array over the whole reference (total_len + 1 slots, contigs back to back, 64-bit offsets);
 * finish turns it into the depth array by hipCUB's inclusive sum in chunks of at most 2^30 slots (the previous chunk's last depth is added
 * to a chunk's first slot first) and cov_window_kernel, one wavefront per window, reduces it.  The array costs 4 bytes per reference
 * base for as long as the handle lives: 12.4 GB for a GRCh38-sized reference of 3.1 Gbp.  Out of scope: per-base quality thresholds,
 * the histograms of `samtools stats` (they are "Alignment statistics" below), duplicate marking, references too large for 4 bytes per base, merging the accumulators of several
 * GPUs. */
typedef struct gdiet_coverage gdiet_coverage;
typedef struct {
	uint64_t records, unmapped, secondary, supplementary, primary_mapped, reverse, excluded_by_flag, excluded_by_mapq, counted, bad;
} gdiet_cov_summary_t;
typedef struct {
	uint64_t n_reads, cov_bases, sum_depth, sum_mapq, sum_baseq, n_baseq;
} gdiet_cov_contig_t;
/* An accumulator over idx's contigs: allocates and clears the difference array (plain hipMalloc) and the counters.  GDIET_E_NOMEM, with
 * the array's size in the text, if the device has too little memory; GDIET_E_PARAM for an index without contigs.  The array also goes
 * when the context is destroyed: a handle that outlives its context takes nothing but close. */
int gdiet_hip_cov_open(gdiet_ctx *ctx, const gdiet_index *idx, uint32_t excl_flags, uint32_t min_mapq, uint32_t window, gdiet_coverage **out);
/* The kernel-level boundary for host records: recs[0, len) holds whole records, each with its block_size.  The host walks the
 * block_size fields for the starts (a block_size below 32 or a range that ends inside a record: GDIET_E_PARAM, nothing was seen and the
 * accumulator stays usable), the records go up and are scattered.  GDIET_E_PARAM for a bad record (above), GDIET_E_HIP for the device. */
int gdiet_hip_cov_add_bam(gdiet_coverage *cov, const void *recs, size_t len);
/* A mapped batch -- the batch arguments of gdiet_hip_bam_batch_into; opt_flag decides which records exist exactly as there --: flattened
 * and encoded on the device by the BAM encoder, scattered from the resident records; nothing is copied down.  Errors as
 * gdiet_hip_bam_batch_into, and GDIET_E_PARAM for a bad record. */
int gdiet_hip_cov_add(gdiet_coverage *cov, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                      const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag);
/* Attach an accumulator (NULL: detach) to a BGZF writer with a context or to a sorter: every later gdiet_hip_bgzf_out_write_bam /
 * gdiet_hip_bam_sort_add scatters from the records it has just encoded, on the stream that holds them, before they are compressed or
 * sorted; the bytes written do not change.  A poisoned or finished accumulator makes those calls fail before they encode.  A writer
 * without a context is refused (GDIET_E_PARAM): its records are on the host.  One accumulator has one producer at a time (it carries a
 * mutex of its own); the caller keeps it open for as long as it is attached. */
int gdiet_hip_bgzf_out_set_coverage(gdiet_bgzf_out *writer, gdiet_coverage *cov);
int gdiet_hip_bam_sort_set_coverage(gdiet_bam_sorter *sorter, gdiet_coverage *cov);
/* The inclusive sum, the window reduction and the counters: contigs_out[0, n_ref) and *summary_out (either may be NULL).  After it the
 * accumulator is read-only: add is refused, finish again returns the same figures.  _chunked: the scan's chunk in slots (0: the
 * default, 2^28; at most 2^30) -- the results do not depend on it; it exists so that tests cross chunk borders on small references. */
int gdiet_hip_cov_finish(gdiet_coverage *cov, gdiet_cov_contig_t *contigs_out, gdiet_cov_summary_t *summary_out);
int gdiet_hip_cov_finish_chunked(gdiet_coverage *cov, uint64_t chunk, gdiet_cov_contig_t *contigs_out, gdiet_cov_summary_t *summary_out);
/* After finish, on an accumulator opened with window > 0: the windows of contig rid.  Returns their number; with both outputs NULL that
 * is all (the size first), else cap, the room of each output in windows, must hold them (GDIET_E_PARAM otherwise). */
int64_t gdiet_hip_cov_windows(gdiet_coverage *cov, uint32_t rid, uint32_t *cov_bases_out, uint64_t *sum_depth_out, size_t cap);
/* After finish: out[0, end - beg) takes the depth of positions [beg, end) of contig rid (0-based, end <= the contig's length). */
int gdiet_hip_cov_depth(gdiet_coverage *cov, uint32_t rid, uint32_t beg, uint32_t end, uint32_t *out);
/* Frees the arrays and the handle, whatever state it is in. */
int gdiet_hip_cov_close(gdiet_coverage *cov);

/* ---- Pileup --------------------------------------------------------------------------------------------------------------------------
 * What the reads show at every position of a list of regions: eight counters per position, accumulated on the device from uncompressed
 * BAM alignment records while they are resident there, and, after finish, a consensus byte per position and the variant sites, formed
 * on the device in integers.  The reference prints SAM and stops: these rules are the definition (tests/pile_ref.py restates them).
 *   REGIONS  (rid, beg, end), 0-based and half-open, given at open.  Refused with GDIET_E_PARAM, the text naming the first offending
 *           region: an empty region (beg >= end), a region past its contig (rid >= n_ref or end > the contig's length), a list that is
 *           not sorted by (rid, beg), overlapping regions.  Abutting regions are allowed.  An empty list means every contig whole.
 *           The positions are numbered region after region with 64-bit offsets; T is their total.
 *   COUNTERS eight uint32 per position in the order A C G T N DEL INS REV: 32 bytes per position, 32 * T bytes of plain hipMalloc for as
 *           long as the handle lives (GDIET_E_NOMEM carries the size in its text): 99 GB for a whole GRCh38 of 3.1 Gbp, 32 MB per Mbp
 *           of panel.  A counter driven above 2^32 - 1, or a depth above it, is out of contract.
 *   WHICH RECORDS COUNT  the real CIGAR, the bad-record reasons and the filter chain are those of "Coverage": bad, then excl_flags, then
 *           min_mapq.  One category is added in front of `counted`: no_seq, a placed record that passes the filters but has l_seq == 0.
 *           The summary is coverage's ten counters, then no_seq, then skipped_baseq.
 *   WALK    of a counted record, with a reference cursor r from pos and a query cursor q from 0:
 *           M = X   for every base b of the run whose position r + b lies in a region: if the record has qualities (qual[0] != 0xff)
 *                   and qual[q + b] < min_baseq, the base adds 1 to skipped_baseq and to no counter; otherwise the SEQ nibble at q + b
 *                   selects the counter -- 1 A, 2 C, 4 G, 8 T, any other code ('=' included) N -- and a record with flag 0x10 also adds
 *                   1 to REV.  Both cursors advance.
 *           D       DEL += 1 at every position of the run that lies in a region; no quality test.  Only r advances.
 *           N       only r advances.
 *           I       if r > pos (an operation before it has consumed reference) and position r - 1 lies in a region, INS += 1 there:
 *                   one count per insertion, whatever its length.  Otherwise it is not counted.  Only q advances.
 *           S       only q advances.   H P   neither cursor advances.
 *           A position outside every region is skipped silently; a run may cross several regions and the gaps between them.
 *   BAD     a bad record touches nothing, fails its call with GDIET_E_PARAM naming the call's first bad record and its reason, and
 *           poisons the handle, exactly as in "Coverage".
 *   CALLS   after finish, with min_depth, min_alt and a fraction num / den (den > 0); no float is formed on the device.
 *           depth = A + C + G + T + N + DEL.  The reference base is that of the index's packed reference S: 0..3, 4 for N.
 *           The consensus byte of a position is 'N' if depth < min_depth or all of A C G T DEL are 0, else the largest of A C G T DEL,
 *           ties going to the earlier in that order, written A C G T *.
 *           A position is a site if depth >= min_depth and (some allele k of A C G T DEL other than the reference base has cnt[k] >=
 *           min_alt and (uint64)cnt[k] * den >= (uint64)num * depth, or INS >= min_alt and (uint64)INS * den >= (uint64)num * depth).
 *           At a reference N every one of A C G T DEL is "other".  Sites come out in position order, region after region, as rows
 *           {rid, pos, ref, alt, depth, cnt[8]}: ref 0..4; alt 0..3 for A C G T, 4 for DEL, 5 for INS -- the largest qualifying allele
 *           of A C G T DEL with the same tie order, 5 only when none of them qualifies.
 *   Every result is a function of the multiset of input records, the regions and the options alone: it does not depend on how the
 *   records were cut into calls, on the route, on the scan's chunk or on the order of atomic arrivals.
 * The device side (csrc/pile.hip.h, statements in csrc/pile.h, which reuses those of csrc/cov.h): pile_scatter_kernel, one wavefront
 * per record, validates as coverage does, then takes the runs of every round of 64 operations one after another, the positions of a run
 * dealt over the 64 lanes, each lane reading its own SEQ nibble and QUAL byte and adding with a plain integer atomic.
 * pile_call_kernel, one thread per position, writes the consensus byte and a 0 / 1 site flag; hipCUB's exclusive sum over the flags,
 * in chunks of at most 2^30 positions with a carry, gives the sites' offsets and pile_site_kernel writes the rows.  Out of scope:
 * per-strand counters per allele, the inserted sequences, genotype likelihoods, VCF, merging the accumulators of several GPUs,
 * regions given after open. */
typedef struct gdiet_pileup gdiet_pileup;
typedef struct { uint32_t rid, beg, end; } gdiet_pile_region_t;
typedef struct {
	uint64_t records, unmapped, secondary, supplementary, primary_mapped, reverse, excluded_by_flag, excluded_by_mapq, counted, bad, no_seq, skipped_baseq;
} gdiet_pile_summary_t;
typedef struct { uint32_t rid, pos, ref, alt, depth, cnt[8]; } gdiet_pile_site_t;
/* An accumulator over regions[0, n_regions) of idx's contigs (n_regions == 0: every contig whole): allocates and clears the counters.
 * idx must stay alive for as long as the handle is used: the calls read its packed reference.  The counters also go when the context is
 * destroyed: a handle that outlives its context takes nothing but close. */
int gdiet_hip_pile_open(gdiet_ctx *ctx, const gdiet_index *idx, const gdiet_pile_region_t *regions, size_t n_regions, uint32_t excl_flags, uint32_t min_mapq, uint32_t min_baseq,
                        gdiet_pileup **out);
/* Host records and a mapped batch: as gdiet_hip_cov_add_bam and gdiet_hip_cov_add (opt_flag decides which records exist). */
int gdiet_hip_pile_add_bam(gdiet_pileup *pile, const void *recs, size_t len);
int gdiet_hip_pile_add(gdiet_pileup *pile, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                       const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag);
/* Attach (NULL: detach) to a BGZF writer with a context or to a sorter, beside gdiet_hip_bgzf_out_set_coverage /
 * gdiet_hip_bam_sort_set_coverage and under their rules; a coverage and a pileup accumulator may be attached at once.  The bytes
 * written do not change.  Lock order: the encoder's mutex, the coverage accumulator's, the pileup accumulator's, the context's lane. */
int gdiet_hip_bgzf_out_set_pileup(gdiet_bgzf_out *writer, gdiet_pileup *pile);
int gdiet_hip_bam_sort_set_pileup(gdiet_bam_sorter *sorter, gdiet_pileup *pile);
/* The summary (may be NULL).  After it the accumulator is read-only: add is refused, finish again returns the same figures.  _chunked:
 * the chunk, in positions, of the exclusive sum that _sites runs (0: the default, 2^24; at most 2^30) -- no result depends on it; it
 * exists so that tests cross chunk borders on small inputs. */
int gdiet_hip_pile_finish(gdiet_pileup *pile, gdiet_pile_summary_t *summary_out);
int gdiet_hip_pile_finish_chunked(gdiet_pileup *pile, uint64_t chunk, gdiet_pile_summary_t *summary_out);
/* After finish: out[0, 8 * (end - beg)) takes the counters of positions [beg, end) of contig rid, which must lie inside one region. */
int gdiet_hip_pile_counts(gdiet_pileup *pile, uint32_t rid, uint32_t beg, uint32_t end, uint32_t *out);
/* After finish: out takes one consensus byte per position of region `region` (its number in the list; a contig's with an empty list). */
int gdiet_hip_pile_consensus(gdiet_pileup *pile, size_t region, uint32_t min_depth, uint8_t *out);
/* After finish: the sites.  Returns their number; with out == NULL that is all (the size first), else cap, the room of out in rows,
 * must hold them (GDIET_E_PARAM otherwise, the text says how many there are). */
int64_t gdiet_hip_pile_sites(gdiet_pileup *pile, uint32_t min_depth, uint32_t min_alt, uint32_t num, uint32_t den, gdiet_pile_site_t *out, size_t cap);
/* Frees the counters and the handle, whatever state it is in. */
int gdiet_hip_pile_close(gdiet_pileup *pile);

/* ---- Alignment statistics ---------------------------------------------------------------------------------------------------------------
 * What `samtools flagstat` and `samtools stats` report after a run, accumulated on the device from uncompressed BAM alignment records
 * while they are resident there: a summary and eleven histograms.  The reference prints SAM and stops: these rules are the definition
 * (tests/stats_ref.py restates them).  Every counter is an unsigned 64-bit integer and every add is an integer add, so every result is a
 * function of the multiset of input records and the options alone: it does not depend on how the records were cut into calls, on the
 * route or on the order of atomic arrivals.  The tables of disjoint sets of records simply add.
 * Options: excl_flags (usual value 0x700: secondary, QC-fail, duplicate), min_mapq (0), cycles (512; 1 .. 1024), max_len (65536;
 * 1 .. 2^20), max_indel (64; 1 .. 4096).  A value out of range is GDIET_E_PARAM with a message.
 *   VALIDATION  the real CIGAR, the bad-record reasons, the poisoning and the naming of the call's first bad record are those of
 *           "Coverage".  A bad record adds to `records`, to `bad` and to the flag counters of coverage's summary, and to nothing else.
 *   TWO POPULATIONS  with f the flag of a good record:
 *           it is a READ if (f & (excl_flags | 0x900)) == 0: unmapped reads are reads, MAPQ is not looked at;
 *           it is an ALIGNMENT if coverage's `counted` holds with the flags excl_flags | 0x4: not excluded, mapq >= min_mapq, refID >= 0.
 *           A supplementary record is an alignment but not a read.  A record may be both, or neither.
 *   BASE CODE  of a SEQ nibble: 1 2 4 8 give A C G T (0 .. 3); every other nibble, '=' included, gives 4 ("other").
 *   CYCLE   of query index qi, in the read's original orientation: lead + qi on the forward strand, trail + (l_seq - 1 - qi) on the
 *           reverse strand (f & 0x10), where lead / trail is the length of a hard clip (operation code 5) that is the first / the last
 *           operation of the real CIGAR, else 0.  A per-cycle table has cycles + 1 rows; row `cycles` takes every cycle >= cycles.
 *   OVER READS
 *           read_len[min(l_seq, max_len)]                      max_len + 1 bins
 *           gc[101]            if l_seq > 0: with a the number of A C G T bases and g the number of C G bases, if a > 0 the bin
 *                              (200 g + a) / (2 a) in integer division (100 g / a rounded, halves up)
 *           base_cycle[cycles + 1][5]   every base by its cycle and its code; on a reverse read the code is complemented (A <-> T,
 *                              C <-> G, other stays other)
 *           with qualities present (l_seq > 0 and the first QUAL byte is not 0xff):
 *           qual_cycle[cycles + 1][2]   per cycle the number of quality bytes and their sum
 *           base_qual[96]      every quality byte q at min(q, 95)
 *   OVER ALIGNMENTS  walking the real CIGAR as "Coverage" does, reference cursor from pos, query cursor from 0:
 *           mapq[256]
 *           ins_len[max_indel + 1]   every I run of length L > 0 at min(L, max_indel);  del_len likewise for D runs.  N is no deletion.
 *           soft- and hard-clipped bases (codes 4 and 5) go into the summary.
 *           for every base of an M = X run, if l_seq > 0, with rc the code of the base as stored and fc the code of the reference base
 *           of its position in the index's packed reference (0 .. 3, 4 for N):
 *             subst[5][5]      cell [fc][rc]: reference orientation
 *             the base is COMPARABLE if rc < 4 and fc < 4, a MATCH if comparable and rc == fc, a MISMATCH if comparable and rc != fc
 *             cmp_cycle[cycles + 1][2]   per cycle of the base the comparable bases and the mismatches
 *           per alignment, with m matches, x mismatches, i and d the numbers of I and D runs of length above 0 and den = m + x + i + d:
 *             identity[101]    if den > 0 the bin 100 m / den (64-bit integer division); else no_identity += 1
 *           an alignment with l_seq == 0 adds to mapq, the indel tables, the clips, no_seq and no_identity.
 *   SUMMARY coverage's ten counters under the flags excl_flags | 0x4 (so `counted` is the number of alignments, and an unmapped record
 *           is excluded_by_flag); duplicate and qcfail (flag bits 0x400 and 0x200, over good records); reads, read_bases (l_seq over
 *           reads); aligned_bases (the bases that entered subst), matches, mismatches, other_bases (not comparable); ins_events,
 *           ins_bases, del_events, del_bases (runs of length above 0); soft_clipped, hard_clipped; no_seq, no_identity.
 *   DUPLICATES  an accumulator attached to a sorter with duplicate marking scatters when the batch is added, before any record carries
 *           0x400: marked duplicates are counted like any other record.  To leave them out feed the finished file's records through
 *           gdiet_hip_stats_add_bam.
 * The device side (csrc/stats.hip.h, statements in csrc/stats.h, which reuses those of csrc/cov.h and csrc/pile.h):
 * stats_scatter_kernel, one wavefront per record, four records to a block.  Every table but read_len is kept per block in local memory
 * as uint32 (about 21 KB with the default options), added to with local-memory atomics and flushed once per block with 64-bit global
 * atomics; adds that many lanes would make to one cell are reduced across the wavefront first; a block flushes before a cell could
 * pass 2^32.  The whole state is n_all * 8 bytes, 43 KB plus 8 bytes per read-length bin.  finish runs no kernel.  Out of scope:
 * insert sizes and other paired-end statistics, per-contig breakdowns, coverage distribution and GC-depth (derivable from "Coverage"),
 * indels per cycle, mismatch counts from NM / MD, merging the tables of several GPUs (add them), plots. */
typedef struct gdiet_stats gdiet_stats;
typedef struct {
	uint64_t records, unmapped, secondary, supplementary, primary_mapped, reverse, excluded_by_flag, excluded_by_mapq, counted, bad;
	uint64_t duplicate, qcfail, reads, read_bases, aligned_bases, matches, mismatches, other_bases;
	uint64_t ins_events, ins_bases, del_events, del_bases, soft_clipped, hard_clipped, no_seq, no_identity;
} gdiet_stats_summary_t;
/* the tables gdiet_hip_stats_table reads, with their sizes in counters */
enum {
	GDIET_STATS_GC = 0,     /* 101 */
	GDIET_STATS_BASE_CYCLE, /* (cycles + 1) * 5, row-major */
	GDIET_STATS_QUAL_CYCLE, /* (cycles + 1) * 2: count, sum */
	GDIET_STATS_BASE_QUAL,  /* 96 */
	GDIET_STATS_MAPQ,       /* 256 */
	GDIET_STATS_INS_LEN,    /* max_indel + 1 */
	GDIET_STATS_DEL_LEN,    /* max_indel + 1 */
	GDIET_STATS_SUBST,      /* 25: [reference code][read code] */
	GDIET_STATS_CMP_CYCLE,  /* (cycles + 1) * 2: comparable, mismatches */
	GDIET_STATS_IDENTITY,   /* 101 */
	GDIET_STATS_READ_LEN    /* max_len + 1 */
};
/* An accumulator over idx's contigs: allocates and clears the tables.  idx must stay alive for as long as the handle takes records: the
 * kernel reads its packed reference.  The tables also go when the context is destroyed: a handle that outlives its context takes
 * nothing but close.  _bounded: the weight, in bases, a block may hold in local memory between two flushes (0: the default, 2^24, which
 * is also the most) -- no result depends on it; it exists so that tests reach the flush and the path of a record too heavy for local
 * memory on small inputs. */
int gdiet_hip_stats_open(gdiet_ctx *ctx, const gdiet_index *idx, uint32_t excl_flags, uint32_t min_mapq, uint32_t cycles, uint32_t max_len, uint32_t max_indel, gdiet_stats **out);
int gdiet_hip_stats_open_bounded(gdiet_ctx *ctx, const gdiet_index *idx, uint32_t excl_flags, uint32_t min_mapq, uint32_t cycles, uint32_t max_len, uint32_t max_indel, uint64_t bound,
                                 gdiet_stats **out);
/* Host records and a mapped batch: as gdiet_hip_cov_add_bam and gdiet_hip_cov_add (opt_flag decides which records exist). */
int gdiet_hip_stats_add_bam(gdiet_stats *stats, const void *recs, size_t len);
int gdiet_hip_stats_add(gdiet_stats *stats, const gdiet_index *idx, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                        const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag);
/* Attach (NULL: detach) to a BGZF writer with a context or to a sorter, beside the coverage and the pileup accumulator and under their
 * rules; all three may be attached at once, and one table of record starts serves them.  The bytes written do not change.  Lock order:
 * the encoder's mutex, the coverage accumulator's, the pileup accumulator's, the statistics accumulator's, the context's lane. */
int gdiet_hip_bgzf_out_set_stats(gdiet_bgzf_out *writer, gdiet_stats *stats);
int gdiet_hip_bam_sort_set_stats(gdiet_bam_sorter *sorter, gdiet_stats *stats);
/* The tables come down (no kernel runs) and *summary_out (may be NULL) is filled.  After it the accumulator is read-only: add is
 * refused, finish again returns the same figures. */
int gdiet_hip_stats_finish(gdiet_stats *stats, gdiet_stats_summary_t *summary_out);
/* After finish: table `which` (GDIET_STATS_*).  Returns its size in counters; with out == NULL that is all, else cap, the room of out in
 * counters, must hold them (GDIET_E_PARAM otherwise). */
int64_t gdiet_hip_stats_table(gdiet_stats *stats, int which, uint64_t *out, size_t cap);
/* Frees the tables and the handle, whatever state it is in. */
int gdiet_hip_stats_close(gdiet_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
