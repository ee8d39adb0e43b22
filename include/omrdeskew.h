/*
 * omrdeskew.h -- C ABI of libomrdeskew.so, the MI355X-native OMR deskew engine.
 *
 * This is the drop-in boundary for the projection-std-dev angle sweep of
 * ch1ny/omr-img-corrector (crate `oics`, packages/lib).  The reference has no FFI layer of its
 * own (it calls OpenCV through the `opencv` crate); a Rust shim crate `oics` binds these entry
 * points 1:1 in an `extern "C"` block (INTEGRATION.md shows it).  Every entry point cites the
 * reference interface it replaces as file:line under /root/reference.
 *
 * Conventions
 *   - images are 8-bit, row-major, `channels` interleaved, `step_bytes >= cols*channels`;
 *     inputs are borrowed and never written; outputs are caller-allocated unless stated.
 *   - return value: 0 on success, otherwise a negative OpenCV-style code
 *     (-215 assertion / bad shape, -5 bad argument, -4 out of memory, -213 not implemented,
 *      -217 GPU API error).  omr_last_error() gives the thread-local message.
 *   - no exceptions and no aborts cross the ABI; all entry points are thread-safe and
 *     re-entrant (the Tauri host runs several corrections at once: thread_pool.rs:41-88).
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point
 *     fails with -217.
 *   - `_device` entry points take device pointers (hipMalloc'ed, same device as the plan) and a
 *     hipStream_t passed as void*; they enqueue work and return without synchronising.
 */
#ifndef OMRDESKEW_H
#define OMRDESKEW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMR_OK 0
#define OMR_ERR_ASSERT (-215)
#define OMR_ERR_BADARG (-5)
#define OMR_ERR_NOMEM (-4)
#define OMR_ERR_NOTIMPL (-213)
#define OMR_ERR_GPU (-217)

/* Borrowed image view: stands for `&opencv::core::Mat` / `&TransformableMatrix`
 * (packages/lib/src/transfer.rs:16-18). */
typedef struct {
    const uint8_t *data;
    int32_t rows, cols, channels;
    int64_t step_bytes;
} omr_image;

/* Owned image returned by the library (free with omr_image_free): stands for the fresh
 * `TransformableMatrix` every reference helper returns (transfer.rs:55-59). */
typedef struct {
    uint8_t *data;
    int32_t rows, cols, channels;
    int64_t step_bytes;
} omr_image_owned;

/* types.rs:7-11 RotateClipStrategy */
#define OMR_CLIP_DEFAULT 0
#define OMR_CLIP_CONTAIN 1
/* omr.rs:41-45 ResultStatus */
#define OMR_STATUS_BELIEVED 0
#define OMR_STATUS_NEED_CHECK 1
#define OMR_STATUS_NOT_A_RESULT 2
/* interpolation flags as the reference passes them (0 = INTER_NEAREST = WARP_POLAR_LINEAR's
 * numeric value, transfer.rs / projection.rs:52; 1 = INTER_LINEAR, core/src/main.rs:76) */
#define OMR_INTER_NEAREST 0
#define OMR_INTER_LINEAR 1
#define OMR_INTER_AREA 3 /* imgproc::INTER_AREA: resize only */
/* warpAffine flags and border modes (OpenCV 4.6.0 numbering) for omr_rotate_ex / omr_rotate_device_ex */
#define OMR_INTER_CUBIC 2
#define OMR_INTER_LANCZOS4 4
#define OMR_WARP_FILL_OUTLIERS 8
#define OMR_WARP_INVERSE_MAP 16
#define OMR_BORDER_CONSTANT 0
#define OMR_BORDER_REPLICATE 1
#define OMR_BORDER_REFLECT 2
#define OMR_BORDER_WRAP 3
#define OMR_BORDER_REFLECT_101 4
#define OMR_BORDER_TRANSPARENT 5
/* erode / dilate (OpenCV 4.6.0 MorphShapes numbering) for omr_structuring_element / omr_morph* */
#define OMR_MORPH_RECT 0
#define OMR_MORPH_CROSS 1
#define OMR_MORPH_ELLIPSE 2
#define OMR_MORPH_ERODE 0
#define OMR_MORPH_DILATE 1

int omr_version(void);
int omr_device_count(void);
const char *omr_last_error(void);
void omr_image_free(omr_image_owned *img);

/* ---- geometry helpers ---------------------------------------------------------------- */

/* imgproc::get_rotation_matrix_2d(center: Point2f, angle, scale) -> 2x3 f64;
 * call sites transfer.rs:475,501; omr.rs:159-163,425-426. */
int omr_get_rotation_matrix_2d(float cx, float cy, double angle_deg, double scale, double M[6]);

/* `(max_angle as f64 / step) as u16` and the half-open candidate range -N..N
 * (projection.rs:36-38, omr.rs:140-145).  Returns A = 2N (>= 0); *N_out = N. */
int omr_candidate_count(uint16_t max_angle, double step, int32_t *N_out);

/* The A forward matrices of a sweep over an image of rows x cols: centre
 * (cols as f32 / 2, rows as f32 / 2), angle (i - N) * step, scale (transfer.rs:473-475;
 * omr.rs:157-163 passes scale = projection_resize_scale).  M_out: A x 6 doubles. */
int omr_sweep_matrices(int32_t rows, int32_t cols, uint16_t max_angle, double step, double scale,
                       double *M_out, int32_t cap_A);

/* ---- the hot path ---------------------------------------------------------------------- */

/* One scan, A candidate matrices, host buffers.  For every candidate: nearest-neighbour
 * warpAffine of the binarised image onto the same canvas with a white border, per-column and
 * per-row count of pixels == 0, population std-dev of each projection.
 * Replaces the body of projection.rs:47-65 / omr.rs:153-180:
 *   rotate_mat DEFAULT (transfer.rs:459-486) -> get_projection_standard_deviations
 *   (transfer.rs:527-536) or get_mat_projection_data (omr.rs:8-39) + calculate.rs:13-23.
 * bin_u8c1: 1 channel; a pixel is black iff its value == 0.
 * fwd_M: A x 6 row-major forward matrices as produced by getRotationMatrix2D.
 * vproj (A x cols) and hproj (A x rows) may be NULL; v_sd / h_sd: A doubles each. */
int omr_projection_sweep(const omr_image *bin_u8c1, const double *fwd_M, int32_t A,
                         uint32_t *vproj, uint32_t *hproj, double *v_sd, double *h_sd);

/* Resident form of the same path: device buffers and fixed-point tables are created once per
 * (rows, cols, matrices) and reused for every scan of that shape. */
typedef struct omr_sweep_plan omr_sweep_plan;

int omr_sweep_plan_create(int32_t rows, int32_t cols, const double *fwd_M, int32_t A,
                          int32_t device, omr_sweep_plan **plan_out);
int omr_sweep_plan_create_angles(int32_t rows, int32_t cols, uint16_t max_angle, double step,
                                 double scale, int32_t device, omr_sweep_plan **plan_out);
void omr_sweep_plan_destroy(omr_sweep_plan *plan);
int omr_sweep_plan_candidates(const omr_sweep_plan *plan); /* A */

/* Enqueue one scan on `stream`.  d_img: device u8, 1 channel, rows x cols, row pitch
 * step_bytes.  A pixel is black iff value <= black_max: pass 0 for an image binarised by
 * transfer_gray_image_to_thresh_binary (transfer.rs:294-301), 127 to fuse that threshold
 * (threshold(127,255,BINARY) then == 0  <=>  gray <= 127) into the load.
 * Outputs are device pointers; any of d_vproj (A x cols u32), d_hproj (A x rows u32),
 * d_best_idx (1 int32: projection.rs:125-190 arg-max, lowest index on exact ties) may be NULL.
 * d_v_sd / d_h_sd: A doubles each. */
int omr_sweep_plan_run_device(omr_sweep_plan *plan, const uint8_t *d_img, int64_t step_bytes,
                              int32_t black_max, void *stream, uint32_t *d_vproj,
                              uint32_t *d_hproj, double *d_v_sd, double *d_h_sd,
                              int32_t *d_best_idx);

/* Same, host image in / host results out (synchronous: H2D, sweep, D2H on `plan`'s stream). */
int omr_sweep_plan_run(omr_sweep_plan *plan, const omr_image *img_u8c1, int32_t black_max,
                       uint32_t *vproj, uint32_t *hproj, double *v_sd, double *h_sd,
                       int32_t *best_idx);

/* Duration in ms of the sweep kernel of the most recent omr_sweep_plan_run*(), measured with
 * HIP events on the stream it was launched on (bench.py's roofline line). Synchronises. */
int omr_sweep_plan_last_kernel_ms(omr_sweep_plan *plan, float *ms_out);
/* Toggle event recording around the sweep kernel (off by default). */
int omr_sweep_plan_set_timing(omr_sweep_plan *plan, int32_t enabled);
/* Select the sweep kernel: 0 = automatic (run-merging kernel for every candidate that qualifies,
 * LDS-staged or generic gather kernel for the rest), 1 = generic gather kernel for all, 2 = LDS-staged
 * gather kernel for all (fails with -5 when a candidate's source footprint does not fit), 3 = as 0 but
 * fails with -5 when no candidate qualifies for the run-merging kernel.  For tests and profiling. */
int omr_sweep_plan_set_kernel(omr_sweep_plan *plan, int32_t which);
/* How the plan splits its candidates: *n_runs are swept by the run-merging kernel (small-angle
 * rotations), *n_gather by the per-sample gather kernels.  Either pointer may be NULL. */
int omr_sweep_plan_info(const omr_sweep_plan *plan, int32_t *n_runs, int32_t *n_gather);
/* Debug/parity hook: copy the fixed-point tables of candidate `a` to host
 * (adelta, bdelta: cols ints; X0, Y0: rows ints) -- OpenCV hal::warpAffine's tables. */
int omr_sweep_plan_tables(omr_sweep_plan *plan, int32_t a, int32_t *adelta, int32_t *bdelta,
                          int32_t *X0, int32_t *Y0);

/* Batch of n scans (all rows x cols, 1 channel) resident on the plan's device, scan i at
 * d_scans + i * scan_stride_bytes.  Scans are independent (one correct_default per file,
 * app/src-tauri/src/task.rs:19-38): they are issued round-robin on `n_streams` internal
 * streams; no collective is involved.  Outputs are device pointers: d_best_idx (n int32),
 * d_v_sd / d_h_sd (n x A doubles, may be NULL).  Returns after enqueueing; call
 * omr_batch_sync() or synchronise the device before reading. */
typedef struct omr_batch_ctx omr_batch_ctx;
int omr_batch_create(int32_t rows, int32_t cols, uint16_t max_angle, double step, double scale,
                     int32_t device, int32_t n_streams, omr_batch_ctx **ctx_out);
void omr_batch_destroy(omr_batch_ctx *ctx);
int omr_batch_run_device(omr_batch_ctx *ctx, const uint8_t *d_scans, int64_t scan_stride_bytes,
                         int64_t step_bytes, int32_t n, int32_t black_max, int32_t *d_best_idx,
                         double *d_v_sd, double *d_h_sd);
int omr_batch_sync(omr_batch_ctx *ctx);
/* Scans carried by one launch of each kernel (default 1; 1..64).  Larger groups amortise the fixed
 * cost between dependent launches (about 30 us per sweep at 2480x3508) over more work; the scratch
 * grows accordingly (about 40 MB per scan of the group at 2480x3508).  Results do not change.
 * Prefer 1, 2, 4, 8 or a multiple of 8: the sweep's grid runs scans fastest and workgroups go
 * round-robin to the 8 XCDs, so each XCD then sees one scan (or two) and keeps its bit image in L2. */
int omr_batch_set_group(omr_batch_ctx *ctx, int32_t scans_per_launch);
/* Split of the candidates between the run-merging kernel and the gather kernels (see
 * omr_sweep_plan_info). */
int omr_batch_info(const omr_batch_ctx *ctx, int32_t *n_runs, int32_t *n_gather);
/* Sum over launch groups of the sweep-stage duration (ms; HIP events on the launch stream around
 * the sweep kernels of a group: one run-merging launch -- all scans of the group, both projections
 * -- plus one gather launch per scan when some candidates do not qualify) and the number of groups
 * timed since the last call (timing must be enabled with omr_batch_set_timing).  Synchronises. */
int omr_batch_set_timing(omr_batch_ctx *ctx, int32_t enabled);
int omr_batch_kernel_ms(omr_batch_ctx *ctx, double *sum_ms, int32_t *launches);
/* The reference's whole unit of work for a batch (omr.rs:339-452 correct_default; core/src/main.rs:69-92): detect
 * every scan's angle, then rotate the scan by it with CONTAIN geometry (transfer.rs:487-519), border_value
 * outside.  Sweep, arg-max and warp stay on the device: the warp reads the winning candidate's index there, and
 * its fixed-point tables exist per candidate (matrices from the host's libm, like omr_rotate*).  interp is
 * OMR_INTER_NEAREST (omr.rs:408-445) or OMR_INTER_LINEAR (core/src/main.rs:72-81).  Scan i's canvas fills the
 * top-left dst_rows x dst_cols pixels of d_out + i * out_stride_bytes (rows out_step_bytes apart) and its size
 * lands in d_out_size[2 i] (rows) and [2 i + 1] (cols); every slot must hold the largest canvas of the candidate
 * set, omr_batch_deskew_canvas().  The result is what omr_rotate_device(angle = (best_idx - N) * step, scale 1,
 * OMR_CLIP_CONTAIN) writes for the same scan, bit for bit.  d_best_idx (n int32) and d_out_size (2 n int32) may be
 * NULL.  Returns after enqueueing, like omr_batch_run_device.
 * Performance note: the warp stages every tile's source box in LDS with dword loads, which needs d_scans,
 * scan_stride_bytes, step_bytes and the scan width to be multiples of 4; otherwise (e.g. a 453-column scan, tightly
 * packed) every tile takes a byte-wise per-tap path straight from memory -- same result, several times slower. */
int omr_batch_deskew_canvas(omr_batch_ctx *ctx, int32_t *max_rows, int32_t *max_cols);
int omr_batch_deskew_device(omr_batch_ctx *ctx, const uint8_t *d_scans, int64_t scan_stride_bytes,
                            int64_t step_bytes, int32_t n, int32_t black_max, int32_t interp,
                            uint8_t border_value, uint8_t *d_out, int64_t out_stride_bytes,
                            int64_t out_step_bytes, int32_t *d_out_size, int32_t *d_best_idx);
/* omr_batch_run_device / omr_batch_deskew_device for scans of `channels` interleaved 8-bit channels.
 * channels = 3: BGR as imread(IMREAD_COLOR) gives it; gray = cvtColor(COLOR_RGB2GRAY) fused into the load
 * (projection.rs:29-32, quirk B8); a pixel is black iff gray <= black_max.  channels = 1: identical to the
 * 1-channel entry points.  Other counts: OMR_ERR_NOTIMPL.  black_max outside 0..255: OMR_ERR_BADARG.
 * Deskew: border_value[0..channels-1] per channel; every output slot holds the largest canvas,
 * out_step_bytes >= channels * max_cols of omr_batch_deskew_canvas().
 * Every argument is checked before any device work (step_bytes >= channels * cols included); no gray image is
 * written.  Scan i's colour canvas is what omr_rotate_device(channels = 3, angle = (best_idx - N) * step, scale 1,
 * OMR_CLIP_CONTAIN) writes for the same scan, bit for bit; the winners and scores are what the 1-channel entry
 * points give for omr_rgb_to_gray_device of the scans.  As with omr_batch_deskew_device, the warp stages source
 * boxes in LDS only when d_scans, scan_stride_bytes and step_bytes are multiples of 4. */
int omr_batch_run_device_cn(omr_batch_ctx *ctx, const uint8_t *d_scans, int64_t scan_stride_bytes,
                            int64_t step_bytes, int32_t channels, int32_t n, int32_t black_max,
                            int32_t *d_best_idx, double *d_v_sd, double *d_h_sd);
int omr_batch_deskew_device_cn(omr_batch_ctx *ctx, const uint8_t *d_scans, int64_t scan_stride_bytes,
                               int64_t step_bytes, int32_t channels, int32_t n, int32_t black_max,
                               int32_t interp, const uint8_t border_value[4], uint8_t *d_out,
                               int64_t out_stride_bytes, int64_t out_step_bytes, int32_t *d_out_size,
                               int32_t *d_best_idx);
/* Streams and pinned staging blocks the per-call entry points lease from a bounded per-device pool (a host
 * that runs every task on a fresh OS thread, thread_pool.rs:41-88, must not leak one of each per call):
 * slots that exist, slots idle in the pool, pinned bytes held by idle slots.  Pointers may be NULL. */
int omr_call_pool_stats(int32_t device, int32_t *live_slots, int32_t *idle_slots, int64_t *idle_pinned_bytes);

/* ---- scan-lane sweep (batches) ------------------------------------ */
/* The batch path sweeps 64 scans per wavefront (lane = scan): the geometry of a candidate -- which source row,
 * word column, shift and destination bits make up every destination word (projection.rs:47-65 ->
 * transfer.rs:459-486) -- is one wave-uniform PROGRAM per (candidate, strip of two word columns), enumerated
 * from warpAffine's integer tables.  This entry point builds one strip's program on the HOST (no GPU needed):
 * n_records rows (pre_rows virtual ones first) of seg_dwords_per_row dwords in the segment stream and of 4 dwords
 * in the fetch stream (layout: csrc/slane.hpp); guard_cols / guard_rows = the zero guard (word columns, rows) the
 * program's entry numbers assume around the interleaved bit image.  NULL output pointers query the sizes.
 * OMR_ERR_NOTIMPL when the strip does not fit the scheme (such candidates stay with the run-merging kernel). */
int omr_slane_strip_program(int32_t rows, int32_t cols, const double *fwd_M, int32_t strip, uint32_t *seg_out,
                            uint32_t *fetch_out, int32_t *seg_dwords_per_row, int32_t *n_records, int32_t *pre_rows,
                            int32_t *most_segments, int32_t *guard_cols, int32_t *guard_rows);

/* Switch a batch context to the scan-lane sweep: every launch then carries up to max_scans_per_launch scans (whole
 * groups of 64, at most 4096), 64 scans per wavefront; results are bit-identical to the run-merging path.  The
 * programs of all (candidate, strip) pairs are generated on the device, once (about 45 ms and 4.7 GB of HBM for
 * 2480x3508 with 400 candidates).  A launch of up to 64 / 128 / 256 scans takes about 5.9 / 10.4 / 19 ms at that size:
 * size launches in multiples of 64.  0 switches back.  OMR_ERR_NOTIMPL, context unchanged, when a candidate does not
 * fit the scheme (beyond about +-10 degrees at unit scale, or more than 8166 rows). */
int omr_batch_set_lanes(omr_batch_ctx *ctx, int32_t max_scans_per_launch);
/* Bytes of programs the context's scan-lane plan holds in HBM, its (candidate, strip) tasks, scans per launch
 * (0 = the context is on the run-merging path).  Pointers may be NULL. */
int omr_batch_lanes_info(omr_batch_ctx *ctx, int64_t *program_bytes, int32_t *tasks, int32_t *scans_per_launch);
/* Inspection: with on != 0 a launch leaves its row counts in the scratch set (needed by
 * omr_batch_lanes_projections); by default they are cleared behind the std-dev kernel, off the sweep's stream. */
int omr_batch_lanes_keep(omr_batch_ctx *ctx, int32_t on);
/* The scan-lane programs of a context are generated on the device; this regenerates them with the host generator (the
 * reference implementation behind omr_slane_strip_program) and compares: *dwords = dwords of programs, *differing = how
 * many differ (0 = identical).  For tests and inspection; seconds at A4. */
int omr_batch_lanes_check_programs(omr_batch_ctx *ctx, int64_t *dwords, int64_t *differing);

/* The integer projections one scan / candidate of the last scan-lane launch left in scratch set `set` (0 for the
 * first launch of a stream): vproj = cols counts, hproj = rows counts; either may be NULL.  Synchronises. */
int omr_batch_lanes_projections(omr_batch_ctx *ctx, int32_t set, int32_t scan, int32_t a, uint32_t *vproj,
                                uint32_t *hproj);

/* ---- batches that start in host memory ("wall-clock including H2D"; core/src/main.rs:68-95) --- */
/* A context for repeated host-memory batches of one shape and sweep: per device the sweep plan (the scan-lane sweep when
 * the candidates fit it and at least 64 scans per device are expected, else the run-merging path), a pinned ring of three
 * 16-scan slots and two device stages of one launch (64 scans) each.  n_devices <= 0 = every visible device,
 * n_devices > omr_device_count() is OMR_ERR_BADARG.  max_scans = the largest n a run may carry. */
typedef struct omr_host_batch omr_host_batch;
int omr_host_batch_create(int32_t rows, int32_t cols, uint16_t max_angle, double step, int32_t n_devices,
                          int32_t max_scans, omr_host_batch **out);
void omr_host_batch_destroy(omr_host_batch *hb);
int omr_host_batch_info(const omr_host_batch *hb, int32_t *n_devices, int32_t *scans_per_launch, int32_t *scan_lane);
/* scans[i] -> device i % n_devices: host memory -> device stage -> sweep; the transfer of one launch overlaps the sweep of
 * the previous one.  Pixels == 0 are black (binarised scans, as omr_sweep_batch).  transfer_mode:
 *   OMR_HOST_PAGEABLE  the context's copier threads move the scans into its pinned ring, DMA from there;
 *   OMR_HOST_PINNED    the caller's memory is page-locked: DMA straight out of it;
 *   OMR_HOST_PACKED    the copier threads -- which touch every byte anyway -- turn each binarised scan into 1 bit per pixel
 *                      on its way into the ring: 1/8 of the bytes cross the link (1.09 MB per A4 scan), a device kernel
 *                      interleaves the packed rows into the scan-lane image.  Contexts on the run-merging path (fewer than
 *                      64 scans per device) transfer the bytes as they are.
 * The three give the same results, bit for bit.  Outputs as omr_sweep_batch. */
#define OMR_HOST_PAGEABLE 0
#define OMR_HOST_PINNED 1
#define OMR_HOST_PACKED 2
int omr_host_batch_run(omr_host_batch *hb, const omr_image *scans, int32_t n, int32_t transfer_mode,
                       int32_t *best_idx, double *best_angle, double *v_sd_opt, double *h_sd_opt);
/* Scans per sweep launch (scan-lane contexts: rounded up to a multiple of 64, at most 512; default 64, which suits the
 * copy-bound u8 modes -- the last launch's sweep is what nothing overlaps; packed transfers are sweep-bound and larger
 * launches sweep faster per scan).  Re-sizes the device stages and the sweep's scratch. */
int omr_host_batch_set_launch(omr_host_batch *hb, int32_t scans_per_launch);

/* Host-buffer batch over the visible devices (SURVEY.md 8b `omr_sweep_batch`): scans[i] goes
 * to device i % n_devices (an omr_host_batch made for this one call: plan and ring creation are inside the call; packed transfers).
 * The scans may have DIFFERENT shapes (the reference corrects one file per call, any size, task.rs:19-38): they are bucketed by
 * (rows, cols), one context per shape, and the results land at the scans' own positions;
 * the only "collective" is the host-side gather of the results.  n_devices <= 0 = every visible device;
 * n_devices > omr_device_count() is OMR_ERR_BADARG (never a silent clamp).
 * best_angle[i] = (best_idx[i] - N) * step (projection.rs:189-190). */
int omr_sweep_batch(const omr_image *scans, int32_t n, uint16_t max_angle, double step,
                    int32_t n_devices, int32_t *best_idx, double *best_angle, double *v_sd_opt,
                    double *h_sd_opt);

/* ---- drivers with the reference's signatures ------------------------------------------ */

/* oics::projection::get_angle_with_projections(&TransformableMatrix, u16, f64, f64, usize) -> f64
 * (projection.rs:17-23).  src: 3 or 4 channels as the reference requires (cvtColor RGB2GRAY);
 * 1 channel is accepted and skips the conversion.  threads_hint is ignored (the reference's
 * multi-thread branch is buggy, projection.rs:94, and no caller uses it). */
int omr_get_angle_with_projections(const omr_image *src, uint16_t max_angle, double step,
                                   double resize_scale, size_t threads_hint, double *angle_out);

/* find_target_angle(max_angle, step, thresh, threads) -> f64 on an already binarised image
 * (app/src-tauri/src/test.rs:83-178, the in-app copy of the same driver). */
int omr_find_target_angle(uint16_t max_angle, double step, const omr_image *thresh_u8c1,
                          size_t threads_hint, double *angle_out);

/* oics::omr::get_result_from_projection(&Mat, u16, f64, i32, i32) -> Result<OmrResult>
 * (omr.rs:52-229).  candidates receives min(cand_len, cand_cap) angles. */
int omr_get_result_from_projection(const omr_image *src, uint16_t max_angle, double step,
                                   int32_t max_w, int32_t max_h, double *angle, int32_t *status,
                                   double *candidates, int32_t cand_cap, int32_t *cand_len);

/* projection.rs:125-190 on host arrays (also used by the drivers above). */
int omr_argmax_projection(const double *v_sd, const double *h_sd, int32_t n, int32_t *index_out);
/* Same policy for scores that live on the device (enqueue only; d_index_out: 1 int32). */
int omr_argmax_projection_device(const double *d_v_sd, const double *d_h_sd, int32_t n,
                                 int32_t *d_index_out, void *stream);
/* omr.rs:147-221 on host arrays. */
int omr_select_projection_result(const double *v_sd, const double *h_sd, int32_t n, int32_t N,
                                 double step, double *angle, int32_t *status, double *candidates,
                                 int32_t cand_cap, int32_t *cand_len);

/* ---- per-image helpers of crate `oics` (GPU-backed) ------------------------------------- */

/* transfer::transfer_gray_image_to_thresh_binary (transfer.rs:294-301): dst = src>127 ? 255 : 0 */
int omr_threshold_binary(const omr_image *gray_u8c1, uint8_t *dst, int64_t dst_step_bytes);
/* transfer::transfer_rgb_image_to_gray_image (transfer.rs:283-290): cvtColor RGB2GRAY on 3/4 ch */
int omr_rgb_to_gray(const omr_image *src, uint8_t *dst, int64_t dst_step_bytes);
/* transfer::rotate_mat (transfer.rs:459-523); border_value = Scalar(b, g, r, a) as u8. */
int omr_rotate(const omr_image *src, double angle_deg, double scale, int32_t interp,
               const uint8_t border_value[4], int32_t clip, omr_image_owned *dst);
/* transfer::get_vertical_projection / get_horizontal_projection (transfer.rs:380-405, :305-333) */
int omr_get_vertical_projection(const omr_image *bin_u8c1, double *out_cols);
int omr_get_horizontal_projection(const omr_image *bin_u8c1, double *out_rows);
/* omr::get_mat_projection_data (omr.rs:8-39): (horizontal[rows], vertical[cols]) */
int omr_get_mat_projection_data(const omr_image *bin_u8c1, double *h_rows, double *v_cols);
/* transfer::get_projection_standard_deviations (transfer.rs:527-536): (vertical, horizontal) */
int omr_get_projection_standard_deviations(const omr_image *bin_u8c1, double *v_sd, double *h_sd);
/* TransformableMatrix::scale_self (transfer.rs:66-91): new size = ((w * scale) as i32, (h * scale) as i32),
 * INTER_LINEAR when scale > 1, INTER_AREA otherwise; scale == 1.0 returns a copy.
 * shrink_to (transfer.rs:93-126; the Projection phase of the in-app benchmark, app/src-tauri/src/test.rs:313):
 * scale = min(max_width / w, max_height / h) (a bound <= 0 means "no bound"), applied only when < 1.
 * resize_self (transfer.rs:128-145): resize to (width, height) with INTER_AREA.
 * The reference mutates `self`; here the result is a new owned image (omr_image_free). */
int omr_scale(const omr_image *src, double scale, omr_image_owned *dst);
int omr_shrink_to(const omr_image *src, int32_t max_width, int32_t max_height, omr_image_owned *dst);
int omr_resize(const omr_image *src, int32_t width, int32_t height, omr_image_owned *dst);

/* ---- the same stages on device-resident images (enqueue on `stream`, no synchronisation) ----
 * These are the building blocks of a fully resident pipeline: front end of omr.rs:87-139,
 * sweep (omr_sweep_plan_run_device / omr_batch_run_device), final deskew of omr.rs:408-445 /
 * transfer.rs:487-519.  All pointers are device pointers; steps are row pitches in bytes. */
int omr_rgb_to_gray_device(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols,
                           int32_t channels, uint8_t *d_dst, int64_t dst_step, void *stream);
/* transfer_rgb_image_to_gray_image for a batch: n device-resident scans of one shape, 3 or 4 channels, scan i at d_src +
 * i * src_stride_bytes (rows src_step apart), its gray image at d_dst + i * dst_stride_bytes (rows dst_step apart), in one
 * launch (one per 65535 scans).  Every output byte is what omr_rgb_to_gray_device writes for that scan: COLOR_RGB2GRAY
 * applied to BGR memory order (quirk B8).  Any base address and any pitch: aligned dwords are read and written along the
 * rows, ragged row ends byte by byte, so nothing outside a row's cols * channels bytes is read and nothing outside its
 * cols bytes is written.  Enqueues only, like omr_rgb_to_gray_device.
 * OMR_ERR_BADARG: a null pointer, n <= 0, src_step < cols * channels, dst_step < cols, a stride below rows * step on
 * either side, source and destination ranges that overlap.  OMR_ERR_ASSERT: an empty image, a side of 32767 or more,
 * channels other than 3 or 4.  Every argument is checked before any device work. */
int omr_rgb_to_gray_batch_device(const uint8_t *d_src, int32_t n, int64_t src_stride_bytes, int64_t src_step, int32_t rows,
                                 int32_t cols, int32_t channels, uint8_t *d_dst, int64_t dst_stride_bytes, int64_t dst_step,
                                 void *stream);
/* erode(3x3 MORPH_ELLIPSE = cross, iterations = 3, BORDER_CONSTANT, default border): omr.rs:98-112 */
int omr_erode3_device(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols,
                      uint8_t *d_dst, int64_t dst_step, void *stream);
/* resize(src, dst size, INTER_AREA): transfer.rs:128-145 / omr.rs:114-126.  Integer shrink factors (the
 * callers' 0.2, 1240x1150 -> 248x230) run resizeAreaFast_; fractional shrink factors build resizeArea_'s
 * tap tables on the host and synchronise `stream` before returning; when an axis ENLARGES OpenCV emulates
 * INTER_AREA with its bilinear kernel (omr.rs:60-82 has no clamp on the scale: quirk B7) -- same here. */
int omr_resize_area_device(const uint8_t *d_src, int64_t src_step, int32_t src_rows, int32_t src_cols,
                           int32_t channels, uint8_t *d_dst, int64_t dst_step, int32_t dst_rows,
                           int32_t dst_cols, void *stream);
int omr_threshold_binary_device(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols,
                                uint8_t *d_dst, int64_t dst_step, void *stream);
/* rotate_mat's canvas (transfer.rs:472-498): DEFAULT keeps the size, CONTAIN grows it. */
int omr_rotate_size(int32_t rows, int32_t cols, double angle_deg, int32_t clip, int32_t *dst_rows,
                    int32_t *dst_cols);
/* rotate_mat on device buffers; dst_rows/dst_cols must equal omr_rotate_size()'s answer. */
int omr_rotate_device(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols,
                      int32_t channels, double angle_deg, double scale, int32_t interp,
                      const uint8_t border_value[4], int32_t clip, uint8_t *d_dst, int64_t dst_step,
                      int32_t dst_rows, int32_t dst_cols, void *stream);
/* rotate_mat with every flag and border mode warpAffine takes (transfer.rs:459-523 passes both through).
 * flags & 7 is the interpolation: NEAREST, LINEAR, CUBIC, LANCZOS4; 3 (INTER_AREA) is LINEAR, as in warpAffine;
 * 5..7 are OMR_ERR_NOTIMPL.  OMR_WARP_INVERSE_MAP uses rotate_mat's matrix as the dst->src map as it is;
 * OMR_WARP_FILL_OUTLIERS is ignored (warpAffine ignores it); any other bit is OMR_ERR_BADARG.  border_mode is
 * OMR_BORDER_CONSTANT..OMR_BORDER_TRANSPARENT (anything else, BORDER_ISOLATED included: OMR_ERR_BADARG).  Canvas
 * and matrix are omr_rotate's; channels 1..4.  Every argument is checked before any device work.  NEAREST and
 * LINEAR (or AREA) with BORDER_CONSTANT and without OMR_WARP_INVERSE_MAP take omr_rotate's path and give its bytes.
 * BORDER_TRANSPARENT: the device form leaves the skipped destination pixels as they were; the host form starts
 * from a zero-filled canvas, so they are 0 there (the reference writes into a fresh Mat: undefined). */
int omr_rotate_ex(const omr_image *src, double angle_deg, double scale, int32_t flags, int32_t border_mode,
                  const uint8_t border_value[4], int32_t clip, omr_image_owned *dst);
int omr_rotate_device_ex(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols, int32_t channels,
                         double angle_deg, double scale, int32_t flags, int32_t border_mode,
                         const uint8_t border_value[4], int32_t clip, uint8_t *d_dst, int64_t dst_step,
                         int32_t dst_rows, int32_t dst_cols, void *stream);
/* rotate_mat for a batch, an angle per image; scale, flags, border mode, border value and clip are the batch's.
 * Flags, border modes, channels and error codes are omr_rotate_device_ex's, and image i's canvas is byte for byte what
 * omr_rotate_device_ex writes for the same image, angle and parameters: the matrices come from the host's libm as
 * they do there, travel in one upload, and the same kernels run once with the image index in blockIdx.z.
 *
 * omr_rotate_batch_canvas (host only, no device needed): image i's canvas is omr_rotate_size(rows, cols, angles[i],
 * clip); *max_rows and *max_cols are the largest rows and the largest cols over the batch, each on its own, so every
 * canvas fits a max_rows x max_cols slot (DEFAULT: rows x cols).  out_size, when given: (rows, cols) of canvas i at
 * [2i], [2i + 1].
 *
 * omr_rotate_batch_device_ex: n same-shape images, image i at d_src + i * src_stride_bytes (any stride >= 0: 0
 * rotates one image by n angles), rows src_step apart.  Canvas i fills the top left of the slot d_dst +
 * i * dst_stride_bytes, rows dst_step apart; the slot's bytes outside the canvas are not written (nor are the pixels
 * BORDER_TRANSPARENT skips).  Its (rows, cols) land in the HOST array out_size when given.  OMR_ERR_BADARG besides
 * omr_rotate_device_ex's own: n <= 0, a null angle array, an angle that is not finite, a slot smaller than
 * omr_rotate_batch_canvas's answer, dst_step < channels * slot_cols, dst_stride_bytes < slot_rows * dst_step,
 * src_stride_bytes < 0, source and destination ranges that overlap.  Every argument is checked before any device
 * work.  The launches are enqueued on `stream`.  Batches of more than 3 images upload a per-call table of matrices and
 * SYNCHRONISE `stream` before the call returns, because the table is given back on return; smaller ones only enqueue.
 *
 * omr_rotate_batch_ex: host images of any mix of shapes and channel counts in, owned images out (dsts[i] belongs to
 * srcs[i]; free each with omr_image_free).  Same-shape images go through omr_rotate_batch_device_ex's path together.
 * On an error no image is returned.  BORDER_TRANSPARENT starts from zero-filled canvases, as omr_rotate_ex does. */
int omr_rotate_batch_canvas(int32_t rows, int32_t cols, const double *angles_deg, int32_t n, int32_t clip,
                            int32_t *max_rows, int32_t *max_cols, int32_t *out_size);
int omr_rotate_batch_device_ex(const uint8_t *d_src, int32_t n, int64_t src_stride_bytes, int64_t src_step,
                               int32_t rows, int32_t cols, int32_t channels, const double *angles_deg, double scale,
                               int32_t flags, int32_t border_mode, const uint8_t border_value[4], int32_t clip,
                               uint8_t *d_dst, int64_t dst_stride_bytes, int64_t dst_step, int32_t slot_rows,
                               int32_t slot_cols, int32_t *out_size, void *stream);
int omr_rotate_batch_ex(const omr_image *srcs, int32_t n, const double *angles_deg, double scale, int32_t flags,
                        int32_t border_mode, const uint8_t border_value[4], int32_t clip, omr_image_owned *dsts);
/* The fixed-point weight table the warp uses for OMR_INTER_CUBIC (k = 4) or OMR_INTER_LANCZOS4 (k = 8): OpenCV's
 * initInterTab2D(method, fixpt = true), 32 * 32 entries of k * k int16, entry fy * 32 + fx, tap row * k + col.
 * *n_out = 1024 * k * k; out == NULL only reports the size; cap < *n_out is OMR_ERR_BADARG.  Host only. */
int omr_warp_coeff_table(int32_t interp, int16_t *out, int32_t cap, int32_t *n_out);

/* ---- erode / dilate with any structuring element (transfer.rs:206-277) -------------------------
 * TransformableMatrix::erode / dilate call imgproc::erode / dilate with get_structuring_element(shape, size,
 * anchor), that anchor, `iterations`, BORDER_CONSTANT and morphology_default_border_value():
 *   dst(y, x) = min (erode) or max (dilate) over the set cells (i, j) of the element of src(y + i - ay, x + j - ax),
 * each channel on its own; positions outside the image take no part (255 for erode, 0 for dilate).  Dilate uses
 * the element unmirrored, as OpenCV does.  iterations == 0, or a 1 x 1 element, copies src; iterations < 0 is
 * OMR_ERR_BADARG; iterations > 1 is that many passes.  kw, kh and iterations have no upper limit (OMR_ERR_NOMEM
 * when a table or the intermediate image cannot be allocated); the element may be larger than the image.
 * Channels 1..4.  Every argument is checked before any device work. */

/* getStructuringElement(shape, Size(kw, kh), Point(ax, ay)) -> out[kh * kw], 0 or 1.  Host only.  An anchor
 * coordinate of -1 is the centre (kw / 2, kh / 2); a 1 x 1 element is RECT; CROSS: row ay full, column ax elsewhere;
 * ELLIPSE ignores the anchor: r = kh / 2, c = kw / 2, row i spans [max(c - dx, 0), min(c + dx + 1, kw)) with
 * dx = cvRound(c * sqrt((r * r - (i - r)^2) / (r * r))).  kw < 1, kh < 1, an anchor outside the element or an
 * unknown shape: OMR_ERR_ASSERT. */
int omr_structuring_element(int32_t shape, int32_t kw, int32_t kh, int32_t ax, int32_t ay, uint8_t *out);
/* per call, host memory to host memory; op: OMR_MORPH_ERODE / OMR_MORPH_DILATE */
int omr_morph(const omr_image *src, int32_t op, int32_t shape, int32_t kw, int32_t kh, int32_t ax, int32_t ay,
              int32_t iterations, omr_image_owned *dst);
/* device-resident; d_src == d_dst is OMR_ERR_BADARG.  Synchronises `stream` before returning when the call had
 * to take an intermediate image (more passes than one launch fuses) or a span table (elements over 31 x 31). */
int omr_morph_device(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols, int32_t channels,
                     int32_t op, int32_t shape, int32_t kw, int32_t kh, int32_t ax, int32_t ay, int32_t iterations,
                     uint8_t *d_dst, int64_t dst_step, void *stream);
/* n same-size images, image i at d_src + i * src_stride_bytes / d_dst + i * dst_stride_bytes, one launch per
 * pass (the image index is blockIdx.z); image i's result is byte-identical to omr_morph_device's. */
int omr_morph_batch_device(const uint8_t *d_src, int32_t n, int64_t src_stride_bytes, int64_t src_step, int32_t rows,
                           int32_t cols, int32_t channels, int32_t op, int32_t shape, int32_t kw, int32_t kh, int32_t ax,
                           int32_t ay, int32_t iterations, uint8_t *d_dst, int64_t dst_stride_bytes, int64_t dst_step,
                           void *stream);

/* ---- the projection pictures (transfer.rs:337-376, :409-455) ---------------------------
 * The input is 8-bit, one channel, ANY values (OMR_ERR_ASSERT for another channel count, an empty image or a side of
 * 32767 or more); each picture has the input's size.  What the reference's loops come to:
 *   horizontal, row r:  k0 = index of the first pixel == 255 (cols when the row has none), K = number of pixels != 255;
 *                       columns [0, k0) keep the source bytes, [k0, K) are 0, [K, cols) are 255;
 *   vertical, column c: n = number of pixels <= 127; rows [0, rows - n) are 255, rows [rows - n, rows) are 0.
 * On a strictly 0 / 255 image the black run of row r is omr_get_horizontal_projection()[r] long and the bar of column c
 * omr_get_vertical_projection()[c] high (those count == 0); on any other image the three predicates differ.
 * Either output may be NULL, not both (OMR_ERR_BADARG); a picture is the same whether or not the other is asked for.
 * OMR_ERR_BADARG besides: a null image or source pointer, n <= 0, a step below cols, a picture stride below rows * step,
 * a negative source stride (any stride >= 0 is taken: 0 draws one scan n times), d_src == a destination.  Every argument
 * is checked before any device work.  Source and destinations MUST NOT OVERLAP; only equal pointers are detected.
 * The bytes of a destination row past `cols` are never written: the caller's pitch padding stays as it was.
 * The device forms enqueue on `stream` only.  A call that draws the horizontal picture alone returns without
 * synchronising; one that draws the vertical picture takes a per-call table of column counts (n x cols uint32) and
 * SYNCHRONISES `stream` before it returns, because the table is given back on return (as omr_rotate_batch_device_ex).
 * Performance note: rows are read and written as dwords when the image's base, stride and step are multiples of 4;
 * any other layout takes byte accesses -- same pictures, slower. */
/* transfer_thresh_binary_to_{horizontal,vertical}_projection; owned images out (omr_image_free each) */
int omr_projection_pictures(const omr_image *src_u8c1, omr_image_owned *horizontal, omr_image_owned *vertical);
/* device-resident */
int omr_projection_pictures_device(const uint8_t *d_src, int64_t src_step, int32_t rows, int32_t cols,
                                   uint8_t *d_horizontal, int64_t h_step, uint8_t *d_vertical, int64_t v_step, void *stream);
/* n scans of one shape, scan i at d_src + i * src_stride_bytes; its pictures at d_horizontal + i * h_stride_bytes and
 * d_vertical + i * v_stride_bytes, byte for byte the per-call form's.  One set of launches for the batch (per 65535 scans). */
int omr_projection_pictures_batch_device(const uint8_t *d_src, int32_t n, int64_t src_stride_bytes, int64_t src_step,
                                         int32_t rows, int32_t cols, uint8_t *d_horizontal, int64_t h_stride_bytes,
                                         int64_t h_step, uint8_t *d_vertical, int64_t v_stride_bytes, int64_t v_step,
                                         void *stream);

/* ---- Hough-line deskew path ---------------------------------------------
 * OpenCV 4.6.0 semantics restated on the GPU: Canny is exact (integer stencils + a set-valued
 * hysteresis); HoughLinesP keeps hough.cpp's point order (cv::RNG seed 2^64-1), float32 votes and
 * 16.16 line walks, so the segments are the reference's segments, not an approximation. */

/* imgproc::canny(src, &mut edges, low, high, 3, false): call sites hough.rs:27 (50, 150 on the gray
 * scan), omr.rs:239 (on the 3-channel scan: per pixel the channel with the largest |dx|+|dy|),
 * omr.rs:323-330.  edges: 1 channel, 0 / 255. */
int omr_canny(const omr_image *src, double low_thresh, double high_thresh, omr_image_owned *edges);

/* imgproc::hough_lines_p(&edges, &mut lines, rho, theta, threshold, min_line_length, max_line_gap):
 * hough.rs:31-43, omr.rs:245-253 (rho 1, theta pi/180, threshold 0).  lines: cap x (x0, y0, x1, y1);
 * *n_lines = segments found (call again with a larger buffer if it exceeds cap).  theta must give
 * at most 256 accumulator angles (-213 otherwise). */
int omr_hough_lines_p(const omr_image *edges_u8c1, double rho, double theta, int32_t threshold,
                      double min_line_length, double max_line_gap, int32_t *lines, int32_t cap,
                      int32_t *n_lines);

/* oics::hough::get_angle_with_hough(&TransformableMatrix, min_line_length, max_line_gap, file_name,
 * edge_image_output_dir) -> Result<f64> (hough.rs:17-100; called core/src/main.rs:103-110,
 * app/src-tauri/src/test.rs:383-390).  No file arguments: encoding and writing the debug picture
 * (imwrite, hough.rs:91-96) is host-side codec work and stays with the caller; the picture itself --
 * the edge map in colour with every segment drawn on (hough.rs:44-63) -- comes from
 * omr_get_angle_with_hough_ex below.  No segment found: -215 (the reference panics on angles[0],
 * hough.rs:74). */
int omr_get_angle_with_hough(const omr_image *gray, double min_line_length, double max_line_gap,
                             double *angle_out);
/* The same detector -- Canny and HoughLinesP run once, *angle_out has the same bits -- which also hands
 * back the reference's picture in colour (186, 88, 255) as an owned 3-channel image (omr_image_free).
 * lined == NULL: exactly omr_get_angle_with_hough.  No segment found: -215 and no picture (lined->data
 * is NULL), as the reference panics before its imwrite. */
int omr_get_angle_with_hough_ex(const omr_image *gray, double min_line_length, double max_line_gap,
                                double *angle_out, omr_image_owned *lined);

/* ---- the detectors' line picture (hough.rs:44-63, fft.rs:173-213) --------------------
 * cvtColor(GRAY2BGR) of an 8-bit one-channel edge map (ANY values), then every segment (x0, y0, x1, y1), as
 * omr_hough_lines_p returns them, drawn on by imgproc::line(.., colour, 1, LINE_AA, 0) -- OpenCV 4.6.0 LineAA restated,
 * tests/lined_ref.py -- one after another in list order: LINE_AA blends into what is there, so where segments cross
 * the order shows.  bgr: the colour's three bytes (B, G, R).  n_lines == 0 gives the GRAY2BGR picture.
 * Every end point must lie inside the picture (HoughLinesP gives no others; clipLine is not restated): OMR_ERR_BADARG
 * otherwise -- found on the host by omr_lined_picture before any device work, by a first kernel in the device forms,
 * which then draw nothing.  OMR_ERR_BADARG besides: a null pointer, n <= 0, n_lines < 0, a line_offsets entry below its
 * predecessor or below 0, a step below cols (edges) or 3 * cols (picture), a picture stride below rows * out_step, a
 * negative edge-map stride, d_edges == d_out.  OMR_ERR_ASSERT: an empty image, a side of 32767 or more, and for the host
 * form a channel count other than 1.  All of these are checked before any device work.
 * The device forms enqueue on `stream` and SYNCHRONISE it before they return (the end-point verdict is read, the
 * per-call segment records are given back).  Picture bytes past 3 * cols of a row are never written.
 * Performance note: picture rows leave as dwords when the picture's base, stride and step are multiples of 4. */
int omr_lined_picture(const omr_image *edges_u8c1, const int32_t *lines, int32_t n_lines, const uint8_t bgr[3],
                      omr_image_owned *picture);
/* device-resident edge map and segments; the picture has its own row pitch */
int omr_lined_picture_device(const uint8_t *d_edges, int64_t edge_step, int32_t rows, int32_t cols,
                             const int32_t *d_lines, int32_t n_lines, const uint8_t bgr[3], uint8_t *d_out,
                             int64_t out_step, void *stream);
/* n edge maps of one shape, map i at d_edges + i * edge_stride_bytes, its picture at d_out + i * out_stride_bytes;
 * picture i draws the segments line_offsets[i] .. line_offsets[i + 1] of d_lines (line_offsets: HOST array of n + 1).
 * One drawing launch for the batch (per 65535 maps); every picture is byte for byte the per-call form's. */
int omr_lined_picture_batch_device(const uint8_t *d_edges, int32_t n, int64_t edge_stride_bytes, int64_t edge_step,
                                   int32_t rows, int32_t cols, const int32_t *d_lines, const int32_t *line_offsets,
                                   const uint8_t bgr[3], uint8_t *d_out, int64_t out_stride_bytes, int64_t out_step,
                                   void *stream);

/* ---- get_angle_with_hough for batches of scans ---------------------------------------
 * n device-resident scans of one shape (scan i at d_scans + i * scan_stride_bytes, rows step_bytes apart; channels 1,
 * 3 or 4, what omr_get_angle_with_hough accepts): Canny, HoughLinesP, the f32 vote within 0.1 degrees and its first
 * maximum for the whole batch, the segments staying on the device.  angles / rc / n_lines: HOST arrays of n (n_lines
 * may be NULL).  angles[i] has the f64 bits omr_get_angle_with_hough returns for scan i and rc[i] is OMR_OK; a scan
 * without any segment gets rc[i] = OMR_ERR_ASSERT (that function's code) and angles[i] = 0.0 -- the call itself still
 * returns OMR_OK: its own code reports bad arguments or a device failure only.
 * d_lined (may be NULL): picture i -- byte for byte omr_get_angle_with_hough_ex's, the edge map as Canny left it in
 * colour with every segment drawn on in (186, 88, 255) -- at d_lined + i * lined_stride_bytes, rows lined_step apart.
 * The slot of a scan without a segment is NOT written (the per-call form makes no picture there either), nor are the
 * bytes past 3 * cols of a row.
 * OMR_ERR_BADARG: a null d_scans / angles / rc, n <= 0, step_bytes < cols * channels, a negative scan stride,
 * lined_step < 3 * cols, lined_stride_bytes < rows * lined_step, d_lined == d_scans.  OMR_ERR_ASSERT: an empty image, a
 * side of 32767 or more, a channel count other than 1, 3 or 4.  All are checked before any device work.
 * Enqueues on `stream` and SYNCHRONISES it before it returns. */
int omr_hough_angles_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows,
                                  int32_t cols, int32_t channels, int64_t step_bytes, double min_line_length,
                                  double max_line_gap, double *angles, int32_t *rc, int32_t *n_lines,
                                  uint8_t *d_lined, int64_t lined_stride_bytes, int64_t lined_step, void *stream);
/* The same for host images of any mix of shapes and channel counts (1 / 3 / 4 each), bucketed by (rows, cols,
 * channels) as omr_get_angles_with_projections_batch does, on the current device: one upload and one device call per
 * bucket (per 64 of its scans; uploads and picture downloads on up to 16 host threads), angles[i] / rc[i] / lined[i]
 * belong to grays[i].  lined (n owned images,
 * omr_image_free each) may be NULL; lined[i].data is NULL where rc[i] != OMR_OK.  Every image is checked as
 * omr_get_angle_with_hough checks it before any device work, and an invalid one fails the whole call: angles and rc
 * are not written, and no picture is returned. */
int omr_get_angles_with_hough_batch(const omr_image *grays, int32_t n, double min_line_length, double max_line_gap,
                                    double *angles, int32_t *rc, omr_image_owned *lined);
/* For tests and inspection: the vote of hough.rs:72-89 alone, for n lists of f32 angles that live on the device --
 * list k is d_angles[d_offsets[k] .. d_offsets[k + 1]) (d_offsets: n + 1 non-decreasing int32 on the DEVICE).
 * d_winner[k] = the smallest i of list k with the largest #{ j : |a_i - a_j| < 0.1f }, in f32; -1 for an empty list.
 * The offsets are TRUSTED: they live on the device and are not validated -- they must not decrease and every list
 * must lie inside d_angles, or the kernel reads outside it.  Enqueue only, like omr_argmax_projection_device. */
int omr_hough_vote_select_device(const float *d_angles, const int32_t *d_offsets, int32_t n, int32_t *d_winner,
                                 void *stream);

/* oics::omr::get_result_from_edges_detection(&Mat, f64, f64) -> Result<OmrResult> (omr.rs:231-302). */
int omr_get_result_from_edges_detection(const omr_image *src, double edges_min_line_length,
                                        double edges_max_line_gap, double *angle, int32_t *status,
                                        double *candidates, int32_t cand_cap, int32_t *cand_len);

/* The same on n device-resident scans of one shape (one workgroup per scan in the sequential Hough
 * stage): BASELINE config 4.  angles / status / n_lines: host arrays of n; a scan without any
 * segment reports status NotAResult and angle 0 instead of the reference's panic. */
int omr_edges_detection_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes,
                                     int32_t rows, int32_t cols, int32_t channels, int64_t step_bytes,
                                     double min_line_length, double max_line_gap, double *angles,
                                     int32_t *status, int32_t *n_lines, void *stream);

/* Tuning knob of the batch above, process-wide: how many scans the sequential Hough stage works on at once
 * (= workgroups of its kernel; each finished workgroup takes the next scan of the batch).  Every scan in
 * flight keeps an accumulator (2.8 MB at A4) and a point mask (1.1 MB) hot, so the count trades cache
 * footprint against occupied compute units.  0 = the library's default (profiles/r03_hough.md).  Returns
 * the previous setting.  No counterpart in the reference (its OpenCV call is one scan per thread). */
int32_t omr_hough_set_scans_in_flight(int32_t scans);

/* The decision of correct_default (omr.rs:351-399): which angle to rotate by and whether the sheet
 * needs a manual check, from the projection result and the edges result. */
void omr_correct_default_decision(double proj_angle, int32_t proj_status, const double *proj_candidates,
                                  int32_t n_cand, double edges_angle, double *rotate_angle,
                                  int32_t *need_check);

/* oics::omr::correct_default(input_file, output_file, u16, f64, i32, i32, f64, f64) ->
 * Result<(f64, bool)> (omr.rs:339-448; called app/src-tauri/src/task.rs:38-47) on a decoded BGR
 * image: imread / imwrite stay on the host side of the shim.  rotated may be NULL. */
int omr_correct_default(const omr_image *src_bgr, uint16_t projection_max_angle,
                        double projection_angle_step, int32_t projection_max_width,
                        int32_t projection_max_height, double hough_min_line_length,
                        double hough_max_line_gap, double *rotate_angle, int32_t *need_check,
                        omr_image_owned *rotated);

/* ---- correct_default for batches of sheets ------------------------------
 * A context for repeated batches of one shape (rows x cols x channels) and one parameter set of omr_correct_default.
 * For every sheet that omr_correct_default accepts, the batch gives its results bit for bit: rotate_angle (as f64
 * bits), need_check and the rotated canvas (NEAREST, white border, CONTAIN, scale 1: size and every byte).
 * channels: 3 (BGR, as imread(IMREAD_COLOR) gives it) or 1 (the gray convenience omr_correct_default also accepts);
 * 4 is OMR_ERR_NOTIMPL, 2 is OMR_ERR_ASSERT as per call.  max_scans = the largest n a run may carry (1..65535). */
typedef struct omr_correct_batch omr_correct_batch;
int omr_correct_batch_create(int32_t rows, int32_t cols, int32_t channels, uint16_t projection_max_angle,
                             double projection_angle_step, int32_t projection_max_width,
                             int32_t projection_max_height, double hough_min_line_length,
                             double hough_max_line_gap, int32_t device, int32_t max_scans,
                             omr_correct_batch **out);
void omr_correct_batch_destroy(omr_correct_batch *cb);
/* Largest CONTAIN canvas any angle can give at rows x cols (cols rounded up to 4, as the batch warp's tables).
 * A pure function: no device needed. */
int omr_correct_batch_canvas(int32_t rows, int32_t cols, int32_t *max_rows, int32_t *max_cols);
/* n device-resident sheets (sheet i at d_scans + i * scan_stride_bytes, rows step_bytes apart) -> per sheet the
 * decision (host arrays of n: rotate_angle, need_check, scan_rc) and, when d_out != NULL, the rotated sheet: its
 * canvas fills the top-left of d_out + i * out_stride_bytes (rows out_step_bytes apart; every slot holds
 * omr_correct_batch_canvas() x channels) and its size lands in the host array out_size[2 i] (rows), [2 i + 1] (cols),
 * which may be NULL.  scan_rc[i] is what omr_correct_default returns for sheet i: 0, OMR_ERR_ASSERT when the Hough
 * fallback finds no segment (the reference panics there, quirk B11), OMR_ERR_NOMEM when it finds more segments than the
 * HoughLinesP buffer holds (65536); such a sheet gets no canvas and size 0 x 0, the other sheets' results stand.  The
 * sheets that are not Believed go through the Hough pass at most 256 at a time (a packed copy of them is the context's
 * largest buffer, up to 256 sheets).  The return value is for errors of the whole call; every argument is checked before
 * any device work.  Synchronous: the decision needs the host, and the call returns when everything is done.
 * Performance note: as for omr_batch_deskew_device_cn, the warp stages source boxes in LDS only when d_scans,
 * scan_stride_bytes and step_bytes are multiples of 4. */
int omr_correct_batch_run_device(omr_correct_batch *cb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                 int64_t step_bytes, int32_t n, double *rotate_angle, int32_t *need_check,
                                 int32_t *scan_rc, uint8_t *d_out, int64_t out_stride_bytes,
                                 int64_t out_step_bytes, int32_t *out_size);
/* How a context's front end (gray + erode x3 + INTER_AREA to the projection size) runs: */
#define OMR_CORRECT_FRONT_AREA_FUSED 0   /* integer factors <= 64 (1 x 1: no resize), one fused kernel */
#define OMR_CORRECT_FRONT_AREA_INT 1     /* integer factors, one of them > 64: eroded sheets, then resizeAreaFast_ */
#define OMR_CORRECT_FRONT_AREA_GENERAL 2 /* fractional shrink: eroded sheets, then resizeArea_ (tap tables) */
#define OMR_CORRECT_FRONT_LINEAR 3       /* an axis enlarges (quirk B7): eroded sheets, then the bilinear emulation */
/* For tests and inspection: the projection size (proj_rows x proj_cols), the front-end mode (OMR_CORRECT_FRONT_*) and
 * the integer shrink factors kx (across) and ky (down), 0 outside the two integer modes.  Pointers may be NULL. */
int omr_correct_batch_info(omr_correct_batch *cb, int32_t *proj_rows, int32_t *proj_cols, int32_t *front_mode,
                           int32_t *kx, int32_t *ky);
/* For tests and inspection: the front end of omr_correct_batch_run_device alone (same dispatch, chunks and stream) on
 * n sheets laid out as there; sheet i's projection-size image, before the threshold, lands in the top-left of
 * d_small + i * small_stride_bytes, rows small_step_bytes apart.  Arguments are checked as
 * omr_correct_batch_run_device does, and small_step_bytes >= proj_cols, small_stride_bytes >= proj_rows x
 * small_step_bytes.  Synchronous.  Runs do not depend on it. */
int omr_correct_batch_front_device(omr_correct_batch *cb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                   int64_t step_bytes, int32_t n, uint8_t *d_small, int64_t small_stride_bytes,
                                   int64_t small_step_bytes);
/* Host images of any shapes, bucketed by (rows, cols, channels) as omr_sweep_batch does, on the current device;
 * results land at the sheets' own positions.  rotated (n owned images, omr_image_free each) may be NULL; a sheet
 * with scan_rc[i] != 0 gets an empty image (data NULL) -- a shape whose projection size truncates to 0 gives every
 * one of its sheets OMR_ERR_ASSERT, as per call.  Runs of up to 256 sheets per shape go through a context the library
 * keeps for later calls with the same device, shape and parameters (the last 4 are kept); uploads and the copies of
 * the rotated sheets into fresh host images run on up to 16 host threads.  On an error of the whole call no image is
 * returned.  When the rotated IMAGES are wanted this form is slower than omr_correct_default from 16 host threads (about
 * 650 sheets/s against 825 on 1150 x 1240 sheets, 3 183 at A4: profiles/r06_correct_batch.md); when the FILES are
 * wanted, omr_correct_default_batch_jpeg below is the faster way (figures and their baseline there).  The
 * device-resident omr_correct_batch_run_device is the fast path. */
int omr_correct_default_batch(const omr_image *srcs, int32_t n, uint16_t projection_max_angle,
                              double projection_angle_step, int32_t projection_max_width,
                              int32_t projection_max_height, double hough_min_line_length,
                              double hough_max_line_gap, double *rotate_angle, int32_t *need_check,
                              int32_t *scan_rc, omr_image_owned *rotated);

/* ---- get_angle_with_projections with its resize_scale for batches of scans ---------------
 * A context for repeated batches of one shape (rows x cols x channels) and one parameter set of
 * omr_get_angle_with_projections.  The reference's order (projection.rs:24-32): scale_self(resize_scale) on the COLOUR
 * scan (transfer.rs:66-91: size truncated with `as i32`, INTER_AREA when the scale is <= 1, INTER_LINEAR above), then
 * RGB2GRAY, threshold(127), the sweep.  Here the whole batch is resized in one launch into a working buffer the
 * context owns (max_scans x wrows x wcols x channels); gray and threshold stay fused in the sweep's loads, so no
 * full-size intermediate is written and every scan byte is read from memory once.  For every scan that
 * omr_get_angle_with_projections accepts, the batch gives its angle as the same f64 bits.
 * channels: 3 (BGR, as imread(IMREAD_COLOR) gives it) or 1 (the gray convenience the per-call function also accepts);
 * 4 is OMR_ERR_NOTIMPL, 2 is OMR_ERR_ASSERT as per call.  max_scans = the largest n a run may carry (1..65535).
 * A working size that truncates to 0 on an axis is OMR_ERR_ASSERT, as per call; an empty candidate range, a
 * resize_scale that is <= 0 or not finite: OMR_ERR_BADARG.  The resize tap tables of a fractional shrink are built
 * when the context is created and stay on the device: a run uploads no table and allocates nothing (the first run
 * that asks for scores sizes their device buffer). */
typedef struct omr_projection_batch omr_projection_batch;
/* How a context's front end (scale_self on the colour scans) runs; the dispatch is resize()'s in OpenCV 4.6.0: */
#define OMR_PROJECTION_FRONT_NONE 0         /* resize_scale == 1.0 (or the size does not change): the scans are swept as they are */
#define OMR_PROJECTION_FRONT_AREA_INT 1     /* both shrink factors are integers: resizeAreaFast_ */
#define OMR_PROJECTION_FRONT_AREA_GENERAL 2 /* any other shrink: resizeArea_ (tap tables) */
#define OMR_PROJECTION_FRONT_LINEAR 3       /* resize_scale > 1: the bilinear kernel */
/* scale_self's size for rows x cols and the mode above.  A pure function: no device needed. */
int omr_projection_batch_working_size(int32_t rows, int32_t cols, double resize_scale, int32_t *wrows, int32_t *wcols,
                                      int32_t *front_mode);
int omr_projection_batch_create(int32_t rows, int32_t cols, int32_t channels, uint16_t max_angle, double step,
                                double resize_scale, int32_t device, int32_t max_scans, omr_projection_batch **out);
void omr_projection_batch_destroy(omr_projection_batch *pb);
/* For tests and inspection: the working size, the front-end mode (OMR_PROJECTION_FRONT_*) and the number of
 * candidates A.  Pointers may be NULL. */
int omr_projection_batch_info(omr_projection_batch *pb, int32_t *wrows, int32_t *wcols, int32_t *front_mode,
                              int32_t *candidates);
/* For tests and inspection: the front end of omr_projection_batch_run_device alone (same dispatch, kernels and
 * stream) on n scans laid out as there; scan i's working image (channels interleaved, before gray and threshold)
 * lands in the top-left of d_small + i * small_stride_bytes, rows small_step_bytes apart: byte for byte what omr_scale
 * returns for the scan.  Arguments are checked as omr_projection_batch_run_device does, and small_step_bytes >=
 * wcols x channels, small_stride_bytes >= wrows x small_step_bytes.  Synchronous.  Runs do not depend on it. */
int omr_projection_batch_front_device(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                      int64_t step_bytes, int32_t n, uint8_t *d_small, int64_t small_stride_bytes,
                                      int64_t small_step_bytes);
/* n device-resident scans (scan i at d_scans + i * scan_stride_bytes, rows step_bytes apart; any stride >= 0) -> host
 * arrays: angle[i] = (best_idx[i] - N) * step (projection.rs:189-190), best_idx (n, may be NULL), v_sd / h_sd (n x A
 * scores, may be NULL).  OMR_ERR_BADARG: a null context, scan or angle pointer, n <= 0 or n > max_scans, step_bytes <
 * channels x cols, a negative stride; every argument is checked before any device work.  Synchronous.
 * Performance note: the resize kernel stages its source rows with dword loads, which needs d_scans, scan_stride_bytes
 * and step_bytes to be multiples of 4; otherwise (e.g. a 453-column colour scan, tightly packed) it stages them byte
 * by byte -- same result, slower. */
int omr_projection_batch_run_device(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                    int64_t step_bytes, int32_t n, double *angle, int32_t *best_idx, double *v_sd,
                                    double *h_sd);
/* Host images of any mix of shapes, bucketed by (rows, cols, channels) as omr_correct_default_batch does, on the
 * current device; angles[i] (and best_idx[i], which may be NULL) belong to srcs[i].  Every image is checked as
 * omr_get_angle_with_projections checks it before any device work, and an invalid one fails the whole call: nothing is
 * written to the outputs.  Runs of up to 256 scans per shape go through a context the library keeps for later calls
 * with the same device, shape and parameters (the last 4 are kept); uploads run on up to 16 host threads.  A bucket a
 * batch context does not take -- 4 channels, a sweep it cannot plan -- goes through omr_get_angle_with_projections
 * image by image, so every image that function accepts is accepted here, with the same answer.
 * Whether this form beats omr_get_angle_with_projections from 16 host threads has NOT been measured yet
 * (profiles/r08_projection_batch.md): like omr_correct_default_batch it pays for uploading every full-size scan, so
 * expect the device-resident omr_projection_batch_run_device to be the fast path. */
int omr_get_angles_with_projections_batch(const omr_image *srcs, int32_t n, uint16_t max_angle, double step,
                                          double resize_scale, double *angles, int32_t *best_idx);
/* ---- ... and the deskewed full-size scans: the reference's benchmark flow, core/src/main.rs:68-95
 * (get_angle_with_projections on the shrunk working image, then rotate_mat of the full-size original by that angle).
 * Largest CONTAIN canvas any candidate angle gives at the context's FULL shape rows x cols (not the working shape), cols
 * rounded up to 4 as omr_batch_deskew_canvas does: what every output slot of omr_projection_batch_deskew_device must
 * hold.  Planned when the context is created: host arithmetic, no device call.  OMR_ERR_BADARG for a null argument;
 * OMR_ERR_ASSERT when a candidate's canvas reaches 32767 on a side (omr_rotate fails there too). */
int omr_projection_batch_deskew_canvas(omr_projection_batch *pb, int32_t *max_rows, int32_t *max_cols);
/* omr_projection_batch_run_device's front end, sweep and arg-max, then every full-size scan warped by its own winner --
 * read on the device, no host round trip in between -- into d_out + i * out_stride_bytes (rows out_step_bytes apart;
 * the canvas fills the slot's top left, the slot's other bytes are not written): CONTAIN, scale 1, BORDER_CONSTANT with
 * border_value (channel c = border_value[c]), the context's channel count; interp OMR_INTER_NEAREST or
 * OMR_INTER_LINEAR.  Host arrays: out_size (2 n: rows, cols of canvas i), angle (n), best_idx (n, may be NULL), written
 * once, at the end.  angle[i] has the f64 bits of omr_get_angle_with_projections, and canvas i is byte for byte what
 * omr_rotate_device writes for scan i and that angle.
 * OMR_ERR_BADARG: what omr_projection_batch_run_device refuses, a null border_value / d_out / out_size / angle, or a
 * slot smaller than the canvas (out_step_bytes < max_cols x channels, out_stride_bytes < max_rows x out_step_bytes);
 * OMR_ERR_NOTIMPL: any other interp, as omr_batch_deskew_device_cn.  Every argument is checked before any device work,
 * and a refused call writes nothing.  Synchronous.
 * Performance note: as for omr_batch_deskew_device_cn, the warp stages source boxes in LDS only when d_scans,
 * scan_stride_bytes and step_bytes are multiples of 4, and only while a tile's source box fits (colour: winners up to
 * about 27 degrees; beyond, taps come from global memory: DESIGN.md section 4.3). */
int omr_projection_batch_deskew_device(omr_projection_batch *pb, const uint8_t *d_scans, int64_t scan_stride_bytes,
                                       int64_t step_bytes, int32_t n, int32_t interp, const uint8_t border_value[4],
                                       uint8_t *d_out, int64_t out_stride_bytes, int64_t out_step_bytes,
                                       int32_t *out_size, double *angle, int32_t *best_idx);
/* The same for host images of any mix of shapes, bucketed and run through cached contexts exactly as
 * omr_get_angles_with_projections_batch does; rotated (n owned images, omr_image_free each) gets image i's deskewed
 * canvas: what omr_rotate(srcs[i], angles[i], 1.0, interp, border_value, OMR_CLIP_CONTAIN) returns.  A bucket a batch
 * context does not take (4 channels, a sweep it cannot plan) goes image by image through
 * omr_get_angle_with_projections and omr_rotate.  interp other than NEAREST / LINEAR: OMR_ERR_NOTIMPL.  On an error of
 * the whole call nothing is written and no image is returned.  Device memory: a run carries up to 32 scans of a shape,
 * each with its scan and an output slot of the largest canvas (26 + 54 MB for an A4 colour sheet at +-45 degrees). */
int omr_deskew_with_projections_batch(const omr_image *srcs, int32_t n, uint16_t max_angle, double step,
                                      double resize_scale, int32_t interp, const uint8_t border_value[4],
                                      double *angles, int32_t *best_idx, omr_image_owned *rotated);

/* ---- FFT deskew path ------------------------------------------------------
 * The 2-D DFT is float32 like the reference's (dft on CV_32F); it is a different factorisation than
 * OpenCV's (radix-2 Stockham / Bluestein chirp-z in LDS), so the 8-bit spectrum pictures agree with
 * the CPU restatement to about one grey level, not bit for bit.  Everything after the picture
 * (Canny, HoughLinesP, votes) is the exact chain of the Hough-line path.  Any axis length up to the image
 * limit (32766) is transformed: lengths <= 8192 and the power of two 16384 inside LDS, longer lines by a chirp-z
 * through global memory (slower: a 600-dpi A3 scan, 9921 x 14032, takes about 12 ms). */

/* oics::fft::get_fft_image(&TransformableMatrix) -> Result<(Mat, Mat)> (fft.rs:124-141):
 * (magnitude_image, magnitude_log_image), both 8-bit single channel.  Either output may be NULL. */
int omr_get_fft_image(const omr_image *gray_u8c1, omr_image_owned *magnitude_image,
                      omr_image_owned *magnitude_log_image);

/* Inspection hook (like omr_hough_vote_select_device and omr_correct_batch_front_device: for the tests, not part of the
 * reference's surface): omr_get_fft_image's run -- the same two passes and picture kernel, one execution -- which also
 * hands back the float arrays the pictures are made from.  R = rows, C = cols, H = C / 2 + 1 (the input is real: the
 * columns beyond C / 2 are mirror images and are never computed).  All arrays are HOST memory, packed, column index major:
 *   row_pass   2 * H * R floats, (re, im) pairs: [c * R + r] = sum_x img(r, x) exp(-2 pi i c x / C), img = u8 * (1 / 255),
 *              the row pass's complex half spectrum, unscaled
 *   magnitude  H * R floats: [c * R + k] = |F(k, c)|, F = DFT2(img) / (R C), exactly as the column pass left it:
 *              UNSHIFTED (DC at [0]); fft_shift (fft.rs:67-86) and the mirror |F(k, c)| = |F((R - k) % R, C - c)| for
 *              c > C / 2 are applied by the picture kernel alone
 *   extrema    2 floats: min |F| and max |F| over the H * R points, as the picture kernel reads them
 *   magnitude_image, magnitude_log_image: the two pictures of the SAME run, as omr_get_fft_image returns them
 * Every output may be NULL (all of them NULL: OMR_ERR_BADARG).  Argument checks as omr_get_fft_image; a refused or
 * failed call writes nothing. */
int omr_fft_spectrum_raw(const omr_image *gray_u8c1, float *row_pass, float *magnitude, float *extrema,
                         omr_image_owned *magnitude_image, omr_image_owned *magnitude_log_image);

/* The magnitude_log pictures of n device-resident scans of one shape (BASELINE config 5):
 * d_magnitude_log: n x rows x cols bytes, packed. */
int omr_fft_image_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows,
                               int32_t cols, int64_t step_bytes, uint8_t *d_magnitude_log, void *stream);

/* oics::fft::get_angle_with_fft(&TransformableMatrix, canny_threshold_1, canny_threshold_2,
 * min_line_length, max_line_gap, file_name, edge_image_output_dir) -> Result<f64> (fft.rs:145-256;
 * called core/src/main.rs:141-150, app/src-tauri/src/test.rs:450-459).  Writing the debug picture stays
 * with the caller (as for omr_get_angle_with_hough); omr_get_angle_with_fft_ex makes it.  Keeps the vote's
 * quirk (fft.rs:231 re-reads line i). */
int omr_get_angle_with_fft(const omr_image *gray_u8c1, double canny_threshold_1, double canny_threshold_2,
                           double min_line_length, double max_line_gap, double *angle_out);
/* The same detector -- the transform, Canny and HoughLinesP run once, *angle_out has the same bits -- which also
 * hands back the reference's picture (fft.rs:173-213): the edges of the log spectrum in colour with every segment
 * drawn on in (186, 88, 255), an owned 3-channel image.  lined == NULL: exactly omr_get_angle_with_fft.  No segment
 * found: angle 0 and the bare GRAY2BGR picture, as the reference gives. */
int omr_get_angle_with_fft_ex(const omr_image *gray_u8c1, double canny_threshold_1, double canny_threshold_2,
                              double min_line_length, double max_line_gap, double *angle_out, omr_image_owned *lined);

/* ---- get_angle_with_fft for batches of scans ------------------------------------------
 * n device-resident 8-bit single-channel scans of one shape (scan i at d_scans + i * scan_stride_bytes, rows step_bytes
 * apart): the log-spectrum pictures in groups of up to 8 scans a launch (as omr_fft_image_batch_device), then Canny
 * (canny_threshold_1, canny_threshold_2), HoughLinesP (threshold 100) and the packed segment list for the whole batch,
 * as omr_hough_angles_batch_device runs them, and the vote of fft.rs:197-247 on the host.  angles / n_lines: HOST
 * arrays of n (n_lines may be NULL).  angles[i] has the f64 bits omr_get_angle_with_fft returns for scan i.  There is no
 * per-scan code: as in the per-call form a scan without any segment gives angle 0.0 and succeeds.
 * d_lined (may be NULL): picture i -- byte for byte omr_get_angle_with_fft_ex's -- at d_lined + i * lined_stride_bytes,
 * rows lined_step apart.  EVERY slot is written: a scan without a segment gets the bare GRAY2BGR edge picture, as the
 * per-call form gives (this is the difference from omr_hough_angles_batch_device, whose per-call form makes no picture
 * there).  Bytes past 3 * cols of a picture row and bytes between pictures are not written.
 * OMR_ERR_BADARG: a null d_scans / angles, n <= 0, step_bytes < cols, a negative scan stride, lined_step < 3 * cols,
 * lined_stride_bytes < rows * lined_step, d_lined == d_scans.  OMR_ERR_ASSERT: an empty image, a side of 32767 or more.
 * All are checked before any device work.  An axis length the transform does not take is reported as by
 * omr_fft_image_batch_device (OMR_ERR_NOTIMPL, when the tables are built).
 * Device memory: for the WHOLE batch at once the library allocates the log pictures and the edge maps (2 bytes a
 * pixel) and, with pictures, a copy of the edge maps (3 in all); the caller's own picture buffer is another 3 bytes a
 * pixel, 6 resident together.  On top come HoughLinesP's point lists (8 bytes per edge pixel), its accumulator and
 * point mask per scan, and the transform's workspace of at most 1 GiB.  n is taken as it is, so the caller bounds it
 * (the host form goes 64 scans at a time).
 * Enqueues on `stream` and SYNCHRONISES it before it returns, on every path. */
int omr_fft_angles_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows,
                                int32_t cols, int64_t step_bytes, double canny_threshold_1, double canny_threshold_2,
                                double min_line_length, double max_line_gap, double *angles, int32_t *n_lines,
                                uint8_t *d_lined, int64_t lined_stride_bytes, int64_t lined_step, void *stream);
/* The same for host images of any mix of shapes, bucketed by shape as omr_get_angles_with_hough_batch does, on the
 * current device: one upload and one device call per bucket (per 64 of its scans; uploads and picture downloads on up
 * to 16 host threads); angles[i] / lined[i] belong to grays[i].  lined (n owned images, omr_image_free each) may be
 * NULL; every lined[i] is filled.  Every image is checked as omr_get_angle_with_fft checks it before any device work,
 * and an invalid one fails the whole call: angles is not written, and no picture is returned. */
int omr_get_angles_with_fft_batch(const omr_image *grays, int32_t n, double canny_threshold_1,
                                  double canny_threshold_2, double min_line_length, double max_line_gap,
                                  double *angles, omr_image_owned *lined);

/* oics::omr::get_result_from_fourier_transform(&Mat, weak, strong, min_line_length, max_line_gap) ->
 * Result<OmrResult> (omr.rs:304-337) on the 3/4-channel scan. */
int omr_get_result_from_fourier_transform(const omr_image *src, double canny_threshold_weak,
                                          double canny_threshold_strong, double fourier_min_line_length,
                                          double fourier_max_line_gap, double *angle, int32_t *status,
                                          double *candidates, int32_t cand_cap, int32_t *cand_len);
/* The same on n device-resident colour scans of one shape (3 or 4 channels; layout as above): RGB2GRAY per scan, the
 * log pictures of the batch, Canny(weak, strong) on them, then omr_edges_detection_batch_device's chain on the edge
 * pictures.  angles / status / n_lines: HOST arrays of n (status and n_lines may be NULL); angles[i] / status[i] are
 * omr_get_result_from_fourier_transform's for scan i, and a scan without any segment reports OMR_STATUS_NOT_A_RESULT
 * and angle 0.0 where that function fails.  OMR_ERR_BADARG: a null d_scans / angles, n <= 0, step_bytes < cols *
 * channels, a negative scan stride.  OMR_ERR_ASSERT: an empty image, a side of 32767 or more, channels other than 3
 * or 4.  All are checked before any device work.  Device memory for the whole batch at once: the gray scans (reused
 * for the edge pictures), the log pictures and the second Canny's edge maps, 3 bytes a pixel, plus HoughLinesP's point
 * lists, accumulator and point mask per scan as in omr_edges_detection_batch_device, and the workspace (<= 1 GiB).
 * Enqueues on `stream` and SYNCHRONISES it before it returns. */
int omr_fourier_transform_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows,
                                       int32_t cols, int32_t channels, int64_t step_bytes, double canny_threshold_weak,
                                       double canny_threshold_strong, double fourier_min_line_length,
                                       double fourier_max_line_gap, double *angles, int32_t *status, int32_t *n_lines,
                                       void *stream);

/* ---- baseline JPEG encoding on the device ---------------------------------------------------
 * What imwrite(.., JPEG, quality) writes: byte for byte, SOI to EOI, libjpeg's stream after jpeg_set_defaults +
 * jpeg_set_quality(quality, TRUE) -- JFIF 1.01 APP0 (no units, density 1 x 1), one DQT per table, SOF0, the standard
 * Huffman tables of Annex K, no restart interval, not optimised, not progressive, forward DCT JDCT_ISLOW.  3 channels
 * (BGR in memory) give YCbCr 4:2:0, interleaved; 1 channel gives a single-component scan.  quality outside 1..100 is
 * clamped (0 -> 1, above 100 -> 100), as libjpeg and imwrite do.  4 channels: OMR_ERR_NOTIMPL; 2: OMR_ERR_ASSERT.
 * Decoding: the omr_jpeg_info / omr_jpeg_decode* section below.
 *
 * The two quantisation tables of `quality` in natural (not zig-zag) order.  Host only. */
int omr_jpeg_quant_tables(int32_t quality, uint16_t luma[64], uint16_t chroma[64]);
/* An upper bound of the stream's length for a rows x cols x channels image of any content at any quality: the header
 * (at most 623 bytes), every block of the scan at its longest code (a DC code of 11 bits with 11 value bits, 63 AC codes
 * of 16 bits with 10 value bits: 1660 bits) with every byte stuffed, and EOI.  OMR_ERR_ASSERT for an empty image or a
 * side above 65535.  Host only. */
int omr_jpeg_bound(int32_t rows, int32_t cols, int32_t channels, int64_t *bytes);
/* n device-resident images, image i at d_imgs + i * img_stride_bytes with rows step_bytes apart, each in a slot of rows x
 * cols x channels.  sizes: HOST array of n x (rows, cols) -- the layout of out_size of omr_correct_batch_run_device and
 * omr_projection_batch_deskew_device, whose canvases feed straight in -- or NULL when every image fills its slot; an
 * entry is at most the slot's size and its image lies at the slot's top left; a 0 x 0 entry gives out_len[i] = 0 and
 * leaves its output slot untouched.  Stream i starts at d_out + i * out_stride_bytes (>= omr_jpeg_bound of the slot) and
 * is out_len[i] bytes long (HOST array); nothing is written behind it.  OMR_ERR_BADARG: a null d_imgs / d_out / out_len,
 * n < 0, step_bytes < cols x channels, img_stride_bytes < rows x step_bytes, a sizes entry that is negative, half empty
 * or larger than the slot, out_stride_bytes below the bound.  OMR_ERR_ASSERT besides the shapes above: a slot whose
 * scan could take more than 2^32 bits (about 2.58 million blocks: bit offsets inside an image are 32-bit).  Every argument is
 * checked before any device work.  Synchronous, on a stream of its own, which has drained on every return path. */
int omr_jpeg_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows,
                                 int32_t cols, int32_t channels, const int32_t *sizes, int32_t n, int32_t quality,
                                 uint8_t *d_out, int64_t out_stride_bytes, int64_t *out_len);
/* A host image -> its stream in `out` (cap bytes), *len = the stream's length.  cap too small (out may be NULL when cap
 * is 0): OMR_ERR_NOMEM with *len = the length needed, nothing written. */
int omr_jpeg_encode(const omr_image *src, int32_t quality, uint8_t *out, int64_t cap, int64_t *len);
/* omr_correct_default_batch with every sheet's rotated canvas encoded on the device and only the streams downloaded:
 * jpeg[i] (malloc'ed, release with omr_bytes_free) holds jpeg_len[i] bytes, NULL / 0 where scan_rc[i] != 0.  Same
 * buckets, context cache and results; on an error of the whole call no stream is returned.  A shape whose canvas slot
 * (omr_correct_batch_canvas) could take more than 2^32 bits of scan data -- colour sheets from about 7400 x 7400 --
 * refuses the call with OMR_ERR_ASSERT before any device work.  Where the files are the result this form is the FASTER
 * one.  Measured at quality 100 (profiles/r17_jpeg.md): 1.2 k sheets/s on the dataset's sheets (about 1150 x 1240, four
 * shapes) and 0.7 k at A4.  The baseline is Pillow (libjpeg-turbo) called from 16 Python threads behind
 * omr_correct_default_batch, 80 and 6 sheets/s, or inside 16 threads of omr_correct_default, 78 and 6.5: 15 x and about
 * 110 x.  Those threads encode no faster than one (31 ms per A4 sheet, 2.8 ms per dataset sheet on one core); a host with
 * an encoder process per core was not measured and would be bound by the correction (650 to 825 sheets/s on dataset-size
 * sheets) or by about 520 A4 sheets/s of encoding. */
int omr_correct_default_batch_jpeg(const omr_image *srcs, int32_t n, uint16_t projection_max_angle,
                                   double projection_angle_step, int32_t projection_max_width,
                                   int32_t projection_max_height, double hough_min_line_length,
                                   double hough_max_line_gap, int32_t quality, double *rotate_angle, int32_t *need_check,
                                   int32_t *scan_rc, uint8_t **jpeg, int64_t *jpeg_len);
void omr_bytes_free(uint8_t *bytes);

/* ---- baseline JPEG decoding on the device ---------------------------------------------------
 * What imread returns: byte for byte libjpeg's output with its defaults (JDCT_ISLOW, fancy up-sampling, no scaling).
 * Streams taken: SOF0, 8 bit, Huffman, one scan; 1 component whatever sampling factors (1..4) it declares -- its scan is
 * not interleaved, one MCU is one block (T.81 A.2.2) -- or 3 components (YCbCr) with Y at 1 x 1, 2 x 1 or 2 x 2 and
 * chroma at 1 x 1 (4:4:4, 4:2:2, 4:2:0); any DHT / DQT tables under any ids, with or without a restart interval, any
 * APPn / COM segments and fill bytes before markers, intervals padded with any bits.  channels = 1 gives the Y plane (of
 * a gray or a colour stream), channels = 3 BGR in memory (B = G = R for a gray stream).
 * OMR_ERR_NOTIMPL, never a wrong picture: SOF1 / SOF2 and the other frame types, 12-bit samples, arithmetic coding, more
 * than one scan, 4 components, other sampling factors of a 3-component frame, an Adobe APP14 segment or component ids
 * R G B, 16-bit quantisation tables, DNL, an EXIF orientation other than 1 (imread would turn the image).
 * OMR_ERR_BADARG: a malformed header -- no SOI, a segment running past the end, a table that SOS names but nobody
 * defined, a size of 0.  OMR_ERR_ASSERT: entropy data that ends early, runs into an invalid code, has other restart
 * markers than DRI predicts or leaves blocks over (the image's content is then unspecified); entropy data of 2^32 bits
 * or more.  Where libjpeg's C code masks out-of-range IDCT results into its range-limit table the kernels saturate, as
 * libjpeg-turbo's SIMD code does; on what an encoder writes the two agree.
 * Measured at 256 host streams a call, upload included (profiles/r18_jpeg_decode.md): 22.5 k of the dataset's sheets a
 * second, 476 A4 colour images/s at quality 100 and 933 at 95; Pillow (libjpeg-turbo) from 16 threads of the same machine
 * decodes 1096, 105 and 122.  From files to files, omr_correct_default_batch_streams below corrects 1264 dataset sheets/s
 * and 140 A4 sheets/s, 2.2 x and 2.3 x omr_correct_default_batch_jpeg with Pillow's decode of its inputs on 16 threads
 * inside the timed region (585 and 62).
 *
 * What a stream's header says: its size, components (1 or 3) and Y's sampling factors as in SOF (0x11, 0x21, 0x22;
 * 0x11 for 1 component, whatever SOF declares).
 * Returns 0, OMR_ERR_NOTIMPL or OMR_ERR_BADARG by the rules above; the size is filled in whenever SOF was readable
 * (else 0).  Any output pointer may be NULL.  Host only. */
int omr_jpeg_info(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *components, int32_t *sampling);
/* n streams in HOST memory -> device-resident images, image i at d_out + i * out_stride_bytes at the top left of a slot of
 * rows x cols x channels with rows step_bytes apart; bytes of a slot outside its image are untouched.  out_size[2 i],
 * [2 i + 1] = image i's rows, cols (HOST array, the layout omr_jpeg_encode_batch_device and the batch contexts take; 0 x 0
 * where rc[i] != 0), rc[i] = 0 or the image's code by the rules above, OMR_ERR_BADARG also for an image larger than the
 * slot (HOST array).  The call itself returns 0 whatever the rc[i].  OMR_ERR_BADARG for the call: n < 0, a null pointer
 * (a null streams[i] included), channels other than 1 or 3, an empty slot, step_bytes < cols x channels,
 * out_stride_bytes < rows x step_bytes.  Every argument and every header is checked before any device work; a call all
 * of whose streams are refused does none.  Synchronous, on a stream of its own, which has drained on every return path. */
int omr_jpeg_decode_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                 uint8_t *d_out, int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                                 int32_t *out_size, int32_t *rc);
/* imread of one buffer: the stream -> a packed host image of `channels` channels (release with omr_image_free). */
int omr_jpeg_decode(const uint8_t *stream, int64_t len, int32_t channels, omr_image_owned *dst);
/* Measurement aid.  Reports what the calling thread's last decode (any of the entry points that decode, on this thread)
 * took, then switches the collection on (enable != 0) or off for the thread's next ones: *sub_bits = the subsequence
 * length the library is built with, *groups = the groups of launches, *rounds = the most synchronisation rounds a group
 * needed (round 0 included), stage_ms[0 .. 5] = device time summed over the groups of upload and clearing, un-stuffing,
 * the synchronisation rounds (their host round trips included), the coefficient pass, the inverse DCT, up-sampling and
 * colour.  All zero when the collection was off.  While on, every group records seven events; results do not change.
 * Any output pointer may be NULL. */
int omr_jpeg_decode_stats(int32_t enable, int32_t *sub_bits, int32_t *groups, int32_t *rounds, double *stage_ms);
/* correct_default from file contents to file contents: omr_correct_default_batch_jpeg with the sheets given as baseline
 * JPEG or PNG streams in host memory (what imread(IMREAD_COLOR) would be given).  A stream that begins with PNG's eight
 * signature bytes (89 50 4E 47 0D 0A 1A 0A) goes by the rules of omr_png_decode_batch_device below, every other one by
 * those of omr_jpeg_decode_batch_device; one batch, and one bucket, may hold both kinds.  The headers are parsed and the
 * sheets bucketed by shape on the host; each bucket is decoded to BGR straight into the scan slots of the cached
 * omr_correct_batch context, corrected and its canvases encoded on the device, so only streams cross the link in either
 * direction.  Outputs (JPEG streams, whatever the input was) as omr_correct_default_batch_jpeg, and identical to what that
 * function returns for imread's decode of the same streams.  A sheet its decoder refuses or whose header is malformed gets
 * that code in scan_rc[i], angle 0 and no output, before any device work; one whose image data is damaged gets
 * OMR_ERR_ASSERT there; the other sheets are unaffected.  OMR_ERR_BADARG for the call: a null pointer (a null streams[i]
 * included), n < 1, a negative length. */
int omr_correct_default_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                      uint16_t projection_max_angle, double projection_angle_step,
                                      int32_t projection_max_width, int32_t projection_max_height,
                                      double hough_min_line_length, double hough_max_line_gap, int32_t quality,
                                      double *rotate_angle, int32_t *need_check, int32_t *scan_rc, uint8_t **jpeg,
                                      int64_t *jpeg_len);

/* ---- PNG decoding on the device ---------------------------------------------------------------
 * What imread returns, byte for byte: libpng's rows after the transforms OpenCV 4.6 sets up -- palette -> RGB, gray of
 * 1 / 2 / 4 bits -> 8 bits, alpha dropped (no blending, no gamma), RGB -> BGR in memory, gray replicated for 3 channels.
 * Streams taken: non-interlaced; colour types 0, 2, 3, 4, 6 at bit depth 8, colour types 0 and 3 also at 1, 2 and 4;
 * any IDAT split, any deflate block kinds, any window size, every filter type; ancillary chunks are skipped without a
 * CRC check (tRNS, gAMA, iCCP, sRGB included).  channels = 3 from any of them, channels = 1 from colour types 0 and 4.
 * OMR_ERR_NOTIMPL, never a wrong picture: Adam7 interlace, 16-bit samples, channels = 1 from a colour or paletted stream
 * (libpng's rgb_to_gray arithmetic is not cvtColor's), an eXIf chunk with an orientation other than 1 (imread would turn
 * the image), an acTL chunk before the first IDAT (APNG).
 * OMR_ERR_BADARG, malformed structure: no signature, a chunk running past the end, IHDR missing, not first, with a size
 * of 0 or an illegal depth / type pair, an unknown critical chunk, no IDAT, IDAT chunks that are not consecutive, a
 * paletted image without PLTE, a PLTE whose length is no multiple of 3 (or that stands behind IDAT), a bad zlib header
 * (CM = 8, window <= 32 K, no FDICT, FCHECK).
 * OMR_ERR_ASSERT, damaged data (the image's content is then unspecified): a critical chunk's CRC, a missing IEND, an
 * invalid deflate code or code set, a distance before the start, input running out, a wrong Adler-32, inflated data
 * shorter or longer than the image needs, a filter byte above 4, a palette index beyond PLTE; a size above imread's own
 * limits (2^20 rows or columns, 2^30 pixels: imread fails there too), raw data of 2^32 bytes or IDAT data of 2^28 bytes
 * or more.  This refuses a little more than libpng, which warns and carries on for surplus data
 * or a wrong checksum; a refused file goes to the host codec.
 * Measured at 256 host streams a call, upload included (profiles/r19_png_decode.md): 940 dataset sheets a second from
 * 8-bit gray PNG, 608 from RGB PNG and 2568 A4 1-bit sheets, where Pillow from 16 threads of the same machine decodes 687,
 * 550 and 144.  NOT faster on long streams: 10 noise-like A4 colour cards (15 MB each) a second against Pillow's 50; one
 * wave inflates one stream, and the stage times blame inflate.  Nor from files to files: on PNG inputs
 * omr_correct_default_batch_streams corrects 292 gray dataset sheets/s where Pillow's decode on 16 threads in front of
 * omr_correct_default_batch_jpeg gives 427; it saves the raw upload and the host's cores.
 *
 * What a stream's IHDR says.  Returns 0, OMR_ERR_NOTIMPL, OMR_ERR_BADARG or OMR_ERR_ASSERT by the rules above, as far as
 * the chunk headers decide them (no CRC is computed); the fields are filled in whenever IHDR was readable (else 0).  Any
 * output pointer may be NULL.  Host only. */
int omr_png_info(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *color_type, int32_t *bit_depth);
/* n streams in HOST memory -> device-resident images, image i at d_out + i * out_stride_bytes at the top left of a slot of
 * rows x cols x channels with rows step_bytes apart; bytes of a slot outside its image are untouched.  out_size[2 i],
 * [2 i + 1] = image i's rows, cols (HOST array, the layout omr_jpeg_encode_batch_device and the batch contexts take; 0 x 0
 * where rc[i] != 0), rc[i] = 0 or the image's code by the rules above, OMR_ERR_BADARG also for an image larger than the
 * slot (HOST array).  The call itself returns 0 whatever the rc[i].  OMR_ERR_BADARG for the call: n < 0, a null pointer
 * (a null streams[i] included), channels other than 1 or 3, an empty slot, step_bytes < cols x channels,
 * out_stride_bytes < rows x step_bytes.  Every argument and every header is checked before any device work; a call all
 * of whose streams are refused does none.  Synchronous, on a stream of its own, which has drained on every return path. */
int omr_png_decode_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                uint8_t *d_out, int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                                int32_t *out_size, int32_t *rc);
/* imread of one buffer: the stream -> a packed host image of `channels` channels (release with omr_image_free). */
int omr_png_decode(const uint8_t *stream, int64_t len, int32_t channels, omr_image_owned *dst);
/* Measurement aid.  Reports what the calling thread's last PNG decode took, then switches the collection on (enable != 0)
 * or off for the thread's next ones: *groups = the groups of launches, stage_ms[0 .. 3] = device time summed over the
 * groups of the upload, inflate, Adler-32, unfilter and convert.  All zero when the collection was off.  While on, every
 * group records five events; results do not change.  Any output pointer may be NULL. */
int omr_png_decode_stats(int32_t enable, int32_t *groups, double *stage_ms);

/* ---- Bilevel TIFF decoding on the device --------------------------------------------------------
 * What sheet-fed scanners write: 1-bit TIFF, CCITT Group 4 (T.6) above all.  The result is what libtiff makes of the file,
 * byte for byte: 255 for a white pixel and 0 for a black one, replicated for 3 channels (B = G = R).
 * Streams taken: classic TIFF in either byte order, the first IFD (imread returns page 0); BitsPerSample 1 and
 * SamplesPerPixel 1 (either tag may be absent); Compression 1 (none), 32773 (PackBits) and 4 (T.6: pass, horizontal and
 * every vertical mode, make-up codes up to 2560 and their repetition, an optional EOFB); Photometric 0 and 1; FillOrder 1
 * and 2; strips with any RowsPerStrip and a short last strip, StripOffsets / StripByteCounts as SHORT or LONG, inline or
 * out of line; T6Options 0.  channels = 1 or 3 from any of them.
 * StripByteCounts may be absent (old writers): strip k then runs from its offset to the smallest strip offset greater
 * than its own, or to the stream's end where there is none, and every check on a strip holds for that length; the decoders
 * stop at the strip's rows, so the surplus is never read as codes.  A present tag is taken at its word: a wrong number of
 * counts or a count of 0 stays OMR_ERR_BADARG.  A T.6 code that begins inside its strip and ends behind it is read with
 * zeros for the missing bits, as libtiff reads it (a writer may drop a last byte that held only trailing zeros).
 * OMR_ERR_NOTIMPL, never a wrong picture: BigTIFF, tiles, any other depth, sample count, compression (3 / T.4 and, at 1
 * bit, 5 / LZW included) or photometric interpretation (a missing Photometric tag too), T6Options bit 1 (uncompressed mode), an
 * Orientation tag other than 1 (what OpenCV 4.6 does with it is not established, as for PNG's eXIf), a T.6 image wider
 * than 12288 columns (its lines' change positions live in LDS).
 * OMR_ERR_BADARG, malformed structure: a stream too short for its header, an IFD, tag value or strip outside the stream, a
 * tag of another type than SHORT or LONG, a size or RowsPerStrip of 0, an empty strip, strip counts that disagree with
 * rows / RowsPerStrip, StripOffsets missing, a Compression 1 strip shorter than its rows, a FillOrder
 * other than 1 or 2, T6Options bits other than bit 1.
 * OMR_ERR_ASSERT, damaged data (the image's content is then unspecified): an invalid or an extension code, a run past the
 * row's end or a run of 0 inside a row (T.6), a run past the strip's rows (PackBits), input that ends before the strip's
 * rows do; a size above imread's own limits (2^20 rows or columns, 2^30 pixels), a strip of 2^28 bytes or more.  This
 * refuses a little more than libtiff, which warns and carries on for some of these; a refused file goes to the host codec.
 * Two of these are chosen differences, streams libtiff reads without a warning: a run of 0 inside a T.6 row, and a PackBits
 * run that passes the strip's rows (libtiff clips it).
 * Speed: see README.md and profiles/r24_tiff_decode.md.
 *
 * 8-bit gray and RGB, what a scanner writes in its gray and colour modes.  Taken besides the above,
 * with the same rules for the file's structure: BitsPerSample 8 with SamplesPerPixel 1 and Photometric 0 or 1 (0 is
 * inverted on reading, as libtiff does); BitsPerSample 8,8,8 with SamplesPerPixel 3, Photometric 2 and
 * PlanarConfiguration 1; Compression 1, 32773 and 5 -- LZW in its TIFF 6.0 form: codes most significant bit first, Clear
 * 256, EOI 257, widths 9 to 12 with the early change; Predictor 1 and, with LZW, 2 (horizontal differencing per sample).
 * libtiff knows the Predictor tag with LZW and Deflate alone: a raw or PackBits file that carries it is read as if it did
 * not, here as there.  A gray file gives gray (channels = 1) or B = G = R (3), an RGB file gives BGR (3); a gray image
 * from an RGB file is OMR_ERR_NOTIMPL (omr_png_decode's rule).  A raw strip needs rows x cols x samples bytes.
 * An LZW strip may lack its EOI, carry bytes behind it, hold more output than its rows and Clear codes anywhere: libtiff
 * reads all of these, and so does the decoder, which stops at the strip's rows.
 * OMR_ERR_NOTIMPL besides the above: LZW at 1 bit; Deflate (8, 32946) and JPEG (6, 7) in TIFF; palette images, ExtraSamples
 * (alpha); 16 bits and every depth other than 1 and 8; PlanarConfiguration 2 with three samples; FillOrder 2 at 8 bits; a
 * Predictor other than 1 and 2 with LZW; old-style LZW (a strip that begins 00 with the low bit of its next byte set).
 * OMR_ERR_ASSERT, damaged LZW data: a strip that does not begin with Clear, a code above the next free entry, a first
 * code after Clear that is no literal, a table pushed past entry 4095, input that ends (EOI, or no room for another
 * code) before the strip's rows do; an LZW strip of 2^31 bytes of rows or more.
 * Speed: see README.md and profiles/r27_tiff8_decode.md.
 *
 * What the first IFD says.  Returns 0, OMR_ERR_NOTIMPL, OMR_ERR_BADARG or OMR_ERR_ASSERT by the rules above, as far as the
 * tags decide them; the fields are filled in as far as the tags were readable (*photometric = -1: no such tag; *strips = 0
 * unless the stream is accepted).  Any output pointer may be NULL.  Host only. */
int omr_tiff_info(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *compression, int32_t *photometric,
                  int32_t *fill_order, int32_t *strips);
/* The same with *bits_per_sample (1 or 8), *samples_per_pixel (1 or 3) and *predictor (1 or 2; 1 for every compression
 * but LZW) of an accepted stream; 1, 1, 1 for a refused one. */
int omr_tiff_info_ex(const uint8_t *stream, int64_t len, int32_t *rows, int32_t *cols, int32_t *compression, int32_t *photometric,
                     int32_t *fill_order, int32_t *strips, int32_t *bits_per_sample, int32_t *samples_per_pixel,
                     int32_t *predictor);
/* The run-length codes of ITU-T T.4 (Tables 2 and 3) as the decoder holds them, for white (black = 0) or black (1) runs:
 * OMR_TIFF_CODES entries each of run[] (0 .. 63, the make-up runs 64 .. 1728, the extended make-up runs 1792 .. 2560),
 * code[] (the code word as a number, its first bit the most significant of bits[] bits).  A test aid.  Host only. */
#define OMR_TIFF_CODES 104
int omr_tiff_code_tables(int32_t black, int32_t *run, int32_t *code, int32_t *bits);
/* The TIFF twin of omr_png_decode_batch_device: every argument, out_size, rc and the OMR_ERR_BADARG rules for the call as
 * there, rc[i] by the rules above. */
int omr_tiff_decode_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                 uint8_t *d_out, int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                                 int32_t *out_size, int32_t *rc);
/* imread of one buffer: the stream -> a packed host image of `channels` channels (release with omr_image_free). */
int omr_tiff_decode(const uint8_t *stream, int64_t len, int32_t channels, omr_image_owned *dst);
/* Measurement aid, as omr_png_decode_stats: *groups = the groups of launches, stage_ms[0 .. 3] = device time summed over
 * the groups of the upload, the PackBits kernel, the T.6 kernel, the unpack kernel.  While on, every group records five
 * events; results do not change.  Any output pointer may be NULL. */
int omr_tiff_decode_stats(int32_t enable, int32_t *groups, double *stage_ms);
/* The same for every stage: stage_ms[0 .. min(capacity, *stages) - 1] = the upload, the PackBits, T.6 and LZW kernels, the
 * unpack kernel (1 bit) and the finishing kernel (8 bits); *stages = OMR_TIFF_DECODE_STAGES.  OMR_ERR_BADARG: a negative
 * capacity, or a null stage_ms with a capacity above 0. */
#define OMR_TIFF_DECODE_STAGES 6
int omr_tiff_decode_stats_ex(int32_t enable, int32_t *groups, double *stage_ms, int32_t capacity, int32_t *stages);

/* ---- imread: EXIF orientation and the three decoders behind one door -----------------------------
 * imread(IMREAD_COLOR) -- the first line of correct_default and of TransformableMatrix::new -- turns a JPEG by the
 * orientation its EXIF block carries; phones and sheet-fed scanners write such files for every portrait capture.  The
 * codes mean what OpenCV's ExifTransform (and Pillow's ImageOps.exif_transpose) does:
 *   1 copy   2 flip left-right   3 turn by 180 degrees   4 flip top-bottom   5 transpose
 *   6 transpose, then flip left-right (90 degrees clockwise)   7 transpose, then flip both (transverse)
 *   8 transpose, then flip top-bottom (90 degrees counter-clockwise)
 * For 5..8 the result has the source's columns as its rows.  The order of the bytes inside a pixel is kept.
 *
 * n device-resident images of 1 or 3 byte channels, each turned by its own code and each of its own size, in one launch.
 * Image i lies at the top left of the slot d_src + i * src_stride_bytes of rows x cols (rows src_step_bytes apart) and is
 * written to the top left of the slot d_dst + i * dst_stride_bytes of dst_rows x dst_cols (rows dst_step_bytes apart): the
 * destination slots have a shape of their own, which the caller passes, so a batch of portrait captures needs no square
 * slots.  sizes: HOST array of 2 n entries (rows, cols of image i, the layout of the decoders' out_size), or NULL: every
 * image fills its slot; a 0 x 0 entry is skipped and leaves its slot untouched.  orient: HOST array of n codes.
 * out_size[2 i], [2 i + 1] (HOST array) = the turned image's rows, cols.  Bytes of a destination slot outside the turned
 * image are not written.  Out of place only.
 * OMR_ERR_BADARG, all before any device work: n < 0, a null pointer (sizes excepted), channels other than 1 or 3, an empty
 * slot, a step below cols x channels or a stride below rows x step on either side, an image larger than its source slot
 * or with one side 0, a code outside 1..8, a turned image that does not fit the destination slot, source and destination
 * slots whose byte ranges meet.  Synchronous, on a stream of its own, which has drained on every return path.
 * Measured (profiles/r22_orient.md) at 256 resident A4 colour images a call: 7.25 .. 7.28 ms for every code, 1.84 TB/s of
 * bytes moved, 0.23 of the 8 TB/s HBM roofline -- the transposing codes run at the speed of the copy; what binds all
 * eight is the address arithmetic per gathered byte and one dword in flight per lane, not LDS banks. */
int omr_orient_batch_device(const uint8_t *d_src, int64_t src_stride_bytes, int64_t src_step_bytes, int32_t rows, int32_t cols,
                            uint8_t *d_dst, int64_t dst_stride_bytes, int64_t dst_step_bytes, int32_t dst_rows,
                            int32_t dst_cols, int32_t channels, const int32_t *sizes, const int32_t *orient, int32_t n,
                            int32_t *out_size);
/* A host image of 1 or 3 channels turned by `orientation` (1..8) -> a packed host image (release with omr_image_free).
 * OMR_ERR_BADARG for other channel counts or codes. */
int omr_orient(const omr_image *src, int32_t orientation, omr_image_owned *dst);

#define OMR_IMREAD_IGNORE_ORIENTATION 128 /* imgcodecs::IMREAD_IGNORE_ORIENTATION: decode a JPEG as stored */
#define OMR_IMREAD_KIND_JPEG 0
#define OMR_IMREAD_KIND_PNG 1
#define OMR_IMREAD_KIND_TIFF 2
/* What imread would return for this stream.  A stream that begins with PNG's eight signature bytes is a PNG
 * (*kind = OMR_IMREAD_KIND_PNG) and goes by omr_png_info's rules, one that begins "II*\0" or "MM\0*" is a TIFF
 * (OMR_IMREAD_KIND_TIFF: omr_tiff_info's rules, *components = 1 or, for an RGB file, 3, *orientation = its Orientation tag), every other one goes
 * by omr_jpeg_info's, with one difference:
 * a JPEG whose EXIF orientation is 2..8 is accepted.  *rows, *cols: the size AFTER the turn (as stored with
 * OMR_IMREAD_IGNORE_ORIENTATION, or when the stream is refused); *components: 1 or 3 as stored (a PNG: 1 for colour types
 * 0 and 4, else 3); *orientation: the code found (1: none), whatever `flags` says.  flags: 0 or
 * OMR_IMREAD_IGNORE_ORIENTATION, anything else OMR_ERR_BADARG.  Any output pointer may be NULL.  Host only.
 * OMR_ERR_NOTIMPL, never a wrong picture: a JPEG whose orientation value is outside 1..8 (without the flag), and a PNG
 * whose eXIf chunk gives an orientation other than 1 (with or without it).  What OpenCV 4.6 does with either could not be
 * established: its EXIF reader is fed from JPEG markers, and eXIf support in its PNG reader may be later than 4.6. */
int omr_imread_info(const uint8_t *stream, int64_t len, int32_t flags, int32_t *rows, int32_t *cols, int32_t *components,
                    int32_t *orientation, int32_t *kind);
/* imread for a batch: omr_jpeg_decode_batch_device / omr_png_decode_batch_device / omr_tiff_decode_batch_device (JPEG, PNG
 * and TIFF may be mixed, told apart
 * as above; every argument, out_size, rc and the OMR_ERR_BADARG rules as theirs, plus `flags` as above), each stream by its
 * decoder's rules, except that a JPEG whose orientation is 2..8 is decoded and turned: "fits the slot" is judged on the
 * turned size, out_size holds the turned size.  Streams that need no turn are decoded straight into their slots; the
 * others into a scratch buffer, which one launch turns into their slots.  With OMR_IMREAD_IGNORE_ORIENTATION a JPEG is
 * decoded as stored. */
int omr_imread_batch_device(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels, int32_t flags,
                            uint8_t *d_out, int64_t out_stride_bytes, int64_t step_bytes, int32_t rows, int32_t cols,
                            int32_t *out_size, int32_t *rc);
/* imread of one buffer, JPEG, PNG or TIFF (bilevel, 8-bit gray or RGB): the stream -> a packed host image of `channels` channels (release with
 * omr_image_free), turned by its EXIF orientation unless `flags` says otherwise. */
int omr_imread(const uint8_t *stream, int64_t len, int32_t channels, int32_t flags, omr_image_owned *dst);

/* ---- PNG encoding on the device ---------------------------------------------------------------
 * A lossless exit for device-resident images: a valid PNG stream that every conforming decoder turns back into the image
 * byte for byte.  PNG has no canonical byte stream, so this is NOT what imwrite(.., PNG) writes byte for byte; it is
 * deterministic: the stream of an image is a function of its pixels, its shape and `compression` alone -- not of its place
 * in the batch, n, the other images, the base address, the pitch or the run.
 * channels: 1 gives colour type 0; 3 (BGR in memory) colour type 2, RGB in the file; 4 (BGRA) colour type 6, RGBA with
 * alpha kept, as imwrite does; 2: OMR_ERR_ASSERT.  Bit depth 8, not interlaced.
 * The stream: the signature, IHDR, ONE IDAT chunk, IEND, every chunk with its CRC-32 (computed on the device), no
 * ancillary chunks.  IDAT holds a zlib stream: the header 78 01 (deflate, 32 K window), deflate blocks, the Adler-32 of
 * the filtered data.  Every row takes the filter with the smallest sum of absolute values (libpng's heuristic; ties: the
 * lowest type).  The filtered data is cut into blocks of 16384 bytes; each is written as a dynamic, a fixed or a stored
 * block, whichever is shortest (ties: stored, fixed, dynamic), and every block but the last is followed by an empty
 * stored block, so blocks start on byte boundaries.
 * compression is imwrite's IMWRITE_PNG_COMPRESSION, clamped to 0 .. 9: 0 writes stored blocks only; 1 .. 9 all select the
 * one compressed method -- the levels are NOT told apart.  That method looks for matches at three distances only (1, the
 * bytes of a pixel, the same byte one row up, where that is within 32768) and parses greedily in pieces of 512 bytes.
 * **It compresses less than zlib does** where content repeats at other distances: measured (profiles/r20_png_encode.md)
 * 0.101 of the raw size on colour dataset sheets where zlib level 6 with Paeth gives 0.067, and 0.007 on thresholded A4
 * cards where imwrite's defaults give 0.005; on gray sheets and noisy cards it equals imwrite's defaults (0.121 / 0.122,
 * 0.570 / 0.571).  At 256 device-resident canvases a call it writes 17.1 k gray and 5.7 k colour dataset sheets/s and 452
 * A4 colour cards/s; Pillow at compress_level 1 on 16 threads of the same machine writes 1049, 109 and 10.
 * Sizes above imread's own limits (2^20 rows or columns, 2^30 pixels) are refused with OMR_ERR_ASSERT, and so is a size
 * whose IDAT chunk could exceed 2^31 - 1 bytes (2 + raw + 5 x blocks + 4, raw = rows x (1 + cols x channels)): offsets
 * inside one image are 32 bits wide, offsets into the batch's buffers 64.
 *
 * An upper bound of the stream's length for a rows x cols x channels image of any content at any level:
 * 43 + raw + 5 x ceil(raw / 16384) + 20 -- signature, IHDR, IDAT's frame and the zlib header; every block stored;
 * Adler-32, IDAT's CRC and IEND.  OMR_ERR_ASSERT by the rules above.  Host only. */
int omr_png_bound(int32_t rows, int32_t cols, int32_t channels, int64_t *bytes);
/* n device-resident images -> n streams.  Slots, sizes (NULL allowed, 0 x 0 entries, an image at its slot's top left),
 * d_out / out_stride_bytes (>= omr_png_bound of the slot) / out_len and the OMR_ERR_BADARG rules are exactly
 * omr_jpeg_encode_batch_device's: nothing is written at or behind out_len[i], a 0 x 0 entry leaves its slot untouched.
 * Every argument is checked before any device work.  Synchronous, on a stream of its own, which has drained on every
 * return path. */
int omr_png_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows,
                                int32_t cols, int32_t channels, const int32_t *sizes, int32_t n, int32_t compression,
                                uint8_t *d_out, int64_t out_stride_bytes, int64_t *out_len);
/* A host image -> its stream in `out` (cap bytes), *len = the stream's length.  cap too small (out may be NULL when cap
 * is 0): OMR_ERR_NOMEM with *len = the length needed, nothing written. */
int omr_png_encode(const omr_image *src, int32_t compression, uint8_t *out, int64_t cap, int64_t *len);
/* Measurement aid, as omr_png_decode_stats.  Reports what the calling thread's last PNG encode took, then switches the
 * collection on (enable != 0) or off for the thread's next ones: *groups = the groups of launches, stage_ms[0 .. 5] =
 * device time summed over the groups of the filter, Adler-32, matches and parse, code sets and placement, the bit writer,
 * and copy + CRC-32 + wrap (which includes the host's placing of the streams).  All zero when the collection was off.
 * While on, every group records seven events; results do not change.  Any output pointer may be NULL. */
int omr_png_encode_stats(int32_t enable, int32_t *groups, double *stage_ms);
/* omr_correct_default_batch_jpeg with the PNG encoder behind the batch colour warp: png[i] (malloc'ed, release with
 * omr_bytes_free) holds png_len[i] bytes that decode to sheet i's rotated canvas exactly, NULL / 0 where scan_rc[i] != 0.
 * Buckets, context cache, rotate_angle, need_check and scan_rc are the JPEG form's.  A shape whose canvas slot
 * (omr_correct_batch_canvas) omr_png_bound refuses refuses the call with OMR_ERR_ASSERT before any device work. */
int omr_correct_default_batch_png(const omr_image *srcs, int32_t n, uint16_t projection_max_angle,
                                  double projection_angle_step, int32_t projection_max_width,
                                  int32_t projection_max_height, double hough_min_line_length,
                                  double hough_max_line_gap, int32_t compression, double *rotate_angle, int32_t *need_check,
                                  int32_t *scan_rc, uint8_t **png, int64_t *png_len);
/* omr_correct_default_batch_streams (JPEG and PNG inputs, mixed) with PNG streams as its outputs. */
int omr_correct_default_batch_streams_png(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                          uint16_t projection_max_angle, double projection_angle_step,
                                          int32_t projection_max_width, int32_t projection_max_height,
                                          double hough_min_line_length, double hough_max_line_gap, int32_t compression,
                                          double *rotate_angle, int32_t *need_check, int32_t *scan_rc, uint8_t **png,
                                          int64_t *png_len);

/* ---- Group 4 TIFF encoding on the device ----------------------------------------------------------
 * The bilevel exit for device-resident images: a 1-bit TIFF, CCITT Group 4 (T.6), whose strips are byte for byte what
 * libtiff writes for the thresholded picture.  A pixel is white iff its gray value is greater than `threshold` (0 .. 254);
 * for 3 channels (BGR in memory) the gray value is omr_rgb_to_gray_batch_device's.  A 0 / 255 image -- the TIFF decoder's
 * output -- encodes to itself at any threshold.  Deterministic: the file is a function of the pixels, the shape, threshold,
 * rows_per_strip and dpi alone -- not of its place in the batch, n, the other images, the base address, the pitch or the run.
 * The file: little-endian classic TIFF, the IFD at offset 8 with its tags in ascending order -- 256 ImageWidth and 257
 * ImageLength (LONG), 258 BitsPerSample 1, 259 Compression 4, 262 Photometric 0 (WhiteIsZero: white paper is coded as
 * white runs), 273 StripOffsets (LONG), 277 SamplesPerPixel 1, 278 RowsPerStrip (LONG), 279 StripByteCounts (LONG), 282 and
 * 283 X and YResolution dpi / 1 (only when dpi > 0), 293 T6Options 0, 296 ResolutionUnit 2 (inch, only when dpi > 0) -- then
 * the resolutions, the two strip arrays (inside their entries when there is one strip), then the strips, FillOrder 1, each
 * at an even offset.  rows_per_strip = 0 means one strip; a value above the rows is taken as the rows.  Every strip is coded
 * under an imaginary white line by libtiff's rule (Fax3Encode2DRow: pass, vertical within 3, else horizontal), ends with
 * EOFB (000000000001 twice) and is padded with zeros to a byte.
 * Sizes above imread's own limits (2^20 rows or columns, 2^30 pixels) are refused with OMR_ERR_ASSERT, and so is a strip
 * that could pass 2^31 - 1 bits (rows of a strip x (7 x cols + 32) + 31): bit offsets inside a strip are 32 bits wide.
 * Speed: see README.md and profiles/r26_tiff_encode.md.
 *
 * An upper bound of the file's length for a rows x cols image of any content: 186 bytes of header, IFD and resolutions,
 * 8 a strip for the arrays, and per strip ceil((its rows x (7 x cols + 32) + 24) / 8) rounded up to even -- a row's code
 * takes at most 7 bits a pixel and 28 more (csrc/oics_tiff_enc.cpp has the argument; alternating pixels take 6 a pixel).
 * OMR_ERR_ASSERT by the rules above, OMR_ERR_BADARG for a null bytes or a negative rows_per_strip.  Host only. */
int omr_tiff_bound(int32_t rows, int32_t cols, int32_t rows_per_strip, int64_t *bytes);
/* n device-resident images -> n files.  Slots, sizes (NULL allowed, 0 x 0 entries, an image at its slot's top left),
 * d_out / out_stride_bytes (>= omr_tiff_bound of the slot) / out_len and the OMR_ERR_BADARG rules are exactly
 * omr_png_encode_batch_device's: nothing is written at or behind out_len[i], a 0 x 0 entry leaves its slot untouched.
 * Also OMR_ERR_BADARG: channels other than 1 or 3, a threshold outside 0 .. 254, a negative rows_per_strip or dpi.
 * Every argument is checked before any device work.  Synchronous, on a stream of its own, which has drained on every
 * return path. */
int omr_tiff_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows,
                                 int32_t cols, int32_t channels, const int32_t *sizes, int32_t n, int32_t threshold,
                                 int32_t rows_per_strip, int32_t dpi, uint8_t *d_out, int64_t out_stride_bytes,
                                 int64_t *out_len);
/* A host image -> its file in `out` (cap bytes), *len = the file's length.  cap too small (out may be NULL when cap is 0):
 * OMR_ERR_NOMEM with *len = the length needed, nothing written. */
int omr_tiff_encode(const omr_image *src, int32_t threshold, int32_t rows_per_strip, int32_t dpi, uint8_t *out, int64_t cap,
                    int64_t *len);
/* Measurement aid, as omr_png_encode_stats: *groups = the groups of launches, stage_ms[0 .. 3] = device time summed over
 * the groups of threshold and pack, the row coder, the placement scans, and head + bit merge (which includes the host's
 * placing of the files).  While on, every group records five events; results do not change.  Any output pointer may be
 * NULL. */
int omr_tiff_encode_stats(int32_t enable, int32_t *groups, double *stage_ms);

/* ---- 8-bit gray and RGB TIFF encoding on the device --------------------------------------------
 * The exit that keeps the gray levels: an 8-bit TIFF of 1 sample (gray) or 3 (BGR in memory, written R, G, B), uncompressed
 * (compression 1) or LZW (5), with Predictor 1, or 2 (horizontal differencing, per sample, mod 256) with LZW only.  The
 * contract is omr_png_encode's: the file is valid, it decodes to the image exactly (libtiff, omr_tiff_decode), and it is
 * deterministic -- a function of the pixels, the shape, compression, predictor, rows_per_strip and dpi alone, not of its
 * place in the batch, n, the other images, the base address, the pitch or the run.  It is NOT libtiff's byte stream.
 * The file: little-endian classic TIFF, the IFD at offset 8 with its tags in ascending order -- 256 ImageWidth and 257
 * ImageLength (LONG), 258 BitsPerSample 8 or 8,8,8, 259 Compression, 262 Photometric 1 (BlackIsZero) or 2 (RGB), 273
 * StripOffsets (LONG), 277 SamplesPerPixel, 278 RowsPerStrip (LONG), 279 StripByteCounts (LONG), 282 and 283 X and
 * YResolution dpi / 1 (only when dpi > 0), 284 PlanarConfiguration 1 (colour only), 296 ResolutionUnit 2 (only when
 * dpi > 0), 317 Predictor 2 (only then) -- then the resolutions, BitsPerSample's three values and a zero SHORT (colour),
 * the two strip arrays (inside their entries when there is one strip), then the strips, each at an even offset with a zero
 * in front where the one before is odd.  rows_per_strip = 0 means libtiff's default, the most rows whose raw strip is at
 * most 8192 bytes and at least one -- not one strip as for Group 4: the strips are coded in parallel, one strip a page is
 * one wave a page.  A value above the rows is taken as the rows.
 * An LZW strip is TIFF 6.0's: codes most significant bit first, Clear (256) first, the longest matches, EOI (257), zeros
 * to a byte; a code's width follows the count of codes since the last Clear (9 bits below 254, 10 below 766, 11 below 1790,
 * then 12: the early change).  Clear is sent when the table is full and only then: it is the code with index 3836 since
 * the last Clear (libtiff's writer's point), so no reader adds an entry above 4092.
 * Refused with OMR_ERR_ASSERT: an empty image, sizes above imread's limits (2^20 rows or columns, 2^30 pixels), a strip
 * that could pass 2^31 - 1 bits, a file that could pass 2^32 - 1 bytes.  Speed: README.md, profiles/r28_tiff8_encode.md.
 *
 * An upper bound of the file's length for any content: 206 bytes of head, 8 a strip for the arrays, and per strip of n raw
 * bytes (its rows x cols x channels), rounded up to even: n uncompressed; ceil(12 x (n + n / 3836 + 2) / 8) for LZW (every
 * code but Clear and EOI takes a byte of input or more, Clear stands in front and behind every 3836 of them, no code is
 * wider than 12 bits).  OMR_ERR_BADARG for a null bytes, channels other than 1 or 3, a compression other than 1 or 5, a
 * negative rows_per_strip.  Host only. */
int omr_tiff8_bound(int32_t rows, int32_t cols, int32_t channels, int32_t compression, int32_t rows_per_strip, int64_t *bytes);
/* n device-resident images -> n files.  Slots, sizes (NULL allowed, 0 x 0 entries, an image at its slot's top left),
 * d_out / out_stride_bytes / out_len and the OMR_ERR_BADARG rules are omr_tiff_encode_batch_device's: nothing is written at
 * or behind out_len[i], a 0 x 0 entry leaves its slot untouched.  out_stride_bytes holds omr_tiff8_bound of the slot and of
 * every image (with rows_per_strip 0 an image narrower than its slot has strips of its own).  Also OMR_ERR_BADARG: a
 * compression other than 1 or 5, a predictor other than 1 or 2, predictor 2 with compression 1, a negative dpi.  Every
 * argument is checked before any device work.  Synchronous, on a stream of its own, which has drained on every return. */
int omr_tiff8_encode_batch_device(const uint8_t *d_imgs, int64_t img_stride_bytes, int64_t step_bytes, int32_t rows,
                                  int32_t cols, int32_t channels, const int32_t *sizes, int32_t n, int32_t compression,
                                  int32_t predictor, int32_t rows_per_strip, int32_t dpi, uint8_t *d_out,
                                  int64_t out_stride_bytes, int64_t *out_len);
/* A host image -> its file in `out` (cap bytes), *len = the file's length.  cap too small (out may be NULL when cap is 0):
 * OMR_ERR_NOMEM with *len = the length needed, nothing written. */
int omr_tiff8_encode(const omr_image *src, int32_t compression, int32_t predictor, int32_t rows_per_strip, int32_t dpi,
                     uint8_t *out, int64_t cap, int64_t *len);
/* Measurement aid, as omr_tiff_encode_stats: stage_ms[0 .. 3] = staging (LZW), the LZW coder (uncompressed: the strips'
 * lengths), the placement scan, and head + strips into the file (which includes the host's placing of the files). */
int omr_tiff8_encode_stats(int32_t enable, int32_t *groups, double *stage_ms);

/* ---- deskew with projections from file contents to file contents ------------------------------
 * The reference's benchmark flow, core/src/main.rs:68-95 -- imread, get_angle_with_projections, rotate_mat of the
 * original (CONTAIN, scale 1, BORDER_CONSTANT), imwrite -- for batches: omr_deskew_with_projections_batch with the scans
 * given as baseline JPEG or PNG streams in host memory and the deskewed canvases returned as JPEG streams.  The streams
 * are told apart by PNG's signature as omr_correct_default_batch_streams does; one batch, and one bucket, may hold both
 * kinds, and each kind goes by its decoder's rules (omr_jpeg_decode_batch_device, omr_png_decode_batch_device), with the
 * one difference of omr_imread_batch_device: a JPEG whose EXIF orientation is 2..8 is decoded and turned as imread turns
 * it, and counts by its turned shape (omr_correct_default_batch_streams does not do this yet and answers -213).  The
 * headers are parsed and the scans bucketed by shape on the host; each bucket is decoded straight into the scan slots of
 * the cached omr_projection_batch context, swept, warped by the winners on the device and encoded there, in runs of 32
 * scans (256 when no outputs are asked for), so only streams cross the link in either direction.
 * channels: 3 is imread(IMREAD_COLOR) -- a gray stream gives B = G = R -- and a 3-component output; 1 is the gray
 * convenience of omr_get_angle_with_projections: the Y plane of a JPEG, colour types 0 and 4 of a PNG (OMR_ERR_NOTIMPL in
 * scan_rc[i] for the others), a single-component JPEG or a colour-type-0 PNG out.  Anything else: OMR_ERR_BADARG.
 * For every scan with scan_rc[i] == 0: angles[i] has the f64 bits of omr_get_angle_with_projections on imread's decode
 * of the stream, best_idx[i] (may be NULL) its candidate, and jpeg[i] (malloc'ed, release with omr_bytes_free; jpeg_len[i]
 * bytes) is byte for byte omr_jpeg_encode(omr_rotate(decode, angles[i], 1.0, interp, border_value, OMR_CLIP_CONTAIN),
 * quality).  A scan's result does not depend on its place in the batch, on n or on the other scans.
 * A scan whose header its decoder refuses or finds malformed gets that code in scan_rc[i], angle 0, best_idx -1 and no
 * output, on the host, before any device work; one whose image data turns out damaged gets OMR_ERR_ASSERT there; one for
 * which the per-call function would fail (a working size that truncates to 0) that code.  The other scans are unaffected
 * and the call returns 0; a call whose every stream is refused does no device work.
 * jpeg and jpeg_len may both be NULL: the angles-only form (get_angle_with_projections from files), which allocates no
 * canvas slot.
 * OMR_ERR_BADARG for the call: a null streams / len / angles / scan_rc / streams[i], n < 1, a negative length, exactly one
 * of jpeg and jpeg_len null, a null border_value when outputs are wanted, an empty candidate range, a resize_scale that is
 * <= 0 or not finite.  OMR_ERR_NOTIMPL: interp other than NEAREST / LINEAR.  OMR_ERR_ASSERT, before any device work: a
 * shape whose deskew canvas (omr_projection_batch_deskew_canvas) could take more than 2^32 bits of scan data.  On an
 * error of the whole call nothing is returned and nothing is left allocated.
 * A bucket the batch context does not take (a sweep it cannot plan, a canvas the warp's tables cannot hold) goes scan by
 * scan through omr_jpeg_decode / omr_png_decode, omr_get_angle_with_projections, omr_rotate and omr_jpeg_encode, so every
 * scan that chain accepts is accepted here, with the same bytes.
 * Measured (profiles/r21_projection_streams.md) at (45, 0.2, 0.2), LINEAR, quality 100: 5.5 k dataset sheets/s from gray
 * JPEG at 256 files a call (6.3 k with channels = 1), 332 / 432 A4 colour cards/s from JPEG at quality 100 / 95 at 64 files a
 * call.  The per-call pair omr_get_angle_with_projections + omr_rotate from 16 threads with Pillow on both ends gives 76
 * and 10 / 10 (73 x, 32 x / 42 x), Pillow's decode + omr_deskew_with_projections_batch + Pillow's save 71 and 9 / 9; both
 * are bound by Pillow's quality-100 save, whose threads encode no faster than one.  The decode is 106 of 119 ms of a chunk
 * of 32 A4 cards.  NOT faster from RGB PNG: 77 dataset sheets/s against 76 and 69 (1.0 x, 1.1 x) -- one wave inflates one
 * stream and a run carries 32 scans, so at most 32 waves inflate at a time. */
int omr_deskew_with_projections_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                              uint16_t max_angle, double step, double resize_scale, int32_t interp,
                                              const uint8_t border_value[4], int32_t quality, double *angles,
                                              int32_t *best_idx, int32_t *scan_rc, uint8_t **jpeg, int64_t *jpeg_len);
/* The same with PNG streams as its outputs (omr_png_encode's, for `compression`): png[i] decodes to the deskewed canvas
 * exactly.  The call-level OMR_ERR_ASSERT is omr_png_bound's refusal of the canvas. */
int omr_deskew_with_projections_batch_streams_png(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                                  int32_t channels, uint16_t max_angle, double step, double resize_scale,
                                                  int32_t interp, const uint8_t border_value[4], int32_t compression,
                                                  double *angles, int32_t *best_idx, int32_t *scan_rc, uint8_t **png,
                                                  int64_t *png_len);
/* The same with Group 4 TIFF files as its outputs: tiff[i] is byte for byte omr_tiff_encode(canvas, threshold,
 * rows_per_strip, dpi) of the deskewed canvas.  OMR_ERR_BADARG for the call also: a threshold outside 0 .. 254, a negative
 * rows_per_strip or dpi.  The call-level OMR_ERR_ASSERT is omr_tiff_bound's refusal of the canvas. */
int omr_deskew_with_projections_batch_streams_tiff(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                                   int32_t channels, uint16_t max_angle, double step, double resize_scale,
                                                   int32_t interp, const uint8_t border_value[4], int32_t threshold,
                                                   int32_t rows_per_strip, int32_t dpi, double *angles, int32_t *best_idx,
                                                   int32_t *scan_rc, uint8_t **tiff, int64_t *tiff_len);
/* The same with 8-bit TIFF files as its outputs: tiff[i] is byte for byte omr_tiff8_encode(canvas, compression, predictor,
 * rows_per_strip, dpi) of the deskewed canvas, gray or colour as `channels` says.  OMR_ERR_BADARG for the call also:
 * omr_tiff8_encode_batch_device's parameter rules.  The call-level OMR_ERR_ASSERT is omr_tiff8_bound's refusal of the canvas. */
int omr_deskew_with_projections_batch_streams_tiff8(const uint8_t *const *streams, const int64_t *len, int32_t n,
                                                    int32_t channels, uint16_t max_angle, double step, double resize_scale,
                                                    int32_t interp, const uint8_t border_value[4], int32_t compression,
                                                    int32_t predictor, int32_t rows_per_strip, int32_t dpi, double *angles,
                                                    int32_t *best_idx, int32_t *scan_rc, uint8_t **tiff, int64_t *tiff_len);

/* ---- deskew with the Hough and FFT detectors for batches ----------------------------------------
 * The other two legs of the reference's benchmark, core/src/main.rs:96-170: get_angle_with_hough / get_angle_with_fft on
 * transfer_rgb_image_to_gray_image(original), then rotate_mat of the ORIGINAL by that angle, then im_write -- with the same
 * three doors the projection leg has (device memory, host images, file contents).  Every stage is an existing one, run as
 * it is: omr_rgb_to_gray_batch_device into the library's scratch for 3-channel scans (1-channel scans are the detector's
 * input as they are), omr_hough_angles_batch_device (channels = 1) or omr_fft_angles_batch_device, omr_rotate_batch_device_ex
 * on the originals.  channels is 1 or 3 (4: OMR_ERR_NOTIMPL, anything else OMR_ERR_ASSERT).
 * For every scan i: angles[i] has the f64 bits of omr_get_angle_with_hough / omr_get_angle_with_fft on omr_rgb_to_gray of the
 * scan, and canvas i is byte for byte omr_rotate_device_ex(scan i, angles[i], 1.0, flags, border_mode, border_value, clip).
 * A scan in which the Hough detector finds no segment keeps omr_hough_angles_batch_device's rule -- rc[i] = OMR_ERR_ASSERT,
 * angles[i] = 0.0 -- and has no canvas: its out_size is 0 x 0 and its slot is NOT written; the call still returns 0 and the
 * other scans are unaffected.  The FFT detector gives such a scan the angle 0.0 and succeeds (fft.rs:197-247): rc[i] is
 * always 0 there, and rc may be NULL.
 *
 * omr_detector_deskew_canvas (host only): the slot every canvas fits.  The detectors' angles are not bounded, so for
 * OMR_CLIP_CONTAIN this is the worst case over all angles, the diagonal rounded up, for rows and cols alike (one more where
 * the diagonal is a whole number, which rounding can exceed); rows x cols for OMR_CLIP_DEFAULT.  OMR_ERR_ASSERT: an empty
 * image, a side or a slot of 32767 or more; OMR_ERR_BADARG: a null output, an unknown clip.
 *
 * omr_hough_deskew_batch_device / omr_fft_deskew_batch_device: n device-resident scans of one shape, scan i at d_scans +
 * i * scan_stride_bytes, rows step_bytes apart; canvas i at the top left of the slot d_out + i * out_stride_bytes, rows
 * out_step_bytes apart, its (rows, cols) in the HOST array out_size at [2i], [2i + 1]; the slot's bytes outside the canvas
 * are not written.  angles / rc / n_lines (may be NULL) / out_size: HOST arrays of n.  The argument rules are the union of the
 * detector's and of omr_rotate_batch_device_ex's, with the slot that of omr_detector_deskew_canvas: OMR_ERR_BADARG for a null
 * d_scans / d_out / border_value / out_size / angles (/ rc for Hough), n <= 0, step_bytes < cols * channels, a negative scan
 * stride, unknown flag bits, border mode or clip, out_step_bytes < channels * max_cols, out_stride_bytes < max_rows *
 * out_step_bytes, source and destination ranges that overlap; OMR_ERR_NOTIMPL for interpolation 5..7; OMR_ERR_ASSERT for
 * an empty or oversized image.  All are checked before any device work, and a refused call writes nothing.  Enqueues on
 * `stream` and SYNCHRONISES it before it returns, as the detectors do. */
int omr_detector_deskew_canvas(int32_t rows, int32_t cols, int32_t clip, int32_t *max_rows, int32_t *max_cols);
int omr_hough_deskew_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows, int32_t cols,
                                  int32_t channels, int64_t step_bytes, double min_line_length, double max_line_gap,
                                  int32_t flags, int32_t border_mode, const uint8_t border_value[4], int32_t clip,
                                  uint8_t *d_out, int64_t out_stride_bytes, int64_t out_step_bytes, int32_t *out_size,
                                  double *angles, int32_t *rc, int32_t *n_lines, void *stream);
int omr_fft_deskew_batch_device(const uint8_t *d_scans, int32_t n, int64_t scan_stride_bytes, int32_t rows, int32_t cols,
                                int32_t channels, int64_t step_bytes, double canny_threshold_1, double canny_threshold_2,
                                double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                                const uint8_t border_value[4], int32_t clip, uint8_t *d_out, int64_t out_stride_bytes,
                                int64_t out_step_bytes, int32_t *out_size, double *angles, int32_t *rc, int32_t *n_lines,
                                void *stream);
/* The same for host images of any mix of shapes, 1 or 3 channels each, bucketed by (rows, cols, channels) as
 * omr_deskew_with_projections_batch does, on the current device, up to 32 scans of a shape a run (scan and slot of an A4
 * colour sheet are 26 + 55 MB on the device).  angles[i] / rc[i] / rotated[i] belong to srcs[i]; rotated[i] is an owned
 * image (omr_image_free), what omr_rotate_ex gives for srcs[i] and angles[i] (BORDER_TRANSPARENT starts from zeros, as
 * there), or has .data == NULL where rc[i] != 0.  rc may be NULL in the FFT form.  Every image is checked before any
 * device work and an invalid one fails the whole call: nothing is written and no image is returned. */
int omr_deskew_with_hough_batch(const omr_image *srcs, int32_t n, double min_line_length, double max_line_gap, int32_t flags,
                                int32_t border_mode, const uint8_t border_value[4], int32_t clip, double *angles, int32_t *rc,
                                omr_image_owned *rotated);
int omr_deskew_with_fft_batch(const omr_image *srcs, int32_t n, double canny_threshold_1, double canny_threshold_2,
                              double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                              const uint8_t border_value[4], int32_t clip, double *angles, int32_t *rc,
                              omr_image_owned *rotated);
/* ... and from file contents to file contents: the streams are baseline JPEG or PNG files, mixed, and go through the imread
 * layer exactly as in omr_deskew_with_projections_batch_streams (headers parsed and scans bucketed by shape on the host,
 * an EXIF-tagged JPEG turned and bucketed by its turned shape, decoded on the device straight into the scan slots); the
 * canvases are encoded on the device, so only streams cross the link.  channels: 3 is imread(IMREAD_COLOR), 1 the gray
 * form, as there.  format 0: out[i] is byte for byte omr_jpeg_encode(canvas, quality_or_compression); format 1:
 * omr_png_encode's stream for that compression level, which decodes to the canvas exactly.  out[i] is malloc'ed (release
 * with omr_bytes_free), out_len[i] bytes long.  A scan whose header its decoder refuses or finds malformed gets that code
 * in scan_rc[i], angle 0 and no output, before any device work; one whose image data turns out damaged gets OMR_ERR_ASSERT
 * there, as does one in which the Hough detector finds no segment, and one whose canvas slot would leave the image limit.
 * The other scans are unaffected and the call returns 0.  out and out_len may both be NULL: the angles alone, no canvas
 * is made.  OMR_ERR_BADARG for the call: a null streams / len / angles / scan_rc / streams[i], n < 1, a negative length,
 * exactly one of out and out_len null, a null border_value when outputs are wanted, channels other than 1 or 3, a format
 * other than 0 or 1, unknown flag bits, border mode or clip.  OMR_ERR_NOTIMPL: interpolation 5..7.  OMR_ERR_ASSERT, before
 * any device work: a shape whose canvas slot the encoder cannot take (omr_jpeg_bound / omr_png_bound's refusal).  On an
 * error of the whole call nothing is returned and nothing is left allocated. */
int omr_deskew_with_hough_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                        double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                                        const uint8_t border_value[4], int32_t clip, int32_t format,
                                        int32_t quality_or_compression, double *angles, int32_t *scan_rc, uint8_t **out,
                                        int64_t *out_len);
int omr_deskew_with_fft_batch_streams(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                      double canny_threshold_1, double canny_threshold_2, double min_line_length,
                                      double max_line_gap, int32_t flags, int32_t border_mode, const uint8_t border_value[4],
                                      int32_t clip, int32_t format, int32_t quality_or_compression, double *angles,
                                      int32_t *scan_rc, uint8_t **out, int64_t *out_len);
/* The two with Group 4 TIFF files as their outputs (the format argument above keeps refusing any value but 0 and 1):
 * out[i] is byte for byte omr_tiff_encode(canvas, threshold, rows_per_strip, dpi).  Everything else as above; OMR_ERR_BADARG
 * for the call also: a threshold outside 0 .. 254, a negative rows_per_strip or dpi; the call-level OMR_ERR_ASSERT is
 * omr_tiff_bound's refusal of the canvas slot. */
int omr_deskew_with_hough_batch_streams_tiff(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                             double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                                             const uint8_t border_value[4], int32_t clip, int32_t threshold,
                                             int32_t rows_per_strip, int32_t dpi, double *angles, int32_t *scan_rc,
                                             uint8_t **out, int64_t *out_len);
int omr_deskew_with_fft_batch_streams_tiff(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                           double canny_threshold_1, double canny_threshold_2, double min_line_length,
                                           double max_line_gap, int32_t flags, int32_t border_mode,
                                           const uint8_t border_value[4], int32_t clip, int32_t threshold,
                                           int32_t rows_per_strip, int32_t dpi, double *angles, int32_t *scan_rc,
                                           uint8_t **out, int64_t *out_len);
/* The two with 8-bit TIFF files as their outputs: out[i] is byte for byte omr_tiff8_encode(canvas, compression, predictor,
 * rows_per_strip, dpi).  Everything else as above; OMR_ERR_BADARG for the call also: omr_tiff8_encode_batch_device's
 * parameter rules; the call-level OMR_ERR_ASSERT is omr_tiff8_bound's refusal of the canvas slot. */
int omr_deskew_with_hough_batch_streams_tiff8(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                              double min_line_length, double max_line_gap, int32_t flags, int32_t border_mode,
                                              const uint8_t border_value[4], int32_t clip, int32_t compression,
                                              int32_t predictor, int32_t rows_per_strip, int32_t dpi, double *angles,
                                              int32_t *scan_rc, uint8_t **out, int64_t *out_len);
int omr_deskew_with_fft_batch_streams_tiff8(const uint8_t *const *streams, const int64_t *len, int32_t n, int32_t channels,
                                            double canny_threshold_1, double canny_threshold_2, double min_line_length,
                                            double max_line_gap, int32_t flags, int32_t border_mode,
                                            const uint8_t border_value[4], int32_t clip, int32_t compression,
                                            int32_t predictor, int32_t rows_per_strip, int32_t dpi, double *angles,
                                            int32_t *scan_rc, uint8_t **out, int64_t *out_len);

/* calculate::get_arithmetic_mean / get_standard_deviation (calculate.rs:2-10, :13-23) */
int omr_get_arithmetic_mean(const double *v, size_t n, double *out);
int omr_get_standard_deviation(const double *v, size_t n, double *out);

#ifdef __cplusplus
}
#endif
#endif
