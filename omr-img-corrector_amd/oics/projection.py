"""oics::projection (packages/lib/src/projection.rs) through the C ABI."""
import ctypes as C

import numpy as np

from ._lib import check, f64p, i32p, lib, u32p
from .transfer import _mat, _take_owned, as_image


def get_angle_with_projections(src_img, max_angle, step, resize_scale, threads):
    """projection.rs:17-23: (&TransformableMatrix, u16, f64, f64, usize) -> f64"""
    a, im = as_image(_mat(src_img))
    out = C.c_double()
    check(lib().omr_get_angle_with_projections(C.byref(im), int(max_angle), float(step), float(resize_scale),
                                               int(threads), C.byref(out)))
    return out.value


def get_angles_with_projections(srcs, max_angle, step, resize_scale, want_idx=False):
    """get_angle_with_projections for a batch (omr_get_angles_with_projections_batch): host images of any mix of shapes,
    angles[i] belongs to srcs[i] and is the per-call function's answer, same f64 bits.  want_idx: (angles, best_idx)."""
    from ._lib import OmrImage
    keep, arr = [], (OmrImage * max(len(srcs), 1))()
    for i, s in enumerate(srcs):
        a, im = as_image(_mat(s))
        keep.append(a)
        arr[i] = im
    n = len(srcs)
    ang = np.zeros(max(n, 1), np.float64)
    idx = np.zeros(max(n, 1), np.int32)
    check(lib().omr_get_angles_with_projections_batch(arr, n, int(max_angle), float(step), float(resize_scale),
                                                      ang.ctypes.data_as(f64p), idx.ctypes.data_as(i32p) if want_idx else None))
    return (ang[:n], idx[:n]) if want_idx else ang[:n]


def _border4(border):
    bv = [int(border)] * 4 if isinstance(border, int) else [int(v) for v in border] + [0] * (4 - len(border))
    return (C.c_uint8 * 4)(*bv[:4])


def get_angles_and_deskew(srcs, max_angle, step, resize_scale, interp=1, border=(255, 255, 255), want_idx=False):
    """The reference benchmark's flow for a batch (omr_deskew_with_projections_batch; core/src/main.rs:68-95):
    get_angle_with_projections on every image, then rotate_mat of the full-size image by its angle (CONTAIN, scale 1,
    constant border; interp 0 = NEAREST, 1 = LINEAR).  Host images of any mix of shapes.  Returns (angles, images):
    angles[i] is the per-call angle of srcs[i] (same f64 bits), images[i] the array transfer.rotate_mat gives for it.
    want_idx: (angles, best_idx, images)."""
    from ._lib import OmrImage, OmrImageOwned
    keep, arr = [], (OmrImage * max(len(srcs), 1))()
    for i, s in enumerate(srcs):
        a, im = as_image(_mat(s))
        keep.append(a)
        arr[i] = im
    n = len(srcs)
    ang = np.zeros(max(n, 1), np.float64)
    idx = np.zeros(max(n, 1), np.int32)
    owned = (OmrImageOwned * max(n, 1))()
    check(lib().omr_deskew_with_projections_batch(arr, n, int(max_angle), float(step), float(resize_scale), int(interp),
                                                  _border4(border), ang.ctypes.data_as(f64p), idx.ctypes.data_as(i32p), owned))
    images = [_take_owned(owned[i]) for i in range(n)]
    return (ang[:n], idx[:n], images) if want_idx else (ang[:n], images)


def _deskew_streams(streams, max_angle, step, resize_scale, interp, border, level, channels, png, want_out, tiff=None,
                    tiff8=None):
    """omr_deskew_with_projections_batch_streams / _png / _tiff (tiff = (rows_per_strip, dpi), level = the threshold) /
    _tiff8 (tiff8 = (predictor, rows_per_strip, dpi), level = the compression) ->
    (angles, best_idx, scan_rc, [bytes or None] or None)"""
    from ._lib import u8p
    bufs = [np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray, memoryview)) else np.ascontiguousarray(s, np.uint8)
            for s in streams]
    bufs = [b if b.size else np.zeros(1, np.uint8) for b in bufs]
    n = len(bufs)
    sp = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    sl = np.array([len(s) for s in streams] + [0], np.int64)
    ang = np.zeros(max(n, 1), np.float64)
    idx = np.zeros(max(n, 1), np.int32)
    rc = np.zeros(max(n, 1), np.int32)
    ptrs = (u8p * max(n, 1))()
    lens = np.zeros(max(n, 1), np.int64)
    fn = lib().omr_deskew_with_projections_batch_streams_png if png else lib().omr_deskew_with_projections_batch_streams
    how = (int(level),)
    if tiff is not None:
        fn, how = lib().omr_deskew_with_projections_batch_streams_tiff, (int(level), int(tiff[0]), int(tiff[1]))
    if tiff8 is not None:
        fn, how = lib().omr_deskew_with_projections_batch_streams_tiff8, (int(level),) + tuple(int(v) for v in tiff8)
    check(fn(sp, sl.ctypes.data_as(C.POINTER(C.c_int64)), n, int(channels), int(max_angle), float(step), float(resize_scale),
             int(interp), _border4(border), *how, ang.ctypes.data_as(f64p), idx.ctypes.data_as(i32p),
             rc.ctypes.data_as(i32p), ptrs if want_out else None,
             lens.ctypes.data_as(C.POINTER(C.c_int64)) if want_out else None))
    out = None
    if want_out:
        out = [None] * n
        for i in range(n):
            if ptrs[i]:
                out[i] = C.string_at(ptrs[i], int(lens[i]))
                lib().omr_bytes_free(ptrs[i])
    return ang[:n], idx[:n], rc[:n], out


def deskew_streams(streams, max_angle, step, resize_scale, interp=1, border=(255, 255, 255), quality=100, channels=3,
                   png=False, want_idx=False):
    """The reference benchmark's flow from file contents to file contents (omr_deskew_with_projections_batch_streams,
    png=True: _streams_png; core/src/main.rs:68-95).  streams: baseline JPEG or PNG file contents (bytes or uint8 arrays,
    both kinds in one batch), decoded, swept, rotated (CONTAIN, scale 1, constant border; interp 0 = NEAREST, 1 = LINEAR)
    and encoded on the device; `quality` is the PNG form's compression level.  channels: 3 as imread(IMREAD_COLOR), or 1
    for gray.  Returns (angles, scan_rc, outputs): angles[i] is the per-call angle of imread's decode of streams[i] (same
    f64 bits), scan_rc[i] 0 or the code of a sheet that was refused or damaged, outputs[i] the encoded canvas as bytes
    (None where scan_rc[i] != 0).  want_idx: (angles, best_idx, scan_rc, outputs)."""
    ang, idx, rc, out = _deskew_streams(streams, max_angle, step, resize_scale, interp, border, quality, channels, png, True)
    return (ang, idx, rc, out) if want_idx else (ang, rc, out)


def deskew_streams_tiff(streams, max_angle, step, resize_scale, interp=1, border=(255, 255, 255), threshold=127,
                        rows_per_strip=0, dpi=0, channels=3, want_idx=False):
    """deskew_streams with Group 4 TIFF files as its outputs (omr_deskew_with_projections_batch_streams_tiff): outputs[i]
    is oics.tiff.encode(canvas, threshold, rows_per_strip, dpi) of the deskewed canvas, byte for byte."""
    ang, idx, rc, out = _deskew_streams(streams, max_angle, step, resize_scale, interp, border, threshold, channels, False, True,
                                        tiff=(rows_per_strip, dpi))
    return (ang, idx, rc, out) if want_idx else (ang, rc, out)


def deskew_streams_tiff8(streams, max_angle, step, resize_scale, interp=1, border=(255, 255, 255), compression=5, predictor=1,
                         rows_per_strip=0, dpi=0, channels=3, want_idx=False):
    """deskew_streams with 8-bit TIFF files as its outputs (omr_deskew_with_projections_batch_streams_tiff8): outputs[i] is
    oics.tiff.encode8(canvas, compression, predictor, rows_per_strip, dpi) of the deskewed canvas, byte for byte -- gray
    for channels = 1, RGB for 3, the gray levels kept."""
    ang, idx, rc, out = _deskew_streams(streams, max_angle, step, resize_scale, interp, border, compression, channels, False, True,
                                        tiff8=(predictor, rows_per_strip, dpi))
    return (ang, idx, rc, out) if want_idx else (ang, rc, out)


def get_angles_from_streams(streams, max_angle, step, resize_scale, channels=3, want_idx=False):
    """deskew_streams' angles alone (get_angle_with_projections from files): no canvas is made.  Returns (angles,
    scan_rc); want_idx: (angles, best_idx, scan_rc)."""
    ang, idx, rc, _ = _deskew_streams(streams, max_angle, step, resize_scale, 1, (255, 255, 255), 100, channels, False, False)
    return (ang, idx, rc) if want_idx else (ang, rc)


def projection_batch_working_size(rows, cols, resize_scale):
    """(wrows, wcols, front mode): scale_self's size (transfer.rs:66-91) and how the batch front end gets there"""
    r, c, m = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().omr_projection_batch_working_size(rows, cols, float(resize_scale), C.byref(r), C.byref(c), C.byref(m)))
    return r.value, c.value, m.value


class ProjectionBatch:
    """omr_projection_batch_*: get_angle_with_projections with its resize_scale for n device-resident scans of one shape."""

    def __init__(self, rows, cols, channels, max_angle, step, resize_scale, max_scans, device=0):
        self.handle = C.c_void_p()
        check(lib().omr_projection_batch_create(rows, cols, channels, int(max_angle), float(step), float(resize_scale), device,
                                                int(max_scans), C.byref(self.handle)))
        self.rows, self.cols, self.channels = rows, cols, channels
        self.wrows, self.wcols, self.front_mode, self.A = self.info()

    def info(self):
        """(working rows, working cols, front mode OMR_PROJECTION_FRONT_*, candidates)"""
        r, c, m, a = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().omr_projection_batch_info(self.handle, C.byref(r), C.byref(c), C.byref(m), C.byref(a)))
        return r.value, c.value, m.value, a.value

    def front_device(self, d_scans, scan_stride, step_bytes, n, d_small, small_stride, small_step):
        """the front end alone: scan i's working image to d_small + i * small_stride (tests, inspection)"""
        check(lib().omr_projection_batch_front_device(self.handle, d_scans, scan_stride, step_bytes, n, d_small, small_stride,
                                                      small_step))

    def run_device(self, d_scans, scan_stride, step_bytes, n, want_sd=False):
        """(angles, best_idx, v_sd, h_sd) of n scans at d_scans + i * scan_stride; the scores only when asked for"""
        ang, idx = np.zeros(n, np.float64), np.zeros(n, np.int32)
        vs = np.zeros((n, self.A)) if want_sd else None
        hs = np.zeros((n, self.A)) if want_sd else None
        check(lib().omr_projection_batch_run_device(self.handle, d_scans, scan_stride, step_bytes, n, ang.ctypes.data_as(f64p),
                                                    idx.ctypes.data_as(i32p), vs.ctypes.data_as(f64p) if want_sd else None,
                                                    hs.ctypes.data_as(f64p) if want_sd else None))
        return ang, idx, vs, hs

    def deskew_canvas(self):
        """(rows, cols) every output slot of deskew_device must hold: the largest CONTAIN canvas of the candidates at the
        full shape (no device call)"""
        r, c = C.c_int32(), C.c_int32()
        check(lib().omr_projection_batch_deskew_canvas(self.handle, C.byref(r), C.byref(c)))
        return r.value, c.value

    def deskew_device(self, d_scans, scan_stride, step_bytes, n, interp, border, d_out, out_stride, out_step):
        """run_device, then every full-size scan warped by its own winner into d_out + i * out_stride:
        (angles, best_idx, out_size [n, 2] = rows, cols of canvas i)"""
        ang, idx, size = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros((n, 2), np.int32)
        check(lib().omr_projection_batch_deskew_device(self.handle, d_scans, scan_stride, step_bytes, n, int(interp), _border4(border),
                                                       d_out, out_stride, out_step, size.ctypes.data_as(i32p),
                                                       ang.ctypes.data_as(f64p), idx.ctypes.data_as(i32p)))
        return ang, idx, size

    def close(self):
        if self.handle:
            lib().omr_projection_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:  # at interpreter shutdown the module globals may already be gone
            self.close()
        except Exception:  # noqa: BLE001
            pass


def find_target_angle(max_angle, step, thresh, threads):
    """app/src-tauri/src/test.rs:83-178"""
    a, im = as_image(_mat(thresh))
    out = C.c_double()
    check(lib().omr_find_target_angle(int(max_angle), float(step), C.byref(im), int(threads), C.byref(out)))
    return out.value


def candidate_count(max_angle, step):
    n = C.c_int32()
    A = lib().omr_candidate_count(int(max_angle), float(step), C.byref(n))
    return n.value, A


def sweep_matrices(rows, cols, max_angle, step, scale=1.0):
    _, A = candidate_count(max_angle, step)
    M = np.zeros((max(A, 1), 6), np.float64)
    check(lib().omr_sweep_matrices(rows, cols, int(max_angle), float(step), float(scale), M.ctypes.data_as(f64p), A))
    return M[:A]


def projection_sweep(bin_img, fwd_M, want_proj=True):
    """The hot loop (projection.rs:47-65 / omr.rs:153-180) for explicit matrices, host buffers."""
    a, im = as_image(_mat(bin_img))
    M = np.ascontiguousarray(fwd_M, np.float64).reshape(-1, 6)
    A = M.shape[0]
    vp = np.zeros((A, im.cols), np.uint32) if want_proj else None
    hp = np.zeros((A, im.rows), np.uint32) if want_proj else None
    vs, hs = np.zeros(A), np.zeros(A)
    check(lib().omr_projection_sweep(C.byref(im), M.ctypes.data_as(f64p), A,
                                     vp.ctypes.data_as(u32p) if want_proj else None,
                                     hp.ctypes.data_as(u32p) if want_proj else None,
                                     vs.ctypes.data_as(f64p), hs.ctypes.data_as(f64p)))
    return vp, hp, vs, hs


def argmax_projection(v_sd, h_sd):
    v = np.ascontiguousarray(v_sd, np.float64)
    h = np.ascontiguousarray(h_sd, np.float64)
    idx = C.c_int32()
    check(lib().omr_argmax_projection(v.ctypes.data_as(f64p), h.ctypes.data_as(f64p), v.size, C.byref(idx)))
    return idx.value


class SweepPlan:
    """Resident form (omr_sweep_plan_*): tables and scratch live on the device across scans."""

    def __init__(self, rows, cols, max_angle=None, step=None, scale=1.0, matrices=None, device=0):
        self.handle = C.c_void_p()
        self.rows, self.cols = rows, cols
        if matrices is not None:
            M = np.ascontiguousarray(matrices, np.float64).reshape(-1, 6)
            check(lib().omr_sweep_plan_create(rows, cols, M.ctypes.data_as(f64p), M.shape[0], device,
                                              C.byref(self.handle)))
        else:
            check(lib().omr_sweep_plan_create_angles(rows, cols, int(max_angle), float(step), float(scale), device,
                                                     C.byref(self.handle)))
        self.A = lib().omr_sweep_plan_candidates(self.handle)

    def close(self):
        if self.handle:
            lib().omr_sweep_plan_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:  # at interpreter shutdown the module globals may already be gone
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def set_kernel(self, which):
        check(lib().omr_sweep_plan_set_kernel(self.handle, which))

    def set_timing(self, on):
        check(lib().omr_sweep_plan_set_timing(self.handle, 1 if on else 0))

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib().omr_sweep_plan_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value

    def info(self):
        """(candidates on the run-merging kernel, candidates on the gather kernels)"""
        r, g = C.c_int32(), C.c_int32()
        check(lib().omr_sweep_plan_info(self.handle, C.byref(r), C.byref(g)))
        return r.value, g.value

    def tables(self, a):
        ad, bd = np.zeros(self.cols, np.int32), np.zeros(self.cols, np.int32)
        X0, Y0 = np.zeros(self.rows, np.int32), np.zeros(self.rows, np.int32)
        check(lib().omr_sweep_plan_tables(self.handle, a, ad.ctypes.data_as(i32p), bd.ctypes.data_as(i32p),
                                          X0.ctypes.data_as(i32p), Y0.ctypes.data_as(i32p)))
        return ad, bd, X0, Y0

    def run(self, img, black_max=0, want_proj=True):
        a, im = as_image(_mat(img))
        vp = np.zeros((self.A, self.cols), np.uint32) if want_proj else None
        hp = np.zeros((self.A, self.rows), np.uint32) if want_proj else None
        vs, hs = np.zeros(self.A), np.zeros(self.A)
        best = C.c_int32()
        check(lib().omr_sweep_plan_run(self.handle, C.byref(im), black_max,
                                       vp.ctypes.data_as(u32p) if want_proj else None,
                                       hp.ctypes.data_as(u32p) if want_proj else None,
                                       vs.ctypes.data_as(f64p), hs.ctypes.data_as(f64p), C.byref(best)))
        return vp, hp, vs, hs, best.value

    def run_device(self, d_img_ptr, step_bytes, black_max, stream, d_vproj, d_hproj, d_v_sd, d_h_sd, d_best):
        check(lib().omr_sweep_plan_run_device(self.handle, d_img_ptr, step_bytes, black_max, stream, d_vproj, d_hproj,
                                              d_v_sd, d_h_sd, d_best))


class Batch:
    """omr_batch_*: n device-resident scans of one shape, round-robin over internal streams."""

    def __init__(self, rows, cols, max_angle, step, scale=1.0, device=0, n_streams=2):
        self.handle = C.c_void_p()
        check(lib().omr_batch_create(rows, cols, int(max_angle), float(step), float(scale), device, n_streams,
                                     C.byref(self.handle)))
        self.N, self.A = candidate_count(max_angle, step)
        self.step = step

    def close(self):
        if self.handle:
            lib().omr_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:  # at interpreter shutdown the module globals may already be gone
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def run_device(self, d_scans, scan_stride, step_bytes, n, black_max, d_best, d_v_sd=None, d_h_sd=None):
        check(lib().omr_batch_run_device(self.handle, d_scans, scan_stride, step_bytes, n, black_max, d_best, d_v_sd,
                                         d_h_sd))

    def deskew_canvas(self):
        """(rows, cols) every output slot of deskew_device must hold: the largest CONTAIN canvas of the candidates"""
        r, c = C.c_int32(), C.c_int32()
        check(lib().omr_batch_deskew_canvas(self.handle, C.byref(r), C.byref(c)))
        return r.value, c.value

    def deskew_device(self, d_scans, scan_stride, step_bytes, n, black_max, interp, border, d_out, out_stride, out_step,
                      d_out_size=None, d_best=None):
        """omr.rs:339-452 for a batch: sweep -> arg-max -> CONTAIN warp by the detected angle, all on the device"""
        check(lib().omr_batch_deskew_device(self.handle, d_scans, scan_stride, step_bytes, n, black_max, interp, border,
                                            d_out, out_stride, out_step, d_out_size, d_best))

    def run_device_cn(self, d_scans, scan_stride, step_bytes, channels, n, black_max, d_best, d_v_sd=None, d_h_sd=None):
        """run_device for scans of `channels` interleaved channels (3 = BGR: gray = cvtColor(COLOR_RGB2GRAY) of the BGR bytes,
        quirk B8, fused into the load; 1 = run_device)"""
        check(lib().omr_batch_run_device_cn(self.handle, d_scans, scan_stride, step_bytes, channels, n, black_max, d_best,
                                            d_v_sd, d_h_sd))

    def deskew_device_cn(self, d_scans, scan_stride, step_bytes, channels, n, black_max, interp, border, d_out, out_stride,
                         out_step, d_out_size=None, d_best=None):
        """deskew_device for scans of `channels` interleaved channels; border = one value per channel (a sequence) or
        one for all; every slot holds the largest canvas with channels * max_cols bytes per row at least"""
        check(lib().omr_batch_deskew_device_cn(self.handle, d_scans, scan_stride, step_bytes, channels, n, black_max, interp,
                                               _border4(border), d_out, out_stride, out_step, d_out_size, d_best))

    def sync(self):
        check(lib().omr_batch_sync(self.handle))

    def set_group(self, scans_per_launch):
        """Scans carried by one launch of each kernel (amortises the launch-to-launch cost)."""
        check(lib().omr_batch_set_group(self.handle, int(scans_per_launch)))

    def set_lanes(self, max_scans_per_launch):
        """Scan-lane sweep: up to this many scans per launch, 64 scans per wavefront (0 = back to the run-merging path)."""
        check(lib().omr_batch_set_lanes(self.handle, int(max_scans_per_launch)))

    def lanes_keep(self, on=True):
        """Inspection: launches leave their row counts in place for lanes_projections()."""
        check(lib().omr_batch_lanes_keep(self.handle, 1 if on else 0))

    def lanes_program_bytes(self):
        b, t, n = C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().omr_batch_lanes_info(self.handle, C.byref(b), C.byref(t), C.byref(n)))
        return b.value

    def lanes_check_programs(self):
        """(dwords of programs, dwords that differ from the host generator's): the device-built plan against the
        reference implementation (tests, inspection)."""
        n, d = C.c_int64(), C.c_int64()
        check(lib().omr_batch_lanes_check_programs(self.handle, C.byref(n), C.byref(d)))
        return n.value, d.value

    def lanes_projections(self, scan, a, rows, cols, scratch_set=0, want_rows=True):
        """(vproj, hproj) of one scan / candidate as the last scan-lane launch left them (tests, inspection).  The row
        counts need lanes_keep(); want_rows=False asks for the column counts alone (hproj is None)."""
        vp, hp = np.zeros(cols, np.uint32), np.zeros(rows, np.uint32) if want_rows else None
        check(lib().omr_batch_lanes_projections(self.handle, scratch_set, scan, a, vp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                hp.ctypes.data_as(C.POINTER(C.c_uint32)) if want_rows else None))
        return vp, hp

    def info(self):
        r, g = C.c_int32(), C.c_int32()
        check(lib().omr_batch_info(self.handle, C.byref(r), C.byref(g)))
        return r.value, g.value

    def set_timing(self, on):
        check(lib().omr_batch_set_timing(self.handle, 1 if on else 0))

    def kernel_ms(self):
        s, n = C.c_double(), C.c_int32()
        check(lib().omr_batch_kernel_ms(self.handle, C.byref(s), C.byref(n)))
        return s.value, n.value


class HostBatch:
    """omr_host_batch: repeated batches that start in host memory (plan, pinned ring and device stages made once)."""

    def __init__(self, rows, cols, max_angle, step, max_scans, n_devices=0):
        self.handle = C.c_void_p()
        self.rows, self.cols = rows, cols
        _, self.A = candidate_count(max_angle, step)
        check(lib().omr_host_batch_create(rows, cols, int(max_angle), float(step), n_devices, int(max_scans),
                                          C.byref(self.handle)))

    def info(self):
        nd, spl, sl = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().omr_host_batch_info(self.handle, C.byref(nd), C.byref(spl), C.byref(sl)))
        return nd.value, spl.value, bool(sl.value)

    PAGEABLE, PINNED, PACKED = 0, 1, 2  # omr_host_batch_run's transfer modes (include/omrdeskew.h)

    def set_launch(self, scans_per_launch):
        """scans per sweep launch (scan-lane contexts: multiples of 64; default 64)"""
        check(lib().omr_host_batch_set_launch(self.handle, int(scans_per_launch)))

    def run(self, scans, pinned=False, want_sd=False, packed=False):
        """scans: list of 2-D u8 arrays (pixels == 0 black).  pinned=True: the arrays live in page-locked memory;
        packed=True: the context's copier threads pack them to 1 bit per pixel and 1/8 of the bytes are uploaded."""
        from ._lib import OmrImage
        keep, arr = [], (OmrImage * len(scans))()
        for i, s in enumerate(scans):
            a, im = as_image(_mat(s))
            keep.append(a)
            arr[i] = im
        n = len(scans)
        best = np.zeros(n, np.int32)
        ang = np.zeros(n, np.float64)
        vs = np.zeros((n, self.A)) if want_sd else None
        hs = np.zeros((n, self.A)) if want_sd else None
        check(lib().omr_host_batch_run(self.handle, arr, n, 2 if packed else 1 if pinned else 0, best.ctypes.data_as(i32p),
                                       ang.ctypes.data_as(f64p), vs.ctypes.data_as(f64p) if want_sd else None,
                                       hs.ctypes.data_as(f64p) if want_sd else None))
        return best, ang, vs, hs

    def close(self):
        if self.handle:
            lib().omr_host_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def sweep_batch(scans, max_angle, step, n_devices=0, want_sd=False):
    """omr_sweep_batch: host images, scan i -> device i % n_devices, host-side gather."""
    from ._lib import OmrImage
    keep, arr = [], (OmrImage * len(scans))()
    for i, s in enumerate(scans):
        a, im = as_image(_mat(s))
        keep.append(a)
        arr[i] = im
    n = len(scans)
    _, A = candidate_count(max_angle, step)
    best = np.zeros(n, np.int32)
    ang = np.zeros(n, np.float64)
    vs = np.zeros((n, A)) if want_sd else None
    hs = np.zeros((n, A)) if want_sd else None
    check(lib().omr_sweep_batch(arr, n, int(max_angle), float(step), n_devices, best.ctypes.data_as(i32p),
                                ang.ctypes.data_as(f64p), vs.ctypes.data_as(f64p) if want_sd else None,
                                hs.ctypes.data_as(f64p) if want_sd else None))
    return best, ang, vs, hs
