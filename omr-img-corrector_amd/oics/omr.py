"""oics::omr (packages/lib/src/omr.rs) through the C ABI."""
import ctypes as C
import os

import numpy as np

from ._lib import OmrImageOwned, check, f64p, i32p, lib
from .transfer import _mat, as_image
from .types import ResultStatus


class OmrResult:
    """omr.rs:46-50"""

    def __init__(self, angle, status, candidates):
        self.angle = angle
        self.status = status
        self.candidates = candidates


def get_mat_projection_data(mat):
    """omr.rs:8-39 -> (horizontal[rows], vertical[cols])"""
    a, im = as_image(_mat(mat))
    h, v = np.empty(im.rows, np.float64), np.empty(im.cols, np.float64)
    check(lib().omr_get_mat_projection_data(C.byref(im), h.ctypes.data_as(f64p), v.ctypes.data_as(f64p)))
    return h, v


def get_result_from_projection(src_mat, projection_max_angle, projection_angle_step, projection_max_width,
                               projection_max_height):
    """omr.rs:52-229"""
    a, im = as_image(_mat(src_mat))
    n = C.c_int32()
    A = lib().omr_candidate_count(int(projection_max_angle), float(projection_angle_step), C.byref(n))
    cand = np.zeros(max(A, 1), np.float64)
    angle, status, clen = C.c_double(), C.c_int32(), C.c_int32()
    check(lib().omr_get_result_from_projection(C.byref(im), int(projection_max_angle), float(projection_angle_step),
                                               int(projection_max_width), int(projection_max_height), C.byref(angle),
                                               C.byref(status), cand.ctypes.data_as(f64p), cand.size, C.byref(clen)))
    return OmrResult(angle.value, ResultStatus(status.value), cand[: clen.value].copy())


def select_projection_result(v_sd, h_sd, N, step):
    """omr.rs:147-221 on host arrays"""
    v = np.ascontiguousarray(v_sd, np.float64)
    h = np.ascontiguousarray(h_sd, np.float64)
    cand = np.zeros(max(v.size, 1), np.float64)
    angle, status, clen = C.c_double(), C.c_int32(), C.c_int32()
    check(lib().omr_select_projection_result(v.ctypes.data_as(f64p), h.ctypes.data_as(f64p), v.size, N, float(step),
                                             C.byref(angle), C.byref(status), cand.ctypes.data_as(f64p), cand.size,
                                             C.byref(clen)))
    return OmrResult(angle.value, ResultStatus(status.value), cand[: clen.value].copy())


def get_result_from_edges_detection(src_mat, edges_min_line_length, edges_max_line_gap):
    """omr.rs:231-302"""
    a, im = as_image(_mat(src_mat))
    cap = 1 << 16
    cand = np.zeros(cap, np.float64)
    angle, status, clen = C.c_double(), C.c_int32(), C.c_int32()
    check(lib().omr_get_result_from_edges_detection(C.byref(im), float(edges_min_line_length), float(edges_max_line_gap),
                                                    C.byref(angle), C.byref(status), cand.ctypes.data_as(f64p), cap,
                                                    C.byref(clen)))
    return OmrResult(angle.value, ResultStatus(status.value), cand[: min(clen.value, cap)].copy())


def edges_detection_batch_device(d_scans_ptr, n, scan_stride, rows, cols, channels, step, min_line_length, max_line_gap,
                                 stream=None):
    """get_result_from_edges_detection on n device-resident scans -> (angles, status, n_lines)"""
    angles = np.zeros(n, np.float64)
    status = np.zeros(n, np.int32)
    nl = np.zeros(n, np.int32)
    check(lib().omr_edges_detection_batch_device(d_scans_ptr, n, scan_stride, rows, cols, channels, step,
                                                 float(min_line_length), float(max_line_gap), angles.ctypes.data_as(f64p),
                                                 status.ctypes.data_as(i32p), nl.ctypes.data_as(i32p), stream))
    return angles, status, nl


def fourier_transform_batch_device(d_scans_ptr, n, scan_stride, rows, cols, channels, step, canny_threshold_weak,
                                   canny_threshold_strong, fourier_min_line_length, fourier_max_line_gap, stream=None):
    """get_result_from_fourier_transform on n device-resident colour scans (3 or 4 channels) -> (angles, status,
    n_lines); a scan without any segment reports status NotAResult and angle 0.0"""
    n = int(n)
    angles = np.zeros(max(n, 0), np.float64)
    status = np.zeros(max(n, 0), np.int32)
    nl = np.zeros(max(n, 0), np.int32)
    check(lib().omr_fourier_transform_batch_device(d_scans_ptr, n, int(scan_stride), int(rows), int(cols), int(channels),
                                                   int(step), float(canny_threshold_weak), float(canny_threshold_strong),
                                                   float(fourier_min_line_length), float(fourier_max_line_gap),
                                                   angles.ctypes.data_as(f64p), status.ctypes.data_as(i32p),
                                                   nl.ctypes.data_as(i32p), stream))
    return angles, status, nl


def hough_set_scans_in_flight(scans):
    """Tuning knob of edges_detection_batch_device (include/omrdeskew.h): scans the sequential Hough stage works on at
    once; 0 = the library's default.  Returns the previous setting."""
    return int(lib().omr_hough_set_scans_in_flight(int(scans)))


def correct_default_decision(projection_result, edges_angle):
    """omr.rs:351-399 -> (rotate_angle, need_check)"""
    c = np.ascontiguousarray(projection_result.candidates, np.float64)
    ang, chk = C.c_double(), C.c_int32()
    lib().omr_correct_default_decision(float(projection_result.angle), int(projection_result.status),
                                       c.ctypes.data_as(f64p), c.size, float(edges_angle), C.byref(ang), C.byref(chk))
    return ang.value, bool(chk.value)


def correct_default(src_mat, projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                    hough_min_line_length, hough_max_line_gap, want_image=True):
    """omr.rs:339-448 on a decoded BGR image (imread / imwrite are the caller's) ->
    (rotate_angle, need_check, rotated image or None)"""
    from .hough import _take
    a, im = as_image(_mat(src_mat))
    ang, chk = C.c_double(), C.c_int32()
    owned = OmrImageOwned()
    check(lib().omr_correct_default(C.byref(im), int(projection_max_angle), float(projection_angle_step),
                                    int(projection_max_width), int(projection_max_height), float(hough_min_line_length),
                                    float(hough_max_line_gap), C.byref(ang), C.byref(chk),
                                    C.byref(owned) if want_image else None))
    return ang.value, bool(chk.value), (_take(owned) if want_image else None)


def correct_batch_canvas(rows, cols):
    """Largest CONTAIN canvas any angle gives at rows x cols (cols rounded up to 4) -> (rows, cols); no GPU needed."""
    r, c = C.c_int32(), C.c_int32()
    check(lib().omr_correct_batch_canvas(int(rows), int(cols), C.byref(r), C.byref(c)))
    return r.value, c.value


class CorrectBatch:
    """omr_correct_batch_*: correct_default for repeated batches of device-resident sheets of one shape and one
    parameter set."""

    def __init__(self, rows, cols, channels, projection_max_angle, projection_angle_step, projection_max_width,
                 projection_max_height, hough_min_line_length, hough_max_line_gap, device=0, max_scans=256):
        self.handle = C.c_void_p()
        check(lib().omr_correct_batch_create(int(rows), int(cols), int(channels), int(projection_max_angle),
                                             float(projection_angle_step), int(projection_max_width),
                                             int(projection_max_height), float(hough_min_line_length),
                                             float(hough_max_line_gap), int(device), int(max_scans), C.byref(self.handle)))
        self.rows, self.cols, self.channels, self.max_scans = rows, cols, channels, max_scans
        self.canvas = correct_batch_canvas(rows, cols)

    def close(self):
        if self.handle:
            lib().omr_correct_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        self.close()

    def run_device(self, d_scans, scan_stride, step, n, d_out=None, out_stride=0, out_step=0):
        """device pointers in -> (rotate_angle f64[n], need_check bool[n], scan_rc i32[n], out_size i32[n, 2])"""
        ang = np.zeros(n, np.float64)
        chk = np.zeros(n, np.int32)
        rc = np.zeros(n, np.int32)
        size = np.zeros((n, 2), np.int32)
        check(lib().omr_correct_batch_run_device(self.handle, d_scans, int(scan_stride), int(step), int(n),
                                                 ang.ctypes.data_as(f64p), chk.ctypes.data_as(i32p), rc.ctypes.data_as(i32p),
                                                 d_out, int(out_stride), int(out_step), size.ctypes.data_as(i32p)))
        return ang, chk.astype(bool), rc, size

    def info(self):
        """-> (proj_rows, proj_cols, front_mode, kx, ky): the front end's projection size, OMR_CORRECT_FRONT_* mode and
        integer shrink factors (0 outside the integer modes).  For tests and inspection."""
        v = [C.c_int32() for _ in range(5)]
        check(lib().omr_correct_batch_info(self.handle, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def front_device(self, d_scans, scan_stride, step, n, d_small, small_stride, small_step):
        """the front end alone: n sheets' projection-size images (before the threshold) to d_small.  For tests and
        inspection."""
        check(lib().omr_correct_batch_front_device(self.handle, d_scans, int(scan_stride), int(step), int(n), d_small,
                                                   int(small_stride), int(small_step)))


FRONT_AREA_FUSED, FRONT_AREA_INT, FRONT_AREA_GENERAL, FRONT_LINEAR = 0, 1, 2, 3  # OMR_CORRECT_FRONT_*


def correct_default_batch(src_mats, projection_max_angle, projection_angle_step, projection_max_width,
                          projection_max_height, hough_min_line_length, hough_max_line_gap, want_image=True):
    """omr_correct_default_batch: correct_default of many decoded sheets of any shapes ->
    [(rotate_angle, need_check, rotated image or None, scan_rc)] in input order (scan_rc != 0: the sheet failed as the
    per-call function would, and carries no image)"""
    from .hough import _take
    from ._lib import OmrImage
    keep, ims = [], []
    for m in src_mats:
        a, im = as_image(_mat(m))
        keep.append(a)
        ims.append(im)
    n = len(ims)
    arr = (OmrImage * n)(*ims)
    ang = np.zeros(n, np.float64)
    chk = np.zeros(n, np.int32)
    rc = np.zeros(n, np.int32)
    owned = (OmrImageOwned * n)() if want_image else None
    check(lib().omr_correct_default_batch(arr, n, int(projection_max_angle), float(projection_angle_step),
                                          int(projection_max_width), int(projection_max_height),
                                          float(hough_min_line_length), float(hough_max_line_gap), ang.ctypes.data_as(f64p),
                                          chk.ctypes.data_as(i32p), rc.ctypes.data_as(i32p), owned))
    imgs = [None] * n
    if want_image:  # one copy per image out of the library's buffer: on threads (numpy's copy releases the GIL)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            imgs = list(ex.map(lambda i: _take(owned[i]) if owned[i].data else None, range(n)))
    return [(float(ang[i]), bool(chk[i]), imgs[i], int(rc[i])) for i in range(n)]


def _streams_out(n, ang, chk, rc, ptrs, lens):
    out = []
    for i in range(n):
        data = None
        if ptrs[i]:
            data = C.string_at(ptrs[i], int(lens[i]))
            lib().omr_bytes_free(ptrs[i])
        out.append((float(ang[i]), bool(chk[i]), data, int(rc[i])))
    return out


def _batch_encoded(symbol, src_mats, params, level):
    """the host-image flow functions that return streams: omr_correct_default_batch_jpeg / _png"""
    from ._lib import OmrImage, u8p
    keep, ims = [], []
    for m in src_mats:
        a, im = as_image(_mat(m))
        keep.append(a)
        ims.append(im)
    n = len(ims)
    arr = (OmrImage * max(n, 1))(*ims)
    ang = np.zeros(n, np.float64)
    chk = np.zeros(n, np.int32)
    rc = np.zeros(n, np.int32)
    ptrs = (u8p * max(n, 1))()
    lens = np.zeros(max(n, 1), np.int64)
    max_angle, angle_step, max_width, max_height, min_line_length, max_line_gap = params
    check(getattr(lib(), symbol)(arr, n, int(max_angle), float(angle_step), int(max_width), int(max_height),
                                 float(min_line_length), float(max_line_gap), int(level), ang.ctypes.data_as(f64p),
                                 chk.ctypes.data_as(i32p), rc.ctypes.data_as(i32p), ptrs,
                                 lens.ctypes.data_as(C.POINTER(C.c_int64))))
    return _streams_out(n, ang, chk, rc, ptrs, lens)


def _streams_encoded(symbol, streams, params, level):
    """the flow functions from streams to streams: omr_correct_default_batch_streams / _streams_png"""
    from ._lib import u8p
    bufs = [np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray, memoryview)) else np.ascontiguousarray(s, np.uint8)
            for s in streams]
    bufs = [b if b.size else np.zeros(1, np.uint8) for b in bufs]
    n = len(bufs)
    sp = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    sl = np.array([len(s) for s in streams] + [0], np.int64)
    ang = np.zeros(max(n, 1), np.float64)
    chk = np.zeros(max(n, 1), np.int32)
    rc = np.zeros(max(n, 1), np.int32)
    ptrs = (u8p * max(n, 1))()
    lens = np.zeros(max(n, 1), np.int64)
    max_angle, angle_step, max_width, max_height, min_line_length, max_line_gap = params
    check(getattr(lib(), symbol)(sp, sl.ctypes.data_as(C.POINTER(C.c_int64)), n, int(max_angle), float(angle_step),
                                 int(max_width), int(max_height), float(min_line_length), float(max_line_gap), int(level),
                                 ang.ctypes.data_as(f64p), chk.ctypes.data_as(i32p), rc.ctypes.data_as(i32p), ptrs,
                                 lens.ctypes.data_as(C.POINTER(C.c_int64))))
    return _streams_out(n, ang, chk, rc, ptrs, lens)


def correct_default_batch_jpeg(src_mats, projection_max_angle, projection_angle_step, projection_max_width,
                               projection_max_height, hough_min_line_length, hough_max_line_gap, quality=100):
    """omr_correct_default_batch_jpeg: correct_default_batch with every rotated sheet encoded on the device ->
    [(rotate_angle, need_check, JPEG bytes or None, scan_rc)] in input order"""
    return _batch_encoded("omr_correct_default_batch_jpeg", src_mats,
                          (projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                           hough_min_line_length, hough_max_line_gap), quality)


def correct_default_batch_png(src_mats, projection_max_angle, projection_angle_step, projection_max_width,
                              projection_max_height, hough_min_line_length, hough_max_line_gap, compression=1):
    """omr_correct_default_batch_png: correct_default_batch_jpeg with lossless PNG streams ->
    [(rotate_angle, need_check, PNG bytes or None, scan_rc)] in input order"""
    return _batch_encoded("omr_correct_default_batch_png", src_mats,
                          (projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                           hough_min_line_length, hough_max_line_gap), compression)


def correct_default_batch_streams(streams, projection_max_angle, projection_angle_step, projection_max_width,
                                  projection_max_height, hough_min_line_length, hough_max_line_gap, quality=100):
    """omr_correct_default_batch_streams: correct_default from file contents to file contents.  streams: baseline JPEG
    streams (bytes or uint8 arrays), decoded to BGR, corrected and encoded on the device -> [(rotate_angle, need_check,
    JPEG bytes or None, scan_rc)] in input order; scan_rc is the decoder's code for a sheet it refused."""
    return _streams_encoded("omr_correct_default_batch_streams", streams,
                            (projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                             hough_min_line_length, hough_max_line_gap), quality)


def correct_default_batch_streams_png(streams, projection_max_angle, projection_angle_step, projection_max_width,
                                      projection_max_height, hough_min_line_length, hough_max_line_gap, compression=1):
    """omr_correct_default_batch_streams_png: correct_default_batch_streams (JPEG and PNG inputs, mixed) with lossless PNG
    streams as its outputs -> [(rotate_angle, need_check, PNG bytes or None, scan_rc)] in input order"""
    return _streams_encoded("omr_correct_default_batch_streams_png", streams,
                            (projection_max_angle, projection_angle_step, projection_max_width, projection_max_height,
                             hough_min_line_length, hough_max_line_gap), compression)


def get_result_from_fourier_transform(src_mat, canny_threshold_weak, canny_threshold_strong, fourier_min_line_length,
                                      fourier_max_line_gap):
    """omr.rs:304-337"""
    a, im = as_image(_mat(src_mat))
    cap = 1 << 16
    cand = np.zeros(cap, np.float64)
    angle, status, clen = C.c_double(), C.c_int32(), C.c_int32()
    check(lib().omr_get_result_from_fourier_transform(C.byref(im), float(canny_threshold_weak),
                                                      float(canny_threshold_strong), float(fourier_min_line_length),
                                                      float(fourier_max_line_gap), C.byref(angle), C.byref(status),
                                                      cand.ctypes.data_as(f64p), cap, C.byref(clen)))
    return OmrResult(angle.value, ResultStatus(status.value), cand[: min(clen.value, cap)].copy())
