"""oics::hough (packages/lib/src/hough.rs) through the C ABI, plus the two OpenCV calls it is made of."""
import ctypes as C

import numpy as np

from ._lib import OmrImage, OmrImageOwned, check, f64p, i32p, lib, u8p
from . import transfer as _transfer
from .transfer import _mat, as_image


def _take(owned):
    n = owned.rows * owned.step_bytes
    out = np.ctypeslib.as_array(C.cast(owned.data, C.POINTER(C.c_uint8)), shape=(n,)).copy()
    out = out.reshape(owned.rows, owned.step_bytes)[:, : owned.cols * owned.channels]
    out = out.reshape(owned.rows, owned.cols) if owned.channels == 1 else out.reshape(owned.rows, owned.cols, owned.channels)
    lib().omr_image_free(C.byref(owned))
    return np.ascontiguousarray(out)


def canny(src, low_thresh=50.0, high_thresh=150.0):
    """imgproc::canny(src, &mut edges, low, high, 3, false) -- hough.rs:27, omr.rs:239"""
    a, im = as_image(_mat(src))
    owned = OmrImageOwned()
    check(lib().omr_canny(C.byref(im), float(low_thresh), float(high_thresh), C.byref(owned)))
    return _take(owned)


def hough_lines_p(edges, rho, theta, threshold, min_line_length, max_line_gap):
    """imgproc::hough_lines_p -- hough.rs:31-43.  Returns int32 [n, 4] (x0, y0, x1, y1)."""
    a, im = as_image(_mat(edges))
    n = C.c_int32(0)
    cap = 4096
    while True:
        lines = np.zeros((cap, 4), np.int32)
        check(lib().omr_hough_lines_p(C.byref(im), float(rho), float(theta), int(threshold), float(min_line_length),
                                      float(max_line_gap), lines.ctypes.data_as(i32p), cap, C.byref(n)))
        if n.value <= cap:
            return lines[: n.value].copy()
        cap = n.value


LINED_COLOR = (186, 88, 255)  # Scalar(186, 88, 255, 0), B G R: hough.rs:59, fft.rs:209


def _bgr(color):
    c = np.asarray(color, np.uint8).reshape(3)
    return c, c.ctypes.data_as(u8p)


def lined_picture(edges, lines, color=LINED_COLOR):
    """omr_lined_picture: GRAY2BGR of an 8-bit one-channel edge map with the segments `lines` ([n, 4] x0 y0 x1 y1, as
    hough_lines_p returns them) drawn on in list order by line(.., color, 1, LINE_AA, 0) -- hough.rs:44-63.  Returns
    [rows, cols, 3] uint8."""
    a, im = as_image(_mat(edges))
    l = np.ascontiguousarray(np.asarray(lines, np.int32).reshape(-1, 4))
    keep, c = _bgr(color)
    owned = OmrImageOwned()
    check(lib().omr_lined_picture(C.byref(im), l.ctypes.data_as(i32p) if len(l) else None, len(l), c, C.byref(owned)))
    return _take(owned)


def lined_picture_batch_device(d_edges, n, edge_stride_bytes, edge_step, rows, cols, d_lines, line_offsets, d_out,
                               out_stride_bytes, out_step, color=LINED_COLOR, stream=None):
    """omr_lined_picture_batch_device: n same-shape device-resident edge maps (d_edges, d_lines, d_out: device
    addresses), picture i at d_out + i * out_stride_bytes with the segments line_offsets[i] .. line_offsets[i + 1] of
    d_lines drawn on; line_offsets is a host sequence of n + 1.  Byte for byte omr_lined_picture_device's pictures.
    Synchronises `stream` before returning."""
    off = np.ascontiguousarray(np.asarray(line_offsets, np.int32).reshape(-1))
    if len(off) != int(n) + 1:
        raise ValueError("line_offsets holds n + 1 entries")
    keep, c = _bgr(color)
    check(lib().omr_lined_picture_batch_device(d_edges, int(n), int(edge_stride_bytes), int(edge_step), int(rows), int(cols),
                                               d_lines, off.ctypes.data_as(i32p), c, d_out, int(out_stride_bytes),
                                               int(out_step), stream))


def get_angle_with_hough(gray_tm, min_line_length, max_line_gap, want_picture=False):
    """hough.rs:17-100; file_name / edge_image_output_dir stay host-side.  want_picture=True returns (angle, picture):
    the picture the reference writes there -- the edge map in colour with every segment drawn on, [rows, cols, 3]."""
    a, im = as_image(_mat(gray_tm))
    out = C.c_double()
    if not want_picture:
        check(lib().omr_get_angle_with_hough(C.byref(im), float(min_line_length), float(max_line_gap), C.byref(out)))
        return out.value
    owned = OmrImageOwned()
    check(lib().omr_get_angle_with_hough_ex(C.byref(im), float(min_line_length), float(max_line_gap), C.byref(out),
                                            C.byref(owned)))
    return out.value, _take(owned)


def hough_angles_batch_device(d_scans, n, scan_stride_bytes, rows, cols, channels, step_bytes, min_line_length, max_line_gap,
                              d_lined=None, lined_stride_bytes=0, lined_step=0, stream=None):
    """omr_hough_angles_batch_device: get_angle_with_hough on n same-shape device-resident scans (d_scans, d_lined:
    device addresses).  Returns (angles float64 [n], rc int32 [n], n_lines int32 [n]): angles[i] has the bits the
    per-call function returns, rc[i] is 0, or -215 with angle 0.0 for a scan without any segment.  With d_lined,
    picture i (the per-call want_picture=True result, byte for byte) lands at d_lined + i * lined_stride_bytes, rows
    lined_step apart; the slot of a scan without a segment is not written.  Synchronises `stream` before returning."""
    n = int(n)
    angles = np.zeros(max(n, 0), np.float64)
    rc = np.zeros(max(n, 0), np.int32)
    n_lines = np.zeros(max(n, 0), np.int32)
    check(lib().omr_hough_angles_batch_device(d_scans, n, int(scan_stride_bytes), int(rows), int(cols), int(channels),
                                              int(step_bytes), float(min_line_length), float(max_line_gap),
                                              angles.ctypes.data_as(f64p), rc.ctypes.data_as(i32p),
                                              n_lines.ctypes.data_as(i32p), d_lined, int(lined_stride_bytes),
                                              int(lined_step), stream))
    return angles, rc, n_lines


def get_angles_with_hough(grays, min_line_length, max_line_gap, want_pictures=False):
    """get_angle_with_hough for a batch (omr_get_angles_with_hough_batch): host images of any mix of shapes and of 1, 3
    or 4 channels; same-shape images go through Canny, HoughLinesP and the vote together on the device.  Returns
    (angles float64 [n], rc int32 [n]): angles[i] is the per-call angle of grays[i] (same bits) and rc[i] is 0, or -215
    with angle 0.0 where the per-call function raises for want of a segment.  want_pictures=True adds a list of n
    pictures ([rows, cols, 3] uint8, the per-call want_picture=True result), None where rc[i] != 0.  An invalid image
    fails the whole call."""
    keep = [as_image(_mat(g)) for g in grays]
    n = len(keep)
    arr = (OmrImage * max(n, 1))(*[im for _, im in keep])
    angles = np.zeros(n, np.float64)
    rc = np.zeros(n, np.int32)
    owned = (OmrImageOwned * max(n, 1))() if want_pictures else None
    check(lib().omr_get_angles_with_hough_batch(arr, n, float(min_line_length), float(max_line_gap),
                                                angles.ctypes.data_as(f64p), rc.ctypes.data_as(i32p), owned))
    if not want_pictures:
        return angles, rc
    return angles, rc, [_take(owned[i]) if owned[i].data else None for i in range(n)]


def deskew_device(d_scans, n, scan_stride_bytes, rows, cols, channels, step_bytes, min_line_length, max_line_gap, flags,
                  border_mode, border_value, clip_strategy, d_out, out_stride_bytes, out_step_bytes, stream=None):
    """omr_hough_deskew_batch_device: the Hough leg of the reference's benchmark on n same-shape device-resident scans of 1
    or 3 channels (d_scans, d_out: device addresses as ints) -- gray, get_angle_with_hough, rotate_mat of the ORIGINAL scan
    by its angle into the top left of its slot (every slot holds transfer.detector_deskew_canvas's answer).  Returns
    (angles, rc, n_lines, sizes): angles[i] has the per-call detector's bits, sizes[i] the canvas's (rows, cols); a scan
    without a segment has rc -215, angle 0.0, size (0, 0) and an untouched slot.  Synchronises `stream`."""
    return _transfer._detector_deskew_device("omr_hough_deskew_batch_device", (min_line_length, max_line_gap), d_scans, n,
                                             scan_stride_bytes, rows, cols, channels, step_bytes, flags, border_mode, border_value,
                                             clip_strategy, d_out, out_stride_bytes, out_step_bytes, stream)


def deskew(srcs, min_line_length, max_line_gap, flags=1, border_mode=0, border_value=(255, 255, 255, 0), clip_strategy=1):
    """omr_deskew_with_hough_batch: the same for host images of any mix of shapes, 1 or 3 channels each.  Returns
    (angles, rc, images): images[i] is what transfer.rotate_mat gives for srcs[i] and angles[i] (an array), None where
    rc[i] != 0.  An invalid image fails the whole call."""
    return _transfer._detector_deskew("omr_deskew_with_hough_batch", (min_line_length, max_line_gap), srcs, flags, border_mode,
                                      border_value, clip_strategy)


def deskew_streams(streams, min_line_length, max_line_gap, flags=1, border_mode=0, border_value=(255, 255, 255, 0),
                   clip_strategy=1, channels=3, png=False, level=100, want_out=True):
    """omr_deskew_with_hough_batch_streams: the same from file contents (baseline JPEG or PNG, mixed, read as imread reads
    them) to file contents (JPEG at quality `level`, or png=True: PNG at compression `level`), decoded and encoded on the
    device.  Returns (angles, scan_rc, outputs): outputs[i] bytes, None where scan_rc[i] != 0 (a refused or damaged file,
    or a scan without a segment); want_out=False: the angles alone, outputs is None."""
    return _transfer._detector_deskew_streams("omr_deskew_with_hough_batch_streams", (min_line_length, max_line_gap), streams,
                                              channels, flags, border_mode, border_value, clip_strategy, 1 if png else 0, level,
                                              want_out)


def deskew_streams_tiff(streams, min_line_length, max_line_gap, flags=1, border_mode=0, border_value=(255, 255, 255, 0),
                        clip_strategy=1, channels=3, threshold=127, rows_per_strip=0, dpi=0, want_out=True):
    """omr_deskew_with_hough_batch_streams_tiff: deskew_streams with Group 4 TIFF files as its outputs, outputs[i] byte for
    byte oics.tiff.encode(canvas, threshold, rows_per_strip, dpi)."""
    return _transfer._detector_deskew_streams("omr_deskew_with_hough_batch_streams_tiff", (min_line_length, max_line_gap), streams,
                                              channels, flags, border_mode, border_value, clip_strategy, 0, threshold, want_out,
                                              tiff=(rows_per_strip, dpi))


def deskew_streams_tiff8(streams, min_line_length, max_line_gap, flags=1, border_mode=0, border_value=(255, 255, 255, 0),
                         clip_strategy=1, channels=3, compression=5, predictor=1, rows_per_strip=0, dpi=0, want_out=True):
    """omr_deskew_with_hough_batch_streams_tiff8: deskew_streams with 8-bit TIFF files as its outputs, outputs[i] byte for
    byte oics.tiff.encode8(canvas, compression, predictor, rows_per_strip, dpi)."""
    return _transfer._detector_deskew_streams("omr_deskew_with_hough_batch_streams_tiff8", (min_line_length, max_line_gap), streams,
                                              channels, flags, border_mode, border_value, clip_strategy, 0, compression, want_out,
                                              tiff=(predictor, rows_per_strip, dpi))
