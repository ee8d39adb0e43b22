"""oics::fft (packages/lib/src/fft.rs) through the C ABI."""
import ctypes as C

import numpy as np

from ._lib import OmrImage, OmrImageOwned, check, f64p, i32p, lib
from .hough import LINED_COLOR, _take, lined_picture as _lined_picture, lined_picture_batch_device as _lined_batch
from . import transfer as _transfer
from .transfer import _mat, as_image


def get_fft_image(gray_tm):
    """fft.rs:124-141 -> (magnitude_image, magnitude_log_image), uint8"""
    a, im = as_image(_mat(gray_tm))
    m, lg = OmrImageOwned(), OmrImageOwned()
    check(lib().omr_get_fft_image(C.byref(im), C.byref(m), C.byref(lg)))
    return _take(m), _take(lg)


def spectrum_raw(gray_tm):
    """omr_fft_spectrum_raw, the inspection hook behind the spectrum tests: get_fft_image's run with the float arrays
    the pictures are made from.  Returns (row_pass, magnitude, (min, max), magnitude_image, magnitude_log_image) for a
    [R, C] scan, H = C // 2 + 1: row_pass complex64 [H, R], the row pass's half spectrum, [c, r] = sum_x img[r, x]
    exp(-2 pi i c x / C) (unscaled); magnitude float32 [H, R], [c, k] = |F(k, c)| with DFT_SCALE, unshifted; the extrema
    of magnitude as float32, as the picture kernel reads them; the two uint8 pictures of the same run."""
    from ._lib import f32p
    a, im = as_image(_mat(gray_tm))
    rows, cols = a.shape[:2]
    half = cols // 2 + 1
    row = np.zeros((half, rows), np.complex64)
    mag = np.zeros((half, rows), np.float32)
    ext = np.zeros(2, np.float32)
    m, lg = OmrImageOwned(), OmrImageOwned()
    check(lib().omr_fft_spectrum_raw(C.byref(im), row.ctypes.data_as(f32p), mag.ctypes.data_as(f32p), ext.ctypes.data_as(f32p),
                                     C.byref(m), C.byref(lg)))
    return row, mag, (ext[0], ext[1]), _take(m), _take(lg)


def fft_image_batch_device(d_scans_ptr, n, scan_stride, rows, cols, step, d_out_ptr, stream=None):
    """magnitude_log pictures of n device-resident scans (config 5)"""
    check(lib().omr_fft_image_batch_device(d_scans_ptr, n, scan_stride, rows, cols, step, d_out_ptr, stream))


def lined_picture(edges, lines, color=LINED_COLOR):
    """fft.rs:173-213: the picture of an edge map and its segments (hough.lined_picture: one entry point serves both)"""
    return _lined_picture(edges, lines, color)


def lined_picture_batch_device(*args, **kwargs):
    """hough.lined_picture_batch_device"""
    return _lined_batch(*args, **kwargs)


def get_angle_with_fft(gray_tm, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, want_picture=False):
    """fft.rs:145-256.  want_picture=True returns (angle, picture): the picture the reference writes there -- the edges
    of the log spectrum in colour with every segment drawn on, [rows, cols, 3]"""
    a, im = as_image(_mat(gray_tm))
    out = C.c_double()
    args = (C.byref(im), float(canny_threshold_1), float(canny_threshold_2), float(min_line_length), float(max_line_gap),
            C.byref(out))
    if not want_picture:
        check(lib().omr_get_angle_with_fft(*args))
        return out.value
    owned = OmrImageOwned()
    check(lib().omr_get_angle_with_fft_ex(*args, C.byref(owned)))
    return out.value, _take(owned)


def fft_angles_batch_device(d_scans, n, scan_stride_bytes, rows, cols, step_bytes, canny_threshold_1, canny_threshold_2,
                            min_line_length, max_line_gap, d_lined=None, lined_stride_bytes=0, lined_step=0, stream=None):
    """omr_fft_angles_batch_device: get_angle_with_fft on n same-shape device-resident 8-bit single-channel scans
    (d_scans, d_lined: device addresses).  Returns (angles float64 [n], n_lines int32 [n]): angles[i] has the bits the
    per-call function returns, 0.0 for a scan without any segment.  With d_lined, picture i (the per-call
    want_picture=True result, byte for byte) lands at d_lined + i * lined_stride_bytes, rows lined_step apart; every
    slot is written, the bare edge picture where there is no segment.  Synchronises `stream` before returning."""
    n = int(n)
    angles = np.zeros(max(n, 0), np.float64)
    n_lines = np.zeros(max(n, 0), np.int32)
    check(lib().omr_fft_angles_batch_device(d_scans, n, int(scan_stride_bytes), int(rows), int(cols), int(step_bytes),
                                            float(canny_threshold_1), float(canny_threshold_2), float(min_line_length),
                                            float(max_line_gap), angles.ctypes.data_as(f64p), n_lines.ctypes.data_as(i32p),
                                            d_lined, int(lined_stride_bytes), int(lined_step), stream))
    return angles, n_lines


def get_angles_with_fft(grays, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, want_pictures=False):
    """get_angle_with_fft for a batch (omr_get_angles_with_fft_batch): 8-bit single-channel host images of any mix of
    shapes; same-shape images go through the transform, Canny and HoughLinesP together on the device.  Returns angles
    float64 [n], angles[i] the per-call angle of grays[i] (same bits).  want_pictures=True returns (angles, pictures):
    n pictures [rows, cols, 3] uint8, the per-call want_picture=True results.  An invalid image fails the whole call."""
    keep = [as_image(_mat(g)) for g in grays]
    n = len(keep)
    arr = (OmrImage * max(n, 1))(*[im for _, im in keep])
    angles = np.zeros(n, np.float64)
    owned = (OmrImageOwned * max(n, 1))() if want_pictures else None
    check(lib().omr_get_angles_with_fft_batch(arr, n, float(canny_threshold_1), float(canny_threshold_2),
                                              float(min_line_length), float(max_line_gap), angles.ctypes.data_as(f64p), owned))
    if not want_pictures:
        return angles
    return angles, [_take(owned[i]) for i in range(n)]


def deskew_device(d_scans, n, scan_stride_bytes, rows, cols, channels, step_bytes, canny_threshold_1, canny_threshold_2,
                  min_line_length, max_line_gap, flags, border_mode, border_value, clip_strategy, d_out, out_stride_bytes,
                  out_step_bytes, stream=None):
    """omr_fft_deskew_batch_device: the FFT leg of the reference's benchmark on n same-shape device-resident scans of 1 or 3
    channels (d_scans, d_out: device addresses as ints) -- gray, get_angle_with_fft, rotate_mat of the ORIGINAL scan by its
    angle into the top left of its slot (every slot holds transfer.detector_deskew_canvas's answer).  Returns (angles, rc,
    n_lines, sizes): angles[i] has the per-call detector's bits (0.0 without a segment), rc is all 0, sizes[i] the
    canvas's (rows, cols).  Synchronises `stream`."""
    return _transfer._detector_deskew_device("omr_fft_deskew_batch_device",
                                             (canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), d_scans, n,
                                             scan_stride_bytes, rows, cols, channels, step_bytes, flags, border_mode, border_value,
                                             clip_strategy, d_out, out_stride_bytes, out_step_bytes, stream)


def deskew(srcs, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags=1, border_mode=0,
           border_value=(255, 255, 255, 0), clip_strategy=1):
    """omr_deskew_with_fft_batch: the same for host images of any mix of shapes, 1 or 3 channels each.  Returns (angles,
    images): images[i] is what transfer.rotate_mat gives for srcs[i] and angles[i] (an array).  An invalid image fails the
    whole call."""
    ang, _, images = _transfer._detector_deskew("omr_deskew_with_fft_batch",
                                                (canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), srcs, flags,
                                                border_mode, border_value, clip_strategy)
    return ang, images


def deskew_streams(streams, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags=1, border_mode=0,
                   border_value=(255, 255, 255, 0), clip_strategy=1, channels=3, png=False, level=100, want_out=True):
    """omr_deskew_with_fft_batch_streams: the same from file contents (baseline JPEG or PNG, mixed, read as imread reads
    them) to file contents (JPEG at quality `level`, or png=True: PNG at compression `level`), decoded and encoded on the
    device.  Returns (angles, scan_rc, outputs): outputs[i] bytes, None where scan_rc[i] != 0 (a refused or damaged file);
    want_out=False: the angles alone, outputs is None."""
    return _transfer._detector_deskew_streams("omr_deskew_with_fft_batch_streams",
                                              (canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), streams,
                                              channels, flags, border_mode, border_value, clip_strategy, 1 if png else 0, level,
                                              want_out)


def deskew_streams_tiff(streams, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags=1, border_mode=0,
                        border_value=(255, 255, 255, 0), clip_strategy=1, channels=3, threshold=127, rows_per_strip=0, dpi=0,
                        want_out=True):
    """omr_deskew_with_fft_batch_streams_tiff: deskew_streams with Group 4 TIFF files as its outputs, outputs[i] byte for
    byte oics.tiff.encode(canvas, threshold, rows_per_strip, dpi)."""
    return _transfer._detector_deskew_streams("omr_deskew_with_fft_batch_streams_tiff",
                                              (canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), streams,
                                              channels, flags, border_mode, border_value, clip_strategy, 0, threshold, want_out,
                                              tiff=(rows_per_strip, dpi))


def deskew_streams_tiff8(streams, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags=1, border_mode=0,
                         border_value=(255, 255, 255, 0), clip_strategy=1, channels=3, compression=5, predictor=1,
                         rows_per_strip=0, dpi=0, want_out=True):
    """omr_deskew_with_fft_batch_streams_tiff8: deskew_streams with 8-bit TIFF files as its outputs, outputs[i] byte for
    byte oics.tiff.encode8(canvas, compression, predictor, rows_per_strip, dpi)."""
    return _transfer._detector_deskew_streams("omr_deskew_with_fft_batch_streams_tiff8",
                                              (canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap), streams,
                                              channels, flags, border_mode, border_value, clip_strategy, 0, compression, want_out,
                                              tiff=(predictor, rows_per_strip, dpi))
