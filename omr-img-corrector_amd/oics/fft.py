"""oics::fft (packages/lib/src/fft.rs) through the C ABI."""
import ctypes as C

from ._lib import OmrImageOwned, check, lib
from .hough import LINED_COLOR, _take, lined_picture as _lined_picture, lined_picture_batch_device as _lined_batch
from .transfer import _mat, as_image


def get_fft_image(gray_tm):
    """fft.rs:124-141 -> (magnitude_image, magnitude_log_image), uint8"""
    a, im = as_image(_mat(gray_tm))
    m, lg = OmrImageOwned(), OmrImageOwned()
    check(lib().omr_get_fft_image(C.byref(im), C.byref(m), C.byref(lg)))
    return _take(m), _take(lg)


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
