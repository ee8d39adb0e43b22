"""TIFF on the device (omr_tiff_*): bilevel files (uncompressed, PackBits and CCITT Group 4 strips, as 255 / 0) and 8-bit
gray and RGB files (uncompressed, PackBits and LZW strips, Predictor 1 and 2) decoded byte for byte to what libtiff gives,
a Group 4 encoder whose strips are byte for byte what libtiff writes, and an 8-bit gray and RGB encoder (uncompressed or
LZW, Predictor 1 and 2) whose files decode to the image exactly."""
import ctypes as C

import numpy as np

from . import _codec
from ._codec import _buf
from ._lib import OMR_TIFF_CODES, OmrImageOwned, check, i32p, lib
from .transfer import _mat, _take_owned, as_image


def info(stream):
    """omr_tiff_info -> (rows, cols, compression, photometric, fill_order, strips): what the first IFD says.  Raises
    OmrError for a stream the decoder refuses (-213), a malformed one (-5) or one above the size limits (-215)."""
    b = _buf(stream)
    v = [C.c_int32() for _ in range(6)]
    check(lib().omr_tiff_info(b.ctypes.data, b.size, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def info_ex(stream):
    """omr_tiff_info_ex -> info's six values and (bits_per_sample, samples_per_pixel, predictor)"""
    b = _buf(stream)
    v = [C.c_int32() for _ in range(9)]
    check(lib().omr_tiff_info_ex(b.ctypes.data, b.size, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def code_tables(black):
    """omr_tiff_code_tables -> [(run, code, bits)]: the T.4 run-length codes of one colour as the decoder holds them"""
    run, code, bits = (np.zeros(OMR_TIFF_CODES, np.int32) for _ in range(3))
    check(lib().omr_tiff_code_tables(int(bool(black)), run.ctypes.data_as(i32p), code.ctypes.data_as(i32p), bits.ctypes.data_as(i32p)))
    return [(int(r), int(c), int(b)) for r, c, b in zip(run, code, bits)]


def decode(stream, channels=3):
    """omr_tiff_decode: imread of one buffer -> (rows, cols) for channels = 1, (rows, cols, 3) BGR for channels = 3.  An
    RGB file asked for as gray raises OmrError (-213)."""
    b = _buf(stream)
    out = OmrImageOwned()
    check(lib().omr_tiff_decode(b.ctypes.data, b.size, int(channels), C.byref(out)))
    return _take_owned(out)


def decode_batch_device(streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols):
    """omr_tiff_decode_batch_device: host streams -> device-resident images, image i at the top left of the slot at
    d_out + i * out_stride_bytes (d_out: a device address).  Returns (out_size int32 [n, 2], rc int32 [n]): the images'
    (rows, cols), 0 x 0 where rc[i] != 0.  Synchronous."""
    return _codec.decode_batch_device(lib().omr_tiff_decode_batch_device, streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols)


STAGES = ("upload", "PackBits", "T.6", "unpack")


def stats(enable=True):
    """omr_tiff_decode_stats (measurement aid): what this thread's last decode took -> (groups, [ms per stage of STAGES]);
    then switches the collection on or off for the thread's next decodes."""
    return _codec.stage_stats(lib().omr_tiff_decode_stats, STAGES, enable)


STAGES_EX = ("upload", "PackBits", "T.6", "LZW", "unpack", "finish8")


def stats_ex(enable=True):
    """omr_tiff_decode_stats_ex: stats with every stage -> (groups, [ms per stage of STAGES_EX])"""
    groups, stages = C.c_int32(), C.c_int32()
    ms = np.zeros(len(STAGES_EX), np.float64)
    check(lib().omr_tiff_decode_stats_ex(int(bool(enable)), C.byref(groups), ms.ctypes.data_as(C.POINTER(C.c_double)), ms.size,
                                         C.byref(stages)))
    assert stages.value == len(STAGES_EX)
    return groups.value, [float(v) for v in ms]


def bound(rows, cols, rows_per_strip=0):
    """omr_tiff_bound: an upper bound of the encoded file's length in bytes"""
    out = C.c_int64()
    check(lib().omr_tiff_bound(int(rows), int(cols), int(rows_per_strip), C.byref(out)))
    return out.value


def encode_batch_device(d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, d_out, out_stride_bytes,
                        threshold=127, rows_per_strip=0, dpi=0):
    """omr_tiff_encode_batch_device: n device-resident images in slots of rows x cols x channels (d_imgs, d_out: device
    addresses; sizes: None or int32 [n, 2] of (rows, cols) per image) -> Group 4 TIFF files; a pixel is white iff its gray
    value is above `threshold`.  Returns out_len int64 [n]: file i is out_len[i] bytes at d_out + i * out_stride_bytes
    (0: a 0 x 0 entry, slot untouched).  Synchronous."""
    return _codec.encode_batch_device(lib().omr_tiff_encode_batch_device, d_imgs, img_stride_bytes, step_bytes, rows, cols, channels,
                                      sizes, n, d_out, out_stride_bytes, threshold, rows_per_strip, dpi)


def encode(mat, threshold=127, rows_per_strip=0, dpi=0):
    """omr_tiff_encode: a host image (gray or BGR) -> a Group 4 TIFF file as bytes, its strips libtiff's for the picture
    thresholded at `threshold`.  One call in the usual case: the first buffer holds an eighth of the pixels, which pages
    stay far below; a file that does not fit answers -4 with its length, and a second call encodes into that."""
    a, im = as_image(_mat(mat))
    first = min(im.rows * im.cols // 8 + 4096, bound(im.rows, im.cols, rows_per_strip))
    return _codec.encode_retry(lib().omr_tiff_encode, im, first, threshold, rows_per_strip, dpi)


STAGES_ENC = ("threshold and pack", "row coder", "placement", "head and bit merge")


def encode_stats(enable=True):
    """omr_tiff_encode_stats (measurement aid): what this thread's last encode took -> (groups, [ms per stage of
    STAGES_ENC]); then switches the collection on or off for the thread's next encodes."""
    return _codec.stage_stats(lib().omr_tiff_encode_stats, STAGES_ENC, enable)


def bound8(rows, cols, channels=1, compression=5, rows_per_strip=0):
    """omr_tiff8_bound: an upper bound of the 8-bit file's length in bytes"""
    out = C.c_int64()
    check(lib().omr_tiff8_bound(int(rows), int(cols), int(channels), int(compression), int(rows_per_strip), C.byref(out)))
    return out.value


def encode8_batch_device(d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, d_out, out_stride_bytes,
                         compression=5, predictor=1, rows_per_strip=0, dpi=0):
    """omr_tiff8_encode_batch_device: n device-resident images in slots of rows x cols x channels (d_imgs, d_out: device
    addresses; sizes: None or int32 [n, 2] of (rows, cols) per image) -> 8-bit TIFF files, gray or RGB, uncompressed
    (compression 1) or LZW (5).  Returns out_len int64 [n]: file i is out_len[i] bytes at d_out + i * out_stride_bytes
    (0: a 0 x 0 entry, slot untouched).  Synchronous."""
    return _codec.encode_batch_device(lib().omr_tiff8_encode_batch_device, d_imgs, img_stride_bytes, step_bytes, rows, cols, channels,
                                      sizes, n, d_out, out_stride_bytes, compression, predictor, rows_per_strip, dpi)


def encode8(mat, compression=5, predictor=1, rows_per_strip=0, dpi=0):
    """omr_tiff8_encode: a host image (gray or BGR) -> an 8-bit TIFF file as bytes that decodes to the image exactly.  One
    call in the usual case: the first buffer holds the raw pixels and a page of head, which LZW passes only on noise; a file
    that does not fit answers -4 with its length, and a second call encodes into that."""
    a, im = as_image(_mat(mat))
    first = im.rows * im.cols * im.channels + 4096 + 8 * im.rows
    return _codec.encode_retry(lib().omr_tiff8_encode, im, first, compression, predictor, rows_per_strip, dpi)


STAGES_ENC8 = ("staging", "LZW", "placement", "head and strips")


def encode8_stats(enable=True):
    """omr_tiff8_encode_stats (measurement aid): what this thread's last 8-bit encode took -> (groups, [ms per stage of
    STAGES_ENC8]); then switches the collection on or off for the thread's next encodes."""
    return _codec.stage_stats(lib().omr_tiff8_encode_stats, STAGES_ENC8, enable)
