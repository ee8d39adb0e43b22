"""Baseline JPEG on the device (omr_jpeg_*): encoding byte for byte what imwrite(.., JPEG, quality) writes, decoding
byte for byte what imread returns."""
import ctypes as C

import numpy as np

from . import _codec
from ._codec import _buf
from ._lib import check, lib
from ._lib import OmrImageOwned
from .transfer import _mat, _take_owned, as_image


def quant_tables(quality):
    """omr_jpeg_quant_tables -> (luma, chroma), uint16 [64] each, natural order"""
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    u16p = C.POINTER(C.c_uint16)
    check(lib().omr_jpeg_quant_tables(int(quality), luma.ctypes.data_as(u16p), chroma.ctypes.data_as(u16p)))
    return luma, chroma


def bound(rows, cols, channels):
    """omr_jpeg_bound: an upper bound of the stream's length in bytes"""
    out = C.c_int64()
    check(lib().omr_jpeg_bound(int(rows), int(cols), int(channels), C.byref(out)))
    return out.value


def encode_batch_device(d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, quality, d_out,
                        out_stride_bytes):
    """omr_jpeg_encode_batch_device: n device-resident images in slots of rows x cols x channels (d_imgs, d_out: device
    addresses; sizes: None or int32 [n, 2] of (rows, cols) per image).  Returns out_len int64 [n]: stream i is
    out_len[i] bytes at d_out + i * out_stride_bytes (0: a 0 x 0 entry, slot untouched).  Synchronous."""
    return _codec.encode_batch_device(lib().omr_jpeg_encode_batch_device, d_imgs, img_stride_bytes, step_bytes, rows, cols, channels,
                                      sizes, n, d_out, out_stride_bytes, quality)


def encode(mat, quality=100):
    """omr_jpeg_encode: a host image (gray or BGR) -> the stream as bytes.  One call in the usual case: the first buffer
    holds the raw image's size plus the header, which all but noise at the highest qualities stays below; a stream that
    does not fit answers -4 with its length, and a second call encodes again into a buffer of that length."""
    a, im = as_image(_mat(mat))
    first = min(im.rows * im.cols * im.channels + 1024, bound(im.rows, im.cols, im.channels))
    return _codec.encode_retry(lib().omr_jpeg_encode, im, first, quality)


def info(stream):
    """omr_jpeg_info -> (rows, cols, components, sampling): what the header says (sampling: Y's factors as in SOF, 0x11,
    0x21 or 0x22).  Raises OmrError for a stream the decoder refuses (-213) or a malformed header (-5)."""
    b = _buf(stream)
    r, c, n, sm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().omr_jpeg_info(b.ctypes.data, b.size, C.byref(r), C.byref(c), C.byref(n), C.byref(sm)))
    return r.value, c.value, n.value, sm.value


def decode(stream, channels=3):
    """omr_jpeg_decode: imread of one buffer -> (rows, cols) for channels = 1, (rows, cols, 3) BGR for channels = 3."""
    b = _buf(stream)
    out = OmrImageOwned()
    check(lib().omr_jpeg_decode(b.ctypes.data, b.size, int(channels), C.byref(out)))
    return _take_owned(out)


def decode_batch(streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols):
    """omr_jpeg_decode_batch_device: host streams -> device-resident images, image i at the top left of the slot at
    d_out + i * out_stride_bytes (d_out: a device address).  Returns (out_size int32 [n, 2], rc int32 [n]): the images'
    (rows, cols), 0 x 0 where rc[i] != 0.  Synchronous."""
    return _codec.decode_batch_device(lib().omr_jpeg_decode_batch_device, streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols)


STAGES = ("upload and clearing", "un-stuffing", "synchronisation rounds", "coefficients", "inverse DCT", "colour")


def decode_stats(enable=True):
    """omr_jpeg_decode_stats (measurement aid): what this thread's last decode took -> (sub_bits, groups, rounds,
    [ms per stage of STAGES]); then switches the collection on or off for the thread's next decodes."""
    bits, groups, rounds = C.c_int32(), C.c_int32(), C.c_int32()
    ms = np.zeros(len(STAGES), np.float64)
    check(lib().omr_jpeg_decode_stats(int(bool(enable)), C.byref(bits), C.byref(groups), C.byref(rounds),
                                      ms.ctypes.data_as(C.POINTER(C.c_double))))
    return bits.value, groups.value, rounds.value, [float(v) for v in ms]
