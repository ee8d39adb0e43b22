"""PNG on the device (omr_png_*): decoding byte for byte what imread returns, and a lossless, deterministic encoder."""
import ctypes as C

import numpy as np

from ._lib import check, i32p, lib, u8p
from ._lib import OmrImageOwned
from .transfer import _mat, _take_owned, as_image


def _buf(stream):
    return np.frombuffer(bytes(stream), np.uint8)


def info(stream):
    """omr_png_info -> (rows, cols, color_type, bit_depth): what IHDR says.  Raises OmrError for a stream the decoder
    refuses (-213), a malformed one (-5) or one without IEND (-215)."""
    b = _buf(stream)
    r, c, ct, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().omr_png_info(b.ctypes.data, b.size, C.byref(r), C.byref(c), C.byref(ct), C.byref(d)))
    return r.value, c.value, ct.value, d.value


def decode(stream, channels=3):
    """omr_png_decode: imread of one buffer -> (rows, cols) for channels = 1, (rows, cols, 3) BGR for channels = 3."""
    b = _buf(stream)
    out = OmrImageOwned()
    check(lib().omr_png_decode(b.ctypes.data, b.size, int(channels), C.byref(out)))
    return _take_owned(out)


def decode_batch_device(streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols):
    """omr_png_decode_batch_device: host streams -> device-resident images, image i at the top left of the slot at
    d_out + i * out_stride_bytes (d_out: a device address).  Returns (out_size int32 [n, 2], rc int32 [n]): the images'
    (rows, cols), 0 x 0 where rc[i] != 0.  Synchronous."""
    bufs = [_buf(s) for s in streams]
    n = len(bufs)
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = np.array([b.size for b in bufs], np.int64)
    out_size, rc = np.zeros((max(n, 1), 2), np.int32), np.zeros(max(n, 1), np.int32)
    check(lib().omr_png_decode_batch_device(ptrs, lens.ctypes.data_as(C.POINTER(C.c_int64)), n, int(channels), d_out,
                                            int(out_stride_bytes), int(step_bytes), int(rows), int(cols),
                                            out_size.ctypes.data_as(i32p), rc.ctypes.data_as(i32p)))
    return out_size[:n], rc[:n]


STAGES = ("upload", "inflate", "Adler-32", "unfilter and convert")


def stats(enable=True):
    """omr_png_decode_stats (measurement aid): what this thread's last decode took -> (groups, [ms per stage of STAGES]);
    then switches the collection on or off for the thread's next decodes."""
    groups = C.c_int32()
    ms = np.zeros(len(STAGES), np.float64)
    check(lib().omr_png_decode_stats(int(bool(enable)), C.byref(groups), ms.ctypes.data_as(C.POINTER(C.c_double))))
    return groups.value, [float(v) for v in ms]


def bound(rows, cols, channels):
    """omr_png_bound: an upper bound of the stream's length in bytes"""
    out = C.c_int64()
    check(lib().omr_png_bound(int(rows), int(cols), int(channels), C.byref(out)))
    return out.value


def encode_batch_device(d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, compression, d_out,
                        out_stride_bytes):
    """omr_png_encode_batch_device: n device-resident images in slots of rows x cols x channels (d_imgs, d_out: device
    addresses; sizes: None or int32 [n, 2] of (rows, cols) per image).  Returns out_len int64 [n]: stream i is
    out_len[i] bytes at d_out + i * out_stride_bytes (0: a 0 x 0 entry, slot untouched).  Synchronous."""
    n = int(n)
    out_len = np.zeros(max(n, 0), np.int64)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
    check(lib().omr_png_encode_batch_device(d_imgs, int(img_stride_bytes), int(step_bytes), int(rows), int(cols),
                                            int(channels), None if sz is None else sz.ctypes.data_as(i32p), n,
                                            int(compression), d_out, int(out_stride_bytes),
                                            out_len.ctypes.data_as(C.POINTER(C.c_int64))))
    return out_len


def encode(mat, compression=1):
    """omr_png_encode: a host image (gray, BGR or BGRA) -> the stream as bytes.  One call in the usual case: the first
    buffer holds half the raw image's size, which sheets stay below; a stream that does not fit answers -4 with its
    length, and a second call encodes again into a buffer of that length."""
    a, im = as_image(_mat(mat))
    n = C.c_int64()
    L = lib()
    buf = np.empty(min(im.rows * im.cols * im.channels // 2 + 1024, bound(im.rows, im.cols, im.channels)), np.uint8)
    rc = L.omr_png_encode(C.byref(im), int(compression), buf.ctypes.data_as(u8p), buf.size, C.byref(n))
    if rc == -4:
        buf = np.empty(n.value, np.uint8)
        rc = L.omr_png_encode(C.byref(im), int(compression), buf.ctypes.data_as(u8p), buf.size, C.byref(n))
    check(rc)
    return buf[: n.value].tobytes()


STAGES_ENC = ("filter", "Adler-32", "matches and parse", "code sets and placement", "bit writer", "copy, CRC-32 and wrap")


def encode_stats(enable=True):
    """omr_png_encode_stats (measurement aid): what this thread's last encode took -> (groups, [ms per stage of
    STAGES_ENC]); then switches the collection on or off for the thread's next encodes."""
    groups = C.c_int32()
    ms = np.zeros(len(STAGES_ENC), np.float64)
    check(lib().omr_png_encode_stats(int(bool(enable)), C.byref(groups), ms.ctypes.data_as(C.POINTER(C.c_double))))
    return groups.value, [float(v) for v in ms]
