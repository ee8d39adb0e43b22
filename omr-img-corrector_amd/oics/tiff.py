"""Bilevel TIFF on the device (omr_tiff_*): uncompressed, PackBits and CCITT Group 4 strips decoded byte for byte to what
libtiff gives, as 255 / 0."""
import ctypes as C

import numpy as np

from ._lib import OMR_TIFF_CODES, OmrImageOwned, check, i32p, lib
from .transfer import _take_owned


def _buf(stream):
    return np.frombuffer(bytes(stream), np.uint8)


def info(stream):
    """omr_tiff_info -> (rows, cols, compression, photometric, fill_order, strips): what the first IFD says.  Raises
    OmrError for a stream the decoder refuses (-213), a malformed one (-5) or one above the size limits (-215)."""
    b = _buf(stream)
    v = [C.c_int32() for _ in range(6)]
    check(lib().omr_tiff_info(b.ctypes.data, b.size, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def code_tables(black):
    """omr_tiff_code_tables -> [(run, code, bits)]: the T.4 run-length codes of one colour as the decoder holds them"""
    run, code, bits = (np.zeros(OMR_TIFF_CODES, np.int32) for _ in range(3))
    check(lib().omr_tiff_code_tables(int(bool(black)), run.ctypes.data_as(i32p), code.ctypes.data_as(i32p), bits.ctypes.data_as(i32p)))
    return [(int(r), int(c), int(b)) for r, c, b in zip(run, code, bits)]


def decode(stream, channels=3):
    """omr_tiff_decode: imread of one buffer -> (rows, cols) for channels = 1, (rows, cols, 3) BGR for channels = 3."""
    b = _buf(stream)
    out = OmrImageOwned()
    check(lib().omr_tiff_decode(b.ctypes.data, b.size, int(channels), C.byref(out)))
    return _take_owned(out)


def decode_batch_device(streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols):
    """omr_tiff_decode_batch_device: host streams -> device-resident images, image i at the top left of the slot at
    d_out + i * out_stride_bytes (d_out: a device address).  Returns (out_size int32 [n, 2], rc int32 [n]): the images'
    (rows, cols), 0 x 0 where rc[i] != 0.  Synchronous."""
    bufs = [_buf(s) for s in streams]
    n = len(bufs)
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = np.array([b.size for b in bufs], np.int64)
    out_size, rc = np.zeros((max(n, 1), 2), np.int32), np.zeros(max(n, 1), np.int32)
    check(lib().omr_tiff_decode_batch_device(ptrs, lens.ctypes.data_as(C.POINTER(C.c_int64)), n, int(channels), d_out,
                                             int(out_stride_bytes), int(step_bytes), int(rows), int(cols),
                                             out_size.ctypes.data_as(i32p), rc.ctypes.data_as(i32p)))
    return out_size[:n], rc[:n]


STAGES = ("upload", "PackBits", "T.6", "unpack")


def stats(enable=True):
    """omr_tiff_decode_stats (measurement aid): what this thread's last decode took -> (groups, [ms per stage of STAGES]);
    then switches the collection on or off for the thread's next decodes."""
    groups = C.c_int32()
    ms = np.zeros(len(STAGES), np.float64)
    check(lib().omr_tiff_decode_stats(int(bool(enable)), C.byref(groups), ms.ctypes.data_as(C.POINTER(C.c_double))))
    return groups.value, [float(v) for v in ms]
