"""PNG on the device (omr_png_*): decoding byte for byte what imread returns."""
import ctypes as C

import numpy as np

from ._lib import check, i32p, lib
from ._lib import OmrImageOwned
from .transfer import _take_owned


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
