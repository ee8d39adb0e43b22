"""imread on the device (omr_imread_*): JPEG, PNG or TIFF (bilevel, 8-bit gray or RGB; see oics.tiff) file contents -> what imread(IMREAD_COLOR) returns, a JPEG turned by
its EXIF orientation as imread does."""
import ctypes as C

import numpy as np

from ._lib import OMR_IMREAD_IGNORE_ORIENTATION, OMR_IMREAD_KIND_JPEG, OMR_IMREAD_KIND_PNG, OMR_IMREAD_KIND_TIFF  # noqa: F401
from ._lib import OmrImageOwned, check, i32p, lib
from .transfer import _take_owned

IGNORE_ORIENTATION = OMR_IMREAD_IGNORE_ORIENTATION


def _buf(stream):
    return np.frombuffer(bytes(stream), np.uint8)


def info(stream, flags=0):
    """omr_imread_info -> (rows, cols, components, orientation, kind): the size imread returns (after the turn, unless
    flags = IGNORE_ORIENTATION), the components as stored, the EXIF orientation found (1: none) and OMR_IMREAD_KIND_JPEG,
    _PNG or _TIFF.  Raises OmrError for a stream its decoder refuses (-213) or a malformed header (-5)."""
    b = _buf(stream)
    r, c, n, o, k = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().omr_imread_info(b.ctypes.data, b.size, int(flags), C.byref(r), C.byref(c), C.byref(n), C.byref(o), C.byref(k)))
    return r.value, c.value, n.value, o.value, k.value


def decode(stream, channels=3, flags=0):
    """omr_imread: imread of one buffer -> (rows, cols) for channels = 1, (rows, cols, 3) BGR for channels = 3."""
    b = _buf(stream)
    out = OmrImageOwned()
    check(lib().omr_imread(b.ctypes.data, b.size, int(channels), int(flags), C.byref(out)))
    return _take_owned(out)


def decode_batch_device(streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols, flags=0):
    """omr_imread_batch_device: host streams (JPEG, PNG and TIFF, mixed) -> device-resident images, image i at the top left of
    the slot at d_out + i * out_stride_bytes (d_out: a device address).  Returns (out_size int32 [n, 2], rc int32 [n]):
    the images' (rows, cols) as imread returns them, 0 x 0 where rc[i] != 0.  Synchronous."""
    bufs = [_buf(s) for s in streams]
    n = len(bufs)
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = np.array([b.size for b in bufs], np.int64)
    out_size, rc = np.zeros((max(n, 1), 2), np.int32), np.zeros(max(n, 1), np.int32)
    check(lib().omr_imread_batch_device(ptrs, lens.ctypes.data_as(C.POINTER(C.c_int64)), n, int(channels), int(flags), d_out,
                                        int(out_stride_bytes), int(step_bytes), int(rows), int(cols),
                                        out_size.ctypes.data_as(i32p), rc.ctypes.data_as(i32p)))
    return out_size[:n], rc[:n]
