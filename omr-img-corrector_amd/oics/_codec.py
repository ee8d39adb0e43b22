"""What the codec modules (jpeg, png, tiff) share: the calls of an omr_*_decode_batch_device, an omr_*_encode_batch_device,
an omr_*_encode with its second try, and an omr_*_stats.  `fn` is the bound library function."""
import ctypes as C

import numpy as np

from ._lib import check, i32p, u8p

i64p = C.POINTER(C.c_int64)


def _buf(stream):
    return np.frombuffer(bytes(stream), np.uint8)


def decode_batch_device(fn, streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols):
    """host streams -> device-resident images in slots; returns (out_size int32 [n, 2], rc int32 [n])"""
    bufs = [_buf(s) for s in streams]
    n = len(bufs)
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = np.array([b.size for b in bufs], np.int64)
    out_size, rc = np.zeros((max(n, 1), 2), np.int32), np.zeros(max(n, 1), np.int32)
    check(fn(ptrs, lens.ctypes.data_as(i64p), n, int(channels), d_out, int(out_stride_bytes), int(step_bytes), int(rows),
             int(cols), out_size.ctypes.data_as(i32p), rc.ctypes.data_as(i32p)))
    return out_size[:n], rc[:n]


def stage_stats(fn, names, enable=True):
    """what this thread's last call of the codec took -> (groups, [ms per stage of names])"""
    groups = C.c_int32()
    ms = np.zeros(len(names), np.float64)
    check(fn(int(bool(enable)), C.byref(groups), ms.ctypes.data_as(C.POINTER(C.c_double))))
    return groups.value, [float(v) for v in ms]


def encode_batch_device(fn, d_imgs, img_stride_bytes, step_bytes, rows, cols, channels, sizes, n, d_out, out_stride_bytes,
                        *params):
    """n device-resident images in slots -> their streams in slots; params: the codec's own, between n and d_out.  Returns
    out_len int64 [n]"""
    n = int(n)
    out_len = np.zeros(max(n, 0), np.int64)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
    check(fn(d_imgs, int(img_stride_bytes), int(step_bytes), int(rows), int(cols), int(channels),
             None if sz is None else sz.ctypes.data_as(i32p), n, *[int(p) for p in params], d_out, int(out_stride_bytes),
             out_len.ctypes.data_as(i64p)))
    return out_len


def encode_retry(fn, im, first_cap, *params):
    """one host image (an OmrImage) -> its stream as bytes: into a buffer of first_cap bytes, and where that answers -4
    with the stream's length, again into a buffer of that length"""
    n = C.c_int64()
    args = [int(p) for p in params]
    buf = np.empty(int(first_cap), np.uint8)
    rc = fn(C.byref(im), *args, buf.ctypes.data_as(u8p), buf.size, C.byref(n))
    if rc == -4:
        buf = np.empty(n.value, np.uint8)
        rc = fn(C.byref(im), *args, buf.ctypes.data_as(u8p), buf.size, C.byref(n))
    check(rc)
    return buf[: n.value].tobytes()
