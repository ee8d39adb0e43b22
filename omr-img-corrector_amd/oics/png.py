"""PNG on the device (omr_png_*): decoding byte for byte what imread returns, and a lossless, deterministic encoder."""
import ctypes as C

from . import _codec
from ._codec import _buf
from ._lib import check, lib
from ._lib import OmrImageOwned
from .transfer import _mat, _take_owned, as_image


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
    return _codec.decode_batch_device(lib().omr_png_decode_batch_device, streams, channels, d_out, out_stride_bytes, step_bytes, rows, cols)


STAGES = ("upload", "inflate", "Adler-32", "unfilter and convert")


def stats(enable=True):
    """omr_png_decode_stats (measurement aid): what this thread's last decode took -> (groups, [ms per stage of STAGES]);
    then switches the collection on or off for the thread's next decodes."""
    return _codec.stage_stats(lib().omr_png_decode_stats, STAGES, enable)


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
    return _codec.encode_batch_device(lib().omr_png_encode_batch_device, d_imgs, img_stride_bytes, step_bytes, rows, cols, channels,
                                      sizes, n, d_out, out_stride_bytes, compression)


def encode(mat, compression=1):
    """omr_png_encode: a host image (gray, BGR or BGRA) -> the stream as bytes.  One call in the usual case: the first
    buffer holds half the raw image's size, which sheets stay below; a stream that does not fit answers -4 with its
    length, and a second call encodes again into a buffer of that length."""
    a, im = as_image(_mat(mat))
    first = min(im.rows * im.cols * im.channels // 2 + 1024, bound(im.rows, im.cols, im.channels))
    return _codec.encode_retry(lib().omr_png_encode, im, first, compression)


STAGES_ENC = ("filter", "Adler-32", "matches and parse", "code sets and placement", "bit writer", "copy, CRC-32 and wrap")


def encode_stats(enable=True):
    """omr_png_encode_stats (measurement aid): what this thread's last encode took -> (groups, [ms per stage of
    STAGES_ENC]); then switches the collection on or off for the thread's next encodes."""
    return _codec.stage_stats(lib().omr_png_encode_stats, STAGES_ENC, enable)
