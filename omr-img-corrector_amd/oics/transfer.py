"""oics::transfer (packages/lib/src/transfer.rs) through the C ABI.

`TransformableMatrix` wraps a numpy u8 array the way the reference wraps a cv::Mat
(transfer.rs:16-18); every helper returns a fresh object, like the reference's.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OmrImage, OmrImageOwned, check, f64p, lib, u8p
from .types import RotateClipStrategy

INTER_NEAREST = 0  # == imgproc::WARP_POLAR_LINEAR's numeric value, what the reference passes
INTER_LINEAR = 1
INTER_CUBIC = _lib.OMR_INTER_CUBIC
INTER_AREA = _lib.OMR_INTER_AREA
INTER_LANCZOS4 = _lib.OMR_INTER_LANCZOS4
WARP_FILL_OUTLIERS = _lib.OMR_WARP_FILL_OUTLIERS
WARP_INVERSE_MAP = _lib.OMR_WARP_INVERSE_MAP
BORDER_CONSTANT = _lib.OMR_BORDER_CONSTANT
BORDER_REPLICATE = _lib.OMR_BORDER_REPLICATE
BORDER_REFLECT = _lib.OMR_BORDER_REFLECT
BORDER_WRAP = _lib.OMR_BORDER_WRAP
BORDER_REFLECT_101 = _lib.OMR_BORDER_REFLECT_101
BORDER_TRANSPARENT = _lib.OMR_BORDER_TRANSPARENT
MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = _lib.OMR_MORPH_RECT, _lib.OMR_MORPH_CROSS, _lib.OMR_MORPH_ELLIPSE


def as_image(a):
    """numpy [rows, cols] or [rows, cols, cn] u8 -> (keep-alive array, OmrImage)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 2:
        rows, cols, cn = a.shape[0], a.shape[1], 1
    elif a.ndim == 3:
        rows, cols, cn = a.shape
    else:
        raise ValueError("image must be 2-D or 3-D")
    return a, OmrImage(a.ctypes.data, rows, cols, cn, a.strides[0] if rows else cols * cn)


class TransformableMatrix:
    def __init__(self, matrix):
        self.matrix = np.ascontiguousarray(matrix, dtype=np.uint8)

    @classmethod
    def from_matrix(cls, mat):
        return cls(np.array(mat, dtype=np.uint8, copy=True))  # transfer.rs:55-59 deep clone

    @classmethod
    def from_jpeg_bytes(cls, stream, channels=3):
        """What im_read gives for a file with these bytes (transfer.rs:147-167), decoded on the GPU (omr_jpeg_decode)."""
        from . import jpeg
        return cls(jpeg.decode(stream, channels))

    @classmethod
    def from_png_bytes(cls, stream, channels=3):
        """What im_read gives for a PNG file with these bytes, decoded on the GPU (omr_png_decode)."""
        from . import png
        return cls(png.decode(stream, channels))

    @classmethod
    def from_tiff_bytes(cls, stream, channels=3):
        """What im_read gives for a TIFF file (bilevel, 8-bit gray or RGB) with these bytes, decoded on the GPU (omr_tiff_decode)."""
        from . import tiff
        return cls(tiff.decode(stream, channels))

    def encode_jpeg(self, quality=100):
        """The bytes im_write(.., JPEG, quality) puts into its file (transfer.rs:169-186), encoded on the GPU
        (omr_jpeg_encode): gray or BGR."""
        from . import jpeg
        return jpeg.encode(self.matrix, quality)

    def encode_png(self, compression=1):
        """A PNG stream that decodes to this image exactly (im_write(.., PNG, level), transfer.rs:162-179), encoded on
        the GPU (omr_png_encode): gray, BGR or BGRA.  Lossless and deterministic, not imwrite's bytes."""
        from . import png
        return png.encode(self.matrix, compression)

    def encode_tiff(self, threshold=127, rows_per_strip=0, dpi=0):
        """A Group 4 TIFF file of the matrix thresholded at `threshold` (white above it), encoded on the GPU
        (omr_tiff_encode): gray or BGR.  The strips are byte for byte what libtiff writes for that picture."""
        from . import tiff
        return tiff.encode(self.matrix, threshold, rows_per_strip, dpi)

    def encode_tiff8(self, compression=5, predictor=1, rows_per_strip=0, dpi=0):
        """The image as an 8-bit TIFF file, gray or RGB, uncompressed (1) or LZW (5), encoded on the GPU (omr_tiff8_encode).
        It decodes to the image exactly."""
        from . import tiff
        return tiff.encode8(self.matrix, compression, predictor, rows_per_strip, dpi)

    def get_mat(self):
        return self.matrix

    def clone(self):
        return TransformableMatrix.from_matrix(self.matrix)

    # the three in-place resizers return self like the reference's `&mut Self` chain (transfer.rs:66-145)
    def scale_self(self, scale):
        """transfer.rs:66-91: INTER_LINEAR when scale > 1, INTER_AREA otherwise, size truncated `as i32`"""
        if scale == 1.0:
            return self
        self.matrix = _owned_call(lib().omr_scale, self.matrix, C.c_double(float(scale)))
        return self

    def shrink_to(self, max_width, max_height):
        """transfer.rs:93-126: never enlarges"""
        self.matrix = _owned_call(lib().omr_shrink_to, self.matrix, C.c_int32(int(max_width)), C.c_int32(int(max_height)))
        return self

    def resize_self(self, width, height):
        """transfer.rs:128-145: INTER_AREA to (width, height)"""
        self.matrix = _owned_call(lib().omr_resize, self.matrix, C.c_int32(int(width)), C.c_int32(int(height)))
        return self

    def dilate(self, kernel_shape, kernel_size, anchor, iterations):
        """transfer.rs:206-231: dilate with get_structuring_element(kernel_shape, kernel_size = (w, h), anchor = (x, y)),
        BORDER_CONSTANT and the default border value; returns a new object"""
        return self._morph(_lib.OMR_MORPH_DILATE, kernel_shape, kernel_size, anchor, iterations)

    def erode(self, kernel_shape, kernel_size, anchor, iterations):
        """transfer.rs:254-277: erode, same parameters"""
        return self._morph(_lib.OMR_MORPH_ERODE, kernel_shape, kernel_size, anchor, iterations)

    def _morph(self, op, kernel_shape, kernel_size, anchor, iterations):
        (kw, kh), (ax, ay) = kernel_size, anchor
        args = [C.c_int32(int(v)) for v in (op, kernel_shape, kw, kh, ax, ay, iterations)]
        return TransformableMatrix(_owned_call(lib().omr_morph, self.matrix, *args))


def get_structuring_element(shape, size, anchor=(-1, -1)):
    """imgproc::get_structuring_element(shape, Size(w, h), Point(x, y)) -> (h, w) uint8 mask of 0 / 1 (host only)"""
    (kw, kh), (ax, ay) = size, anchor
    out = np.zeros((max(int(kh), 0), max(int(kw), 0)), np.uint8)
    check(lib().omr_structuring_element(int(shape), int(kw), int(kh), int(ax), int(ay), out.ctypes.data_as(u8p)))
    return out


def _take_owned(out):
    try:
        shape = (out.rows, out.cols) if out.channels == 1 else (out.rows, out.cols, out.channels)
        n = out.rows * out.step_bytes
        return np.frombuffer((C.c_uint8 * n).from_address(out.data), np.uint8).reshape(shape).copy()
    finally:
        lib().omr_image_free(C.byref(out))


def _owned_call(fn, mat, *args):
    a, im = as_image(mat)
    out = OmrImageOwned()
    check(fn(C.byref(im), *args, C.byref(out)))
    return _take_owned(out)


def _mat(src):
    return src.matrix if isinstance(src, TransformableMatrix) else np.asarray(src)


def transfer_rgb_image_to_gray_image(src):
    """transfer.rs:283-290"""
    a, im = as_image(_mat(src))
    out = np.empty((im.rows, im.cols), np.uint8)
    check(lib().omr_rgb_to_gray(C.byref(im), out.ctypes.data_as(u8p), out.strides[0]))
    return TransformableMatrix(out)


def rgb_to_gray_batch(d_src, n, src_stride_bytes, src_step, rows, cols, channels, d_dst, dst_stride_bytes, dst_step, stream=None):
    """omr_rgb_to_gray_batch_device: transfer_rgb_image_to_gray_image of n same-shape device-resident scans of 3 or 4
    channels (d_src, d_dst: device addresses as ints) in one launch, scan i at d_src + i * src_stride_bytes, its gray image
    at d_dst + i * dst_stride_bytes; byte for byte the per-call conversion, any alignment and pitch.  Enqueues only."""
    check(lib().omr_rgb_to_gray_batch_device(C.c_void_p(int(d_src)) if d_src else None, int(n), int(src_stride_bytes), int(src_step),
                                             int(rows), int(cols), int(channels), C.c_void_p(int(d_dst)) if d_dst else None,
                                             int(dst_stride_bytes), int(dst_step), C.c_void_p(int(stream)) if stream else None))


def detector_deskew_canvas(rows, cols, clip_strategy=RotateClipStrategy.CONTAIN):
    """omr_detector_deskew_canvas (host only): (max_rows, max_cols), the slot that holds rotate_mat's canvas of a rows x
    cols image at any angle -- what hough.deskew_device / fft.deskew_device ask of every output slot."""
    mr, mc = C.c_int32(), C.c_int32()
    check(lib().omr_detector_deskew_canvas(int(rows), int(cols), int(clip_strategy), C.byref(mr), C.byref(mc)))
    return mr.value, mc.value


def _detector_deskew_device(symbol, detector_args, d_scans, n, scan_stride_bytes, rows, cols, channels, step_bytes, flags,
                            border_mode, border_value, clip_strategy, d_out, out_stride_bytes, out_step_bytes, stream):
    """omr_hough_deskew_batch_device / omr_fft_deskew_batch_device -> (angles, rc, n_lines, sizes)"""
    n = int(n)
    angles = np.zeros(max(n, 1), np.float64)
    rc = np.zeros(max(n, 1), np.int32)
    n_lines = np.zeros(max(n, 1), np.int32)
    sizes = np.zeros((max(n, 1), 2), np.int32)
    b = np.array([int(v) for v in border_value], np.uint8)
    check(getattr(lib(), symbol)(C.c_void_p(int(d_scans)) if d_scans else None, n, int(scan_stride_bytes), int(rows), int(cols),
                                 int(channels), int(step_bytes), *[float(v) for v in detector_args], int(flags), int(border_mode),
                                 b.ctypes.data_as(u8p), int(clip_strategy), C.c_void_p(int(d_out)) if d_out else None,
                                 int(out_stride_bytes), int(out_step_bytes), sizes.ctypes.data_as(_lib.i32p),
                                 angles.ctypes.data_as(f64p), rc.ctypes.data_as(_lib.i32p), n_lines.ctypes.data_as(_lib.i32p),
                                 C.c_void_p(int(stream)) if stream else None))
    return angles[:n], rc[:n], n_lines[:n], sizes[:n]


def _detector_deskew(symbol, detector_args, srcs, flags, border_mode, border_value, clip_strategy):
    """omr_deskew_with_hough_batch / omr_deskew_with_fft_batch -> (angles, rc, [image or None])"""
    views = [as_image(_mat(s)) for s in srcs]
    n = len(views)
    ims = (OmrImage * max(n, 1))(*[v[1] for v in views])
    angles = np.zeros(max(n, 1), np.float64)
    rc = np.zeros(max(n, 1), np.int32)
    outs = (OmrImageOwned * max(n, 1))()
    b = np.array([int(v) for v in border_value], np.uint8)
    check(getattr(lib(), symbol)(ims, n, *[float(v) for v in detector_args], int(flags), int(border_mode), b.ctypes.data_as(u8p),
                                 int(clip_strategy), angles.ctypes.data_as(f64p), rc.ctypes.data_as(_lib.i32p), outs))
    return angles[:n], rc[:n], [_take_owned(outs[i]) if outs[i].data else None for i in range(n)]


def _detector_deskew_streams(symbol, detector_args, streams, channels, flags, border_mode, border_value, clip_strategy, fmt,
                             level, want_out, tiff=None):
    """omr_deskew_with_hough_batch_streams / omr_deskew_with_fft_batch_streams -> (angles, scan_rc, [bytes or None] or None).
    tiff = (rows_per_strip, dpi): the _tiff symbol, which takes (threshold = level, rows_per_strip, dpi) for (fmt, level);
    tiff = (predictor, rows_per_strip, dpi): the _tiff8 symbol, level = the compression"""
    how = (int(fmt), int(level)) if tiff is None else (int(level),) + tuple(int(v) for v in tiff)
    bufs = [np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray, memoryview)) else np.ascontiguousarray(s, np.uint8)
            for s in streams]
    bufs = [b if b.size else np.zeros(1, np.uint8) for b in bufs]
    n = len(bufs)
    sp = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    sl = np.array([len(s) for s in streams] + [0], np.int64)
    angles = np.zeros(max(n, 1), np.float64)
    rc = np.zeros(max(n, 1), np.int32)
    ptrs = (u8p * max(n, 1))()
    lens = np.zeros(max(n, 1), np.int64)
    b = np.array([int(v) for v in border_value], np.uint8)
    check(getattr(lib(), symbol)(sp, sl.ctypes.data_as(C.POINTER(C.c_int64)), n, int(channels), *[float(v) for v in detector_args],
                                 int(flags), int(border_mode), b.ctypes.data_as(u8p), int(clip_strategy), *how,
                                 angles.ctypes.data_as(f64p), rc.ctypes.data_as(_lib.i32p), ptrs if want_out else None,
                                 lens.ctypes.data_as(C.POINTER(C.c_int64)) if want_out else None))
    out = None
    if want_out:
        out = [None] * n
        for i in range(n):
            if ptrs[i]:
                out[i] = C.string_at(ptrs[i], int(lens[i]))
                lib().omr_bytes_free(ptrs[i])
    return angles[:n], rc[:n], out


def transfer_gray_image_to_thresh_binary(src):
    """transfer.rs:294-301"""
    a, im = as_image(_mat(src))
    out = np.empty((im.rows, im.cols), np.uint8)
    check(lib().omr_threshold_binary(C.byref(im), out.ctypes.data_as(u8p), out.strides[0]))
    return TransformableMatrix(out)


def get_horizontal_projection(src):
    """transfer.rs:305-333"""
    a, im = as_image(_mat(src))
    out = np.empty(im.rows, np.float64)
    check(lib().omr_get_horizontal_projection(C.byref(im), out.ctypes.data_as(f64p)))
    return out


def get_vertical_projection(src):
    """transfer.rs:380-405"""
    a, im = as_image(_mat(src))
    out = np.empty(im.cols, np.float64)
    check(lib().omr_get_vertical_projection(C.byref(im), out.ctypes.data_as(f64p)))
    return out


def get_projection_standard_deviations(src):
    """transfer.rs:527-536 -> (vertical sd, horizontal sd)"""
    a, im = as_image(_mat(src))
    v, h = C.c_double(), C.c_double()
    check(lib().omr_get_projection_standard_deviations(C.byref(im), C.byref(v), C.byref(h)))
    return v.value, h.value


def projection_pictures(src, horizontal=True, vertical=True):
    """omr_projection_pictures: (horizontal picture, vertical picture) of an 8-bit one-channel image of any values, each
    a TransformableMatrix of the image's size -- or None for a picture that was not asked for (not both)."""
    a, im = as_image(_mat(src))
    h, v = OmrImageOwned(), OmrImageOwned()
    check(lib().omr_projection_pictures(C.byref(im), C.byref(h) if horizontal else None, C.byref(v) if vertical else None))
    # both images are taken over before either is wrapped, so neither of the library's buffers is lost
    mats = [_take_owned(o) if want else None for o, want in ((h, horizontal), (v, vertical))]
    return tuple(None if m is None else TransformableMatrix(m) for m in mats)


def transfer_thresh_binary_to_horizontal_projection(src):
    """transfer.rs:337-376: per row, the pixels before the first 255 stay, then as many 0 as the row has pixels != 255
    in all, then 255"""
    return projection_pictures(src, vertical=False)[0]


def transfer_thresh_binary_to_vertical_projection(src):
    """transfer.rs:409-455: per column, a black bar from the bottom edge as high as the column has pixels <= 127"""
    return projection_pictures(src, horizontal=False)[1]


def projection_pictures_batch_device(d_src, n, src_stride_bytes, src_step, rows, cols, d_horizontal, h_stride_bytes, h_step,
                                     d_vertical, v_stride_bytes, v_step, stream=None):
    """omr_projection_pictures_batch_device: n same-shape device-resident one-channel scans (d_src, d_horizontal,
    d_vertical: device addresses as ints; 0 / None for a picture that is not wanted, not both), scan i's pictures at
    d_* + i * *_stride_bytes, byte for byte omr_projection_pictures_device's.  Synchronises `stream` before returning
    when the vertical picture is asked for."""
    check(lib().omr_projection_pictures_batch_device(
        C.c_void_p(int(d_src)), int(n), int(src_stride_bytes), int(src_step), int(rows), int(cols),
        C.c_void_p(int(d_horizontal)) if d_horizontal else None, int(h_stride_bytes), int(h_step),
        C.c_void_p(int(d_vertical)) if d_vertical else None, int(v_stride_bytes), int(v_step),
        C.c_void_p(int(stream)) if stream else None))


def rotate_mat(src, angle, scale, flags, border_mode=0, border_value=(255.0, 255.0, 255.0, 0.0),
               clip_strategy=RotateClipStrategy.DEFAULT):
    """transfer.rs:459-523 through omr_rotate_ex: every warpAffine flag (INTER_NEAREST / LINEAR / CUBIC / AREA /
    LANCZOS4, WARP_INVERSE_MAP, WARP_FILL_OUTLIERS) and border mode (BORDER_CONSTANT .. BORDER_TRANSPARENT; the pixels
    TRANSPARENT skips are 0)."""
    a, im = as_image(_mat(src))
    b = np.array([int(v) for v in border_value], np.uint8)
    out = OmrImageOwned()
    check(lib().omr_rotate_ex(C.byref(im), float(angle), float(scale), int(flags), int(border_mode),
                              b.ctypes.data_as(u8p), int(clip_strategy), C.byref(out)))
    try:
        shape = (out.rows, out.cols) if out.channels == 1 else (out.rows, out.cols, out.channels)
        n = out.rows * out.step_bytes
        arr = np.frombuffer((C.c_uint8 * n).from_address(out.data), np.uint8).reshape(shape).copy()
    finally:
        lib().omr_image_free(C.byref(out))
    return TransformableMatrix(arr)


def orient(src, orientation):
    """omr_orient: a gray or 3-channel image turned by an EXIF orientation code 1..8 (what imread does to a JPEG that
    carries one: OpenCV's ExifTransform, Pillow's exif_transpose) -> a new TransformableMatrix."""
    return TransformableMatrix(_owned_call(lib().omr_orient, _mat(src), C.c_int32(int(orientation))))


def orient_batch_device(d_src, src_stride_bytes, src_step, rows, cols, d_dst, dst_stride_bytes, dst_step, dst_rows, dst_cols,
                        channels, sizes, orientations):
    """omr_orient_batch_device: n device-resident images (d_src, d_dst: device addresses as ints) in slots of rows x cols,
    image i turned by orientations[i] into the top left of its slot of dst_rows x dst_cols; sizes: None (every image fills
    its slot) or int32 [n, 2].  -> out_size int32 [n, 2], the turned images' (rows, cols).  Synchronous."""
    o = np.ascontiguousarray(orientations, np.int32).reshape(-1)
    n = o.size
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
    out = np.zeros((max(n, 1), 2), np.int32)
    check(lib().omr_orient_batch_device(C.c_void_p(int(d_src)), int(src_stride_bytes), int(src_step), int(rows), int(cols),
                                        C.c_void_p(int(d_dst)), int(dst_stride_bytes), int(dst_step), int(dst_rows),
                                        int(dst_cols), int(channels), None if sz is None else sz.ctypes.data_as(_lib.i32p),
                                        o.ctypes.data_as(_lib.i32p), n, out.ctypes.data_as(_lib.i32p)))
    return out[:n]


def _angles(angles):
    a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
    return a, (a.ctypes.data_as(f64p) if a.size else None)


def rotate_batch_canvas(rows, cols, angles, clip_strategy=RotateClipStrategy.DEFAULT):
    """omr_rotate_batch_canvas (host only): -> (max_rows, max_cols, sizes), sizes[i] = (rows, cols) of the canvas
    rotate_mat gives a rows x cols image at angles[i]; every canvas fits a max_rows x max_cols slot."""
    a, ap = _angles(angles)
    mr, mc = C.c_int32(), C.c_int32()
    sizes = np.zeros((a.size, 2), np.int32)
    check(lib().omr_rotate_batch_canvas(int(rows), int(cols), ap, a.size, int(clip_strategy), C.byref(mr), C.byref(mc),
                                        sizes.ctypes.data_as(_lib.i32p) if a.size else None))
    return mr.value, mc.value, sizes


def rotate_batch_device_ex(d_src, n, src_stride_bytes, src_step, rows, cols, channels, angles, scale, flags, border_mode,
                           border_value, clip_strategy, d_dst, dst_stride_bytes, dst_step, slot_rows, slot_cols, stream=None):
    """omr_rotate_batch_device_ex: n same-shape device-resident images (d_src, d_dst: device addresses as ints), image i
    rotated by angles[i] into the top left of its slot; -> sizes[n, 2], the canvases' (rows, cols).  Image i's canvas is
    byte for byte omr_rotate_device_ex's.  Synchronises `stream` before returning when n > 3."""
    a, ap = _angles(angles)
    if a.size != int(n):
        raise ValueError("%d angles for %d images" % (a.size, int(n)))
    b = np.array([int(v) for v in border_value], np.uint8)
    sizes = np.zeros((a.size, 2), np.int32)
    check(lib().omr_rotate_batch_device_ex(C.c_void_p(int(d_src)), int(n), int(src_stride_bytes), int(src_step), int(rows),
                                           int(cols), int(channels), ap, float(scale), int(flags), int(border_mode),
                                           b.ctypes.data_as(u8p), int(clip_strategy), C.c_void_p(int(d_dst)),
                                           int(dst_stride_bytes), int(dst_step), int(slot_rows), int(slot_cols),
                                           sizes.ctypes.data_as(_lib.i32p) if a.size else None,
                                           C.c_void_p(int(stream)) if stream else None))
    return sizes


def rotate_batch_ex(srcs, angles, scale, flags, border_mode=0, border_value=(255.0, 255.0, 255.0, 0.0),
                    clip_strategy=RotateClipStrategy.DEFAULT):
    """omr_rotate_batch_ex: rotate_mat of every image of `srcs` (any mix of shapes and channel counts) by its own angle
    in one call -> a list of TransformableMatrix at the inputs' positions, each what rotate_mat gives."""
    views = [as_image(_mat(s)) for s in srcs]
    a, ap = _angles(angles)
    if a.size != len(views):
        raise ValueError("%d angles for %d images" % (a.size, len(views)))
    ims = (OmrImage * max(len(views), 1))(*[v[1] for v in views])
    outs = (OmrImageOwned * max(len(views), 1))()
    b = np.array([int(v) for v in border_value], np.uint8)
    check(lib().omr_rotate_batch_ex(ims, len(views), ap, float(scale), int(flags), int(border_mode), b.ctypes.data_as(u8p),
                                    int(clip_strategy), outs))
    return [TransformableMatrix(_take_owned(outs[i])) for i in range(len(views))]
