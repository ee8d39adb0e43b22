"""The line picture of the Hough and FFT detectors (packages/lib/src/hough.rs:44-63, fft.rs:173-213) restated for the
tests, numpy and plain Python only: cvtColor(GRAY2BGR) of the edge map, then every HoughLinesP segment drawn with
imgproc::line(img, p1, p2, Scalar(186, 88, 255, 0), 1, LINE_AA, 0), one after another in list order.

`draw_line_aa_literal` restates OpenCV 4.6.0 modules/imgproc/src/drawing.cpp for an 8-bit 3-channel image, thickness 1,
LINE_AA, shift 0: line() -> ThickLine() (end points << XY_SHIFT) -> LineAA(), statement by statement: the 16.16
coordinates (XY_SHIFT = 16), the swap that makes the major axis run upwards, x_step / y_step = (d << 16) / (a | 1) with
C's truncating division, SlopeCorrTable, the nine-entry end-point table ep_table, FilterTable, the three pixels of a
step across the minor axis and ICV_PUT_POINT's integer blend (applied twice per channel).  The end points must lie
inside the picture (HoughLinesP gives no others), so clipLine() changes nothing and is not restated.

`draw_line_aa` is the closed form the kernel implements (csrc/lined.hip): every step k of LineAA's loop has its state as
a function of k alone -- scount = k, ecount = E - k, the major coordinate m0 + k, the minor 16.16 value v0 + k * step --
so the steps can be taken in any order and from any starting k; the pixels of one segment's steps are disjoint.
tests/test_lined_ref.py asserts that the two agree.

OpenCV is not among this project's dependencies: the tables below are written from the published source, and
tests/test_lined_ref.py compares with cv2.line byte for byte where a cv2 can be imported."""
import numpy as np

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT
COLOR = (186, 88, 255)  # hough.rs:59, fft.rs:209 (B, G, R)

# drawing.cpp: SlopeCorrTable
SLOPE_CORR_TABLE = (
    181, 181, 181, 182, 182, 183, 184, 185, 187, 188, 190, 192, 194, 196, 198, 201,
    203, 206, 209, 211, 214, 218, 221, 224, 227, 231, 235, 238, 242, 246, 250, 254)

# drawing.cpp: FilterTable ("Gaussian for antialiasing filter")
FILTER_TABLE = (
    168, 177, 185, 194, 202, 210, 218, 224, 231, 236, 241, 246, 249, 252, 254, 254,
    254, 254, 252, 249, 246, 241, 236, 231, 224, 218, 210, 202, 194, 185, 177, 168,
    158, 149, 140, 131, 122, 114, 105, 99, 91, 85, 79, 72, 67, 61, 56, 51,
    46, 42, 38, 34, 30, 27, 24, 21, 18, 16, 14, 12, 10, 8, 7, 6)


def gray2bgr(edges):
    """cvtColor(GRAY2BGR): the byte in all three channels"""
    e = np.asarray(edges)
    assert e.ndim == 2 and e.dtype == np.uint8, "8-bit, one channel"
    return np.repeat(e[:, :, None], 3, axis=2)


def _cdiv(a, b):
    """C's integer division: truncates towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _check_inside(img, x0, y0, x1, y1):
    rows, cols = img.shape[:2]
    assert 0 <= x0 < cols and 0 <= x1 < cols and 0 <= y0 < rows and 0 <= y1 < rows, "end point outside the picture"


def segment_setup(x0, y0, x1, y1):
    """LineAA up to its loops, for integer end points (shift 0) -> (x_major, m0, E, v0, step, ep_table): the loop runs
    k = 0 .. E with scount = k, ecount = E - k, major coordinate m0 + k and minor 16.16 value v0 + k * step"""
    p1x, p1y, p2x, p2y = (int(v) << XY_SHIFT for v in (x0, y0, x1, y1))   # ThickLine: p <<= XY_SHIFT - shift
    dx, dy = p2x - p1x, p2y - p1y
    j = -1 if dx < 0 else 0
    ax = (dx ^ j) - j
    i = -1 if dy < 0 else 0
    ay = (dy ^ i) - i
    if ax > ay:
        dy = (dy ^ j) - j
        if j:                                       # the three XOR swaps under the mask j
            p1x, p2x, p1y, p2y = p2x, p1x, p2y, p1y
        y_step = _cdiv(dy << XY_SHIFT, ax | 1)
        p2x += XY_ONE
        ecount = (p2x >> XY_SHIFT) - (p1x >> XY_SHIFT)
        j = -(p1x & (XY_ONE - 1))
        p1y += ((y_step * j) >> XY_SHIFT) + (XY_ONE >> 1)
        slope = (y_step >> (XY_SHIFT - 5)) & 0x3f
        slope ^= 0x3f if y_step < 0 else 0
        i = (p1x >> (XY_SHIFT - 7)) & 0x78          # "Get 4-bit fractions for end-points": 0 at shift 0
        j = (p2x >> (XY_SHIFT - 7)) & 0x78
        x_major, m0, v0, step = True, p1x >> XY_SHIFT, p1y, y_step
    else:
        dx = (dx ^ i) - i
        if i:
            p1x, p2x, p1y, p2y = p2x, p1x, p2y, p1y
        x_step = _cdiv(dx << XY_SHIFT, ay | 1)
        p2y += XY_ONE
        ecount = (p2y >> XY_SHIFT) - (p1y >> XY_SHIFT)
        j = -(p1y & (XY_ONE - 1))
        p1x += ((x_step * j) >> XY_SHIFT) + (XY_ONE >> 1)
        slope = (x_step >> (XY_SHIFT - 5)) & 0x3f
        slope ^= 0x3f if x_step < 0 else 0
        i = (p1y >> (XY_SHIFT - 7)) & 0x78
        j = (p2y >> (XY_SHIFT - 7)) & 0x78
        x_major, m0, v0, step = False, p1y >> XY_SHIFT, p1x, x_step
    slope = 0x100 if slope & 0x20 else SLOPE_CORR_TABLE[slope]
    # "Calc end point correction table"
    t0 = slope << 7
    t1 = ((0x78 - i) | 4) * slope
    t2 = (j | 4) * slope
    ep = [0] * 9
    ep[0] = 0
    ep[8] = slope
    ep[1] = ep[3] = ((((j - i) & 0x78) | 4) * slope >> 8) & 0x1ff
    ep[2] = (t1 >> 8) & 0x1ff
    ep[4] = ((((j - i) + 0x80) | 4) * slope >> 8) & 0x1ff
    ep[5] = ((t1 + t0) >> 8) & 0x1ff
    ep[6] = (t2 >> 8) & 0x1ff
    ep[7] = ((t2 + t0) >> 8) & 0x1ff
    return x_major, m0, ecount, v0, step, ep


def _put_point(img, x, y, a, color):
    """ICV_PUT_POINT for three channels: the blend runs twice per channel"""
    for c in range(3):
        v = int(img[y, x, c])
        v += ((color[c] - v) * a + 127) >> 8
        v += ((color[c] - v) * a + 127) >> 8
        img[y, x, c] = v                            # (uchar)


def draw_line_aa_literal(img, x0, y0, x1, y1, color=COLOR):
    """LineAA's loops as they are written: scount counts up, ecount down, the minor coordinate is accumulated"""
    _check_inside(img, x0, y0, x1, y1)
    rows, cols = img.shape[:2]
    x_major, m, ecount, v, step, ep = segment_setup(x0, y0, x1, y1)
    scount = 0
    while ecount >= 0:
        major_size, minor_size = (cols, rows) if x_major else (rows, cols)
        if 0 <= m < major_size:                     # (unsigned)x >= (unsigned)size0.width: continue
            n = (v >> XY_SHIFT) - 1
            ep_corr = ep[(((scount >= 2) + 1) & (scount | 2)) * 3 + (((ecount >= 2) + 1) & (ecount | 2))]
            dist = (v >> (XY_SHIFT - 5)) & 31
            for off, f in ((0, FILTER_TABLE[dist + 32]), (1, FILTER_TABLE[dist]), (2, FILTER_TABLE[63 - dist])):
                a = (ep_corr * f >> 8) & 0xff
                if 0 <= n + off < minor_size:
                    if x_major:
                        _put_point(img, m, n + off, a, color)
                    else:
                        _put_point(img, n + off, m, a, color)
        m += 1
        v += step
        scount += 1
        ecount -= 1
    return img


def draw_line_aa(img, x0, y0, x1, y1, color=COLOR):
    """the same picture from the closed form: all steps at once (their pixels are disjoint)"""
    _check_inside(img, x0, y0, x1, y1)
    rows, cols = img.shape[:2]
    x_major, m0, E, v0, step, ep = segment_setup(x0, y0, x1, y1)
    major_size, minor_size = (cols, rows) if x_major else (rows, cols)
    k = np.arange(E + 1, dtype=np.int64)
    m = m0 + k
    v = v0 + k * step
    n = (v >> XY_SHIFT) - 1
    dist = (v >> (XY_SHIFT - 5)) & 31
    ep_corr = np.asarray(ep, np.int64)[np.minimum(k, 2) * 3 + np.minimum(E - k, 2)]
    ft = np.asarray(FILTER_TABLE, np.int64)
    col = np.asarray(color, np.int64)
    for off, f in ((0, ft[dist + 32]), (1, ft[dist]), (2, ft[63 - dist])):
        a = ((ep_corr * f) >> 8) & 0xff
        ok = (m >= 0) & (m < major_size) & (n + off >= 0) & (n + off < minor_size)
        mm, nn, aa = m[ok], n[ok] + off, a[ok][:, None]
        ys, xs = (nn, mm) if x_major else (mm, nn)
        p = img[ys, xs, :].astype(np.int64)
        p += ((col - p) * aa + 127) >> 8
        p += ((col - p) * aa + 127) >> 8
        img[ys, xs, :] = p.astype(np.uint8)
    return img


def draw_lines_aa(picture_bgr, lines, color=COLOR, literal=False):
    """picture_bgr (rows, cols, 3) uint8 with every segment (x0, y0, x1, y1) of `lines` drawn on a copy, in list order"""
    img = np.array(picture_bgr, dtype=np.uint8, copy=True)
    assert img.ndim == 3 and img.shape[2] == 3, "8-bit, three channels"
    draw = draw_line_aa_literal if literal else draw_line_aa
    for x0, y0, x1, y1 in np.asarray(lines, np.int64).reshape(-1, 4):
        draw(img, int(x0), int(y0), int(x1), int(y1), color)
    return img


def lined_picture(edges, lines, color=COLOR):
    """hough.rs:44-63 / fft.rs:173-213: GRAY2BGR, then the segments"""
    return draw_lines_aa(gray2bgr(edges), lines, color)


def chebyshev_far_mask(shape, lines, dist):
    """True where a pixel is more than `dist` (Chebyshev) from every point of every segment"""
    rows, cols = shape
    ys, xs = np.mgrid[0:rows, 0:cols].astype(np.float64)
    far = np.ones((rows, cols), bool)
    for x0, y0, x1, y1 in np.asarray(lines, np.float64).reshape(-1, 4):
        # Chebyshev distance to a segment: minimise max(|x - px(t)|, |y - py(t)|) over t -- sampled densely enough for
        # pictures of a few hundred pixels (the segment moves < 0.25 px between samples)
        steps = int(4 * max(abs(x1 - x0), abs(y1 - y0))) + 1
        d = np.full((rows, cols), np.inf)
        for t in np.linspace(0.0, 1.0, steps + 1):
            px, py = x0 + t * (x1 - x0), y0 + t * (y1 - y0)
            d = np.minimum(d, np.maximum(np.abs(xs - px), np.abs(ys - py)))
        far &= d > dist
    return far
