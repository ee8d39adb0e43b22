"""Float64 first-principles references for the geometric and photometric kernels, and the bounds a fixed-point
implementation may differ from them by.  numpy only: nothing here imports the oracle, warp_ref or the library, and
nothing is taken from OpenCV's fixed-point code -- only the textbook definitions of the operations it computes:

  warp          affine resampling with a nearest, bilinear, Keys-cubic (A = -0.75) or Lanczos-4 kernel and the five
                border extensions, the source coordinates in float64, the result unrounded
  area_resize   the exact integral of the piecewise-constant image over each destination cell, over the cell's area
  linear_resize bilinear at (x + 0.5) * cols / dcols - 0.5 with clamped indices
  gray          0.114 B + 0.587 G + 0.299 R

Each bound is a function whose docstring holds its derivation from the number formats of the published algorithm
(warpAffine: 1/32 px coordinates, 10-bit matrix tables, 15-bit weights; resize: 11-bit coefficients or float32
sums; cvtColor: 14-bit coefficients).  None of them was fitted to what the code under test gives.
tests/test_geom_exact.py holds the restatements (warp_ref.py, oracle.c) to these bounds, tests/test_gpu_geom_exact.py
the kernels."""
import functools
import math

import numpy as np

NEAREST, LINEAR, CUBIC, AREA, LANCZOS4 = 0, 1, 2, 3, 4
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT = 0, 1, 2, 3, 4, 5
INVERSE_MAP = 16
TAPS = {NEAREST: 1, LINEAR: 2, CUBIC: 4, AREA: 2, LANCZOS4: 8}
DEFAULT, CONTAIN = 0, 1
COORD_DELTA = 1.0 / 64 + 1.0 / 1024  # see general_warp_bound
NEAREST_TIE = 2.0 / 1024             # see nearest_candidates


# ---- geometry ------------------------------------------------------------------------------------------------------
def rotate_geometry(rows, cols, angle, scale, clip, inverse_map=False):
    """rotate_mat's matrix and canvas (the reference's transfer.rs:459-519) -> (dst2src [2, 3] float64, drows, dcols).

    getRotationMatrix2D(centre, angle, scale): a = s cos, b = s sin, [[a, b, (1 - a) cx - b cy], [-b, a, b cx + (1 - a) cy]].
    DEFAULT (transfer.rs:472-486): centre (cols / 2, rows / 2), the canvas is the source's size.
    CONTAIN (transfer.rs:487-519): canvas (ceil(rows |sin| + cols |cos|), ceil(cols |sin| + rows |cos|)) as (width,
    height), centre (ceil(width / 2), ceil(height / 2)), then ceil((width - cols) / 2) and ceil((height - rows) / 2) added
    to the two translations.
    warpAffine maps destination to source with the inverse of that matrix, or with the matrix itself under
    WARP_INVERSE_MAP; the inverse is taken here in float64."""
    t = angle * math.pi / 180.0
    if clip == DEFAULT:
        cx, cy, dr, dc, ox, oy = cols / 2.0, rows / 2.0, rows, cols, 0.0, 0.0
    else:
        sn, cs = abs(math.sin(t)), abs(math.cos(t))
        rw, rh = math.ceil(rows * sn + cols * cs), math.ceil(cols * sn + rows * cs)
        cx, cy, dr, dc = math.ceil(rw / 2.0), math.ceil(rh / 2.0), int(rh), int(rw)
        ox, oy = math.ceil((rw - cols) / 2.0), math.ceil((rh - rows) / 2.0)
    a, b = scale * math.cos(t), scale * math.sin(t)
    M = np.array([[a, b, (1 - a) * cx - b * cy + ox], [-b, a, b * cx + (1 - a) * cy + oy]], np.float64)
    if inverse_map:
        return M, dr, dc
    A = np.linalg.inv(M[:, :2])
    return np.concatenate([A, -(A @ M[:, 2:])], 1), dr, dc


def snap(dst2src, den=32):
    """A map whose every term is, mathematically, a multiple of 1 / den (a quarter turn at a dyadic scale about a
    centre on that grid), freed of what float64 trigonometry and inversion left on it: cos(90 deg) = 6e-17 and
    1 / (32 / 33) = 33 / 32 (1 + 2e-16) would otherwise move a sample that lies exactly on a rounding boundary.  Asserts
    that the map was within 1e-9 of that grid, so no other map can be passed off as exact."""
    q = np.round(np.asarray(dst2src, np.float64) * den) / den
    assert np.abs(q - dst2src).max() < 1e-9, dst2src
    return q


def source_coords(dst2src, dr, dc):
    """(x, y) float64 [dr, dc] source coordinates of the destination pixel centres"""
    yy, xx = np.mgrid[:dr, :dc].astype(np.float64)
    M = np.asarray(dst2src, np.float64)
    return M[0, 0] * xx + M[0, 1] * yy + M[0, 2], M[1, 0] * xx + M[1, 1] * yy + M[1, 2]


# ---- the interpolation kernels, float64 ----------------------------------------------------------------------------
def weights(interp, t):
    """[..., K] float64 weights of taps first .. first + K - 1 (first = -(K / 2 - 1)) at fraction t in [0, 1)"""
    t = np.asarray(t, np.float64)
    K = TAPS[interp]
    if K == 2:
        return np.stack([1 - t, t], -1)
    if K == 4:  # Keys' cubic convolution kernel, A = -0.75, taps -1 .. 2
        A = -0.75
        d = np.abs(t[..., None] - np.arange(-1, 3))
        near = ((A + 2) * d - (A + 3)) * d * d + 1
        far = ((A * d - 5 * A) * d + 8 * A) * d - 4 * A
        return np.where(d <= 1, near, far)
    if K == 8:  # Lanczos, a = 4: sinc(x) sinc(x / 4), taps -3 .. 4, normalised to sum 1
        x = t[..., None] - np.arange(-3, 5)
        px = np.pi * np.where(x == 0, 1.0, x)
        w = np.where(x == 0, 1.0, np.sin(px) * np.sin(px / 4) / (px * px / 4))
        return w / w.sum(-1, keepdims=True)
    raise ValueError(interp)


def border_index(p, n, mode):
    """(index int64, inside bool): the border extension by index arithmetic; BORDER_CONSTANT marks the taps outside"""
    p = np.asarray(p, np.int64)
    inside = (p >= 0) & (p < n)
    if mode == CONSTANT:
        return np.clip(p, 0, n - 1), inside
    if mode == REPLICATE:
        q = np.clip(p, 0, n - 1)
    elif mode == REFLECT:        # fedcba|abcdefgh|hgfedcb
        m = np.mod(p, 2 * n)
        q = np.where(m < n, m, 2 * n - 1 - m)
    elif mode == WRAP:           # cdefgh|abcdefgh|abcdefg
        q = np.mod(p, n)
    elif mode in (REFLECT_101, TRANSPARENT):  # gfedcb|abcdefgh|gfedcba; TRANSPARENT's written pixels extend this way
        if n == 1:
            q = np.zeros_like(p)
        else:
            m = np.mod(p, 2 * n - 2)
            q = np.where(m < n, m, 2 * n - 2 - m)
    else:
        raise ValueError(mode)
    return q, np.ones(p.shape, bool)


def _sample(src3, ix, iy, okx, oky, border_value):
    """src3[iy, ix] as float64 [..., cn], the border value where either index is marked outside"""
    v = src3[iy, ix].astype(np.float64)
    cv = np.asarray(border_value, np.float64)[:src3.shape[2]]
    return np.where((okx & oky)[..., None], v, cv)


def warp_at(src, x, y, interp, border_mode, border_value):
    """the interpolated image at float64 source coordinates x, y (same shape) -> float64 [..., cn], unrounded"""
    a = np.asarray(src)
    src3 = a if a.ndim == 3 else a[:, :, None]
    h, w, _ = src3.shape
    K = TAPS[interp]
    if K == 1:
        ix, okx = border_index(np.floor(x + 0.5), w, border_mode)
        iy, oky = border_index(np.floor(y + 0.5), h, border_mode)
        return _sample(src3, ix, iy, okx, oky, border_value)
    fx, fy = np.floor(x), np.floor(y)
    wx, wy = weights(interp, x - fx), weights(interp, y - fy)
    first = -(K // 2 - 1)
    out = 0.0
    for i in range(K):
        iy, oky = border_index(fy + first + i, h, border_mode)
        for j in range(K):
            ix, okx = border_index(fx + first + j, w, border_mode)
            out = out + (wy[..., i] * wx[..., j])[..., None] * _sample(src3, ix, iy, okx, oky, border_value)
    return out


def warp(src, dst2src, dr, dc, interp, border_mode, border_value):
    """the dr x dc canvas of `src` resampled through dst2src -> float64 [dr, dc, cn], unrounded and unclipped"""
    x, y = source_coords(dst2src, dr, dc)
    return warp_at(src, x, y, interp, border_mode, border_value)


def nearest_candidates(src, dst2src, dr, dc, border_mode, border_value):
    """NEAREST at a general angle -> (reference [dr, dc, cn], alternatives [4, dr, dc, cn], ambiguous [dr, dc] bool).

    The fixed-point coordinate is round((M x) 1024) + round((M y + b) 1024) + 512 >> 10: two table roundings of half a
    unit each and float64 products good to far less, so it is floor(x + 0.5 + e) with |e| <= 1 / 1024; NEAREST_TIE =
    2 / 1024 doubles that.  A pixel whose exact x + 0.5 or y + 0.5 lies that close to an integer may take the neighbour on
    either side of it (the four alternatives are the samples at x -+ tie, y -+ tie); every other pixel has one answer."""
    x, y = source_coords(dst2src, dr, dc)

    def near(v):
        f = v + 0.5 - np.floor(v + 0.5)
        return (f < NEAREST_TIE) | (f > 1 - NEAREST_TIE)

    alts = np.stack([warp_at(src, x + sx * NEAREST_TIE, y + sy * NEAREST_TIE, NEAREST, border_mode, border_value)
                     for sx in (-1, 1) for sy in (-1, 1)])
    return warp_at(src, x, y, NEAREST, border_mode, border_value), alts, near(x) | near(y)


# ---- resize and gray -----------------------------------------------------------------------------------------------
def _cell_weights(n, dn):
    """[dn, n] float64: the length of source sample i's unit interval [i, i + 1) inside destination cell j =
    [j n / dn, (j + 1) n / dn) clipped to the image, over the clipped cell's length"""
    lo = np.arange(dn, dtype=np.float64) * n / dn
    hi = np.minimum((np.arange(dn, dtype=np.float64) + 1) * n / dn, n)
    i = np.arange(n, dtype=np.float64)
    ov = np.clip(np.minimum(hi[:, None], i[None, :] + 1) - np.maximum(lo[:, None], i[None, :]), 0, None)
    return ov / (hi - lo)[:, None]


def area_resize(src, drows, dcols):
    """the mean of the piecewise-constant image over each destination cell -> float64 [drows, dcols, cn]"""
    a = np.asarray(src)
    s = (a if a.ndim == 3 else a[:, :, None]).astype(np.float64)
    wy, wx = _cell_weights(s.shape[0], drows), _cell_weights(s.shape[1], dcols)
    return np.einsum("yi,ijc,xj->yxc", wy, s, wx)


def linear_resize(src, drows, dcols):
    """bilinear enlargement: source coordinate (x + 0.5) cols / dcols - 0.5, indices clamped -> float64 [drows, dcols, cn]"""
    a = np.asarray(src)
    s = a if a.ndim == 3 else a[:, :, None]
    y = (np.arange(drows) + 0.5) * s.shape[0] / drows - 0.5
    x = (np.arange(dcols) + 0.5) * s.shape[1] / dcols - 0.5
    yy, xx = np.meshgrid(y, x, indexing="ij")
    return warp_at(s, xx, yy, LINEAR, REPLICATE, (0, 0, 0, 0))


def gray(bgr):
    """the luma of [..., 3 or 4] samples in B, G, R order: 0.114 B + 0.587 G + 0.299 R -> float64 [...]"""
    c = np.asarray(bgr).astype(np.float64)
    return 0.114 * c[..., 0] + 0.587 * c[..., 1] + 0.299 * c[..., 2]


# ---- the bounds ----------------------------------------------------------------------------------------------------
def wq(interp):
    """What the 15-bit weight table may move a pixel by, in levels.  Bilinear: the entries (32 - fy)(32 - fx) 32 are the
    exact weights times 32768, so 0.  Cubic and Lanczos-4 (K = 4, 8): each of the K * K products is rounded to a
    multiple of 1 / 32768 (half a unit each: K * K / 2 units over the window), and the fix that makes the table row sum to
    32768 moves one entry by a few units more (4 allowed); every unit is worth at most 255 / 32768 of a level."""
    K = TAPS[interp]
    return 0.0 if K <= 2 else 255.0 * (K * K / 2.0 + 4) / 32768


def exact_warp_bound(interp):
    """|got - clip(exact, 0, 255)| for a warp whose fixed-point coordinates are exact (every term of the map a multiple
    of 1 / 32): the final rounding to a level, half a level, plus wq.  Clipping is 1-Lipschitz, so it adds nothing."""
    return 0.5 + wq(interp)


@functools.lru_cache(maxsize=None)
def kernel_norms(interp):
    """(S, A) of the 1-D kernel over the fraction t, numerically from `weights`:
    A = max sum_j |w_j(t)|, S = max sum_k |sum_{j <= k} w_j'(t)| (the derivative by central differences)."""
    t = np.linspace(0, 1, 4097)[:-1] + 1.0 / 8192
    h = 1e-6
    A = np.abs(weights(interp, np.linspace(0, 1, 4097)[:-1])).sum(-1).max()
    d = (weights(interp, t + h) - weights(interp, t - h)) / (2 * h)
    S = np.abs(np.cumsum(d, -1)[..., :-1]).sum(-1).max()
    return float(S), float(A)


def adjacent_differences(src, border_mode, border_value):
    """(Lx, Ly): the largest difference of two neighbouring samples of the extended image along each axis.  The
    reflecting and replicating extensions repeat differences the image already has (or 0); BORDER_WRAP puts the last
    sample next to the first; BORDER_CONSTANT puts the border value next to every edge sample."""
    a = np.asarray(src)
    s = (a if a.ndim == 3 else a[:, :, None]).astype(np.float64)
    cv = np.asarray(border_value, np.float64)[:s.shape[2]]
    L = []
    for ax in (1, 0):
        v = [np.abs(np.diff(s, axis=ax)).max()] if s.shape[ax] > 1 else [0.0]
        first, last = np.take(s, 0, axis=ax), np.take(s, -1, axis=ax)
        if border_mode == WRAP:
            v.append(np.abs(first - last).max())
        if border_mode == CONSTANT:
            v += [np.abs(first - cv).max(), np.abs(last - cv).max()]
        L.append(float(max(v)))
    return L[0], L[1]


def general_warp_bound(interp, src, border_mode, border_value):
    """|got - clip(exact, 0, 255)| for LINEAR, CUBIC and LANCZOS4 at any affine map:
    0.5 + wq(K) + S(K) A(K) (Lx + Ly) delta.

    The fixed-point sample position differs from the exact one by at most delta = 1 / 64 + 1 / 1024 px on each axis:
    the coordinate is rounded to the nearest 1 / 32 px (1 / 64), and it is the sum of two table entries each rounded to
    1 / 1024 px (AB_BITS = 10; half a unit each).  The interpolant V(x, y) = sum_i sum_j wy_i wx_j I_ij is continuous
    (each kernel is, and is 0 at the ends of its support) and piecewise smooth, with, by summation by parts (sum_j w_j' =
    0), dV/dx = -sum_i wy_i sum_k (sum_{j <= k} w_j') (I_{i, k + 1} - I_{i, k}), so |dV/dx| <= A S Lx, and likewise in y."""
    S, A = kernel_norms(interp)
    Lx, Ly = adjacent_differences(src, border_mode, border_value)
    return 0.5 + wq(interp) + S * A * (Lx + Ly) * COORD_DELTA


def area_bound(rows, cols, drows, dcols):
    """|got - exact| for the area resize: 0.5 + eps.  The integer-factor form sums integers exactly and multiplies by a
    float32 reciprocal (2 x 2 cells: (sum + 2) >> 2, exact); the fractional form multiplies by float32 weights and sums
    in float32: nx taps along a row, then ny row sums, each a product and a sum.  With u = 2^-24 and all terms
    non-negative and summing to at most 255, the standard bound is 255 gamma(nx + ny + 4), gamma(n) = n u / (1 - n u),
    nx = ceil(cols / dcols) + 1 taps (two partial ones).  The published tap table drops a partial tap narrower than 1e-3
    source pixels; overlaps here are multiples of 1 / dcols (or 1 / drows), so with fewer than 1000 cells it never does."""
    assert drows < 1000 and dcols < 1000
    n = (math.ceil(cols / dcols) + 1) + (math.ceil(rows / drows) + 1) + 4
    u = 2.0 ** -24
    return 0.5 + 255.0 * n * u / (1 - n * u)


LINEAR_RESIZE_Q = ((2.0 / 2048) * (1 + 1.0 / 2048) + 2.0 ** -20) + (0.5 + (1.0 / 128) * (1 + 1.0 / 2048)) / 255


def linear_resize_bound():
    """|got - exact| for the 8-bit bilinear resize: 0.5 + 255 q, from the published integer scheme.

    The four coefficients (1 - fx, fx, 1 - fy, fy) are rounded to 11 bits, 1 / 4096 each (the float32 fraction adds
    less than 2^-20).  V = sum b_i a_j S_ij with the pairs summing to at most 1 + 1 / 2048, so the coefficients move V by at
    most 255 (2 / 4096 + 2 / 4096)(1 + 1 / 2048) = 255 (2 / 2048)(1 + 1 / 2048).  The row sums h = S0 a0 + S1 a1 are exact in
    units of 1 / 2048 level; the vertical pass takes h >> 4 (drops less than 1 / 128 level, weighted by at most 1 + 1 / 2048),
    then each of its two products >> 16 (each drops less than a quarter level: the sum is in units of a quarter), then
    rounds (+ 2) >> 2 to the nearest level (0.5).  The droppings are one-sided, 0.5 + 1 / 128 in all, and not scaled by
    the image: as a share of 255 they complete q.  255 q = 0.757; the restated oracle's worst on the test inputs is 0.78 levels of the
    1.257 (tests/test_geom_exact.py)."""
    return 0.5 + 255.0 * LINEAR_RESIZE_Q


def gray_bound():
    """|got - exact| for the gray conversion: the three coefficients are 14-bit (half a unit of 1 / 16384 each) on samples
    of at most 255, then one rounding to a level."""
    return 0.5 + 255.0 * 3 * 0.5 / 16384


# ---- reporting -----------------------------------------------------------------------------------------------------
def worst(got, exact, bound, clip=True):
    """(violations, (index, got, exact, bound) of the worst pixel, worst error / bound).  `bound` a number or an array
    that broadcasts against the pixels."""
    e = np.clip(exact, 0, 255) if clip else np.asarray(exact, np.float64)
    g = np.asarray(got, np.float64).reshape(e.shape)
    err = np.abs(g - e)
    b = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    ratio = err / b
    k = np.unravel_index(int(np.argmax(ratio)), err.shape) if err.size else ()
    at = (tuple(int(v) for v in k), float(g[k]), float(e[k]), float(b[k])) if err.size else None
    return int((err > b).sum()), at, float(ratio[k]) if err.size else 0.0
