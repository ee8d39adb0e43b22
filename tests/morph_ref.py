"""numpy restatement of erode / dilate as TransformableMatrix::erode / dilate call them (transfer.rs:206-277):
getStructuringElement(shape, size, anchor) of OpenCV 4.6.0, then `iterations` passes of

    dst(y, x) = min (erode) or max (dilate) over the set cells (i, j) of the element of src(y + i - ay, x + j - ax)

per channel, with BORDER_CONSTANT and morphologyDefaultBorderValue(): positions outside the image take no part
(255 for erode, 0 for dilate).  Dilate uses the element unmirrored, as cv::dilate does.  Every pass pads the image
with the neutral value afresh, so nothing from outside the image survives from one pass to the next.

Written from those semantics alone; it takes nothing from the library."""
import math

import numpy as np

RECT, CROSS, ELLIPSE = 0, 1, 2
ERODE, DILATE = 0, 1


def normalize_anchor(kw, kh, anchor):
    ax, ay = anchor
    ax = kw // 2 if ax == -1 else ax
    ay = kh // 2 if ay == -1 else ay
    if not (0 <= ax < kw and 0 <= ay < kh):
        raise ValueError("anchor outside the element")
    return ax, ay


def cv_round(v):
    """cvRound: nearest, ties to even"""
    return int(np.rint(v))


def get_structuring_element(shape, size, anchor=(-1, -1)):
    """(kh, kw) uint8 mask of 0 / 1; size = (kw, kh), anchor = (ax, ay)"""
    kw, kh = size
    if shape not in (RECT, CROSS, ELLIPSE) or kw < 1 or kh < 1:
        raise ValueError("bad element")
    ax, ay = normalize_anchor(kw, kh, anchor)
    if (kw, kh) == (1, 1):
        shape = RECT
    r = c = 0
    inv_r2 = 0.0
    if shape == ELLIPSE:
        r, c = kh // 2, kw // 2
        inv_r2 = 1.0 / (r * r) if r else 0.0
    m = np.zeros((kh, kw), np.uint8)
    for i in range(kh):
        j1 = j2 = 0
        if shape == RECT or (shape == CROSS and i == ay):
            j2 = kw
        elif shape == CROSS:
            j1, j2 = ax, ax + 1
        else:
            dy = i - r
            if abs(dy) <= r:
                dx = cv_round(c * math.sqrt((r * r - dy * dy) * inv_r2))
                j1, j2 = max(c - dx, 0), min(c + dx + 1, kw)
        m[i, j1:j2] = 1
    return m


def morph_mask(a, op, mask, anchor, iterations):
    """`iterations` passes of the element `mask` (kh, kw) anchored at (ax, ay) over a (rows, cols[, cn]) uint8 image"""
    if iterations < 0:
        raise ValueError("iterations < 0")
    kh, kw = mask.shape
    ax, ay = anchor
    neutral = 255 if op == ERODE else 0
    pick = np.minimum if op == ERODE else np.maximum
    a = np.ascontiguousarray(a)
    rows, cols = a.shape[:2]
    cells = [(i, j) for i in range(kh) for j in range(kw) if mask[i, j]]
    for _ in range(iterations):
        p = np.full((rows + kh - 1, cols + kw - 1) + a.shape[2:], neutral, np.uint8)
        p[ay:ay + rows, ax:ax + cols] = a
        out = np.full(a.shape, neutral, np.uint8)
        for i, j in cells:
            out = pick(out, p[i:i + rows, j:j + cols])
        a = out
    return a.copy()


def morph(a, op, shape, size, anchor=(-1, -1), iterations=1):
    kw, kh = size
    anchor = normalize_anchor(kw, kh, anchor)
    return morph_mask(a, op, get_structuring_element(shape, size, anchor), anchor, iterations)


def erode(a, shape, size, anchor=(-1, -1), iterations=1):
    return morph(a, ERODE, shape, size, anchor, iterations)


def dilate(a, shape, size, anchor=(-1, -1), iterations=1):
    return morph(a, DILATE, shape, size, anchor, iterations)
