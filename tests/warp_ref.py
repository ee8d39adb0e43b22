"""numpy restatement of warpAffine as rotate_mat calls it (transfer.rs:459-523), for every interpolation and border mode
omr_rotate_ex takes.  OpenCV 4.6.0 imgwarp.cpp:

  * coordinates: WarpAffineInvoker's fixed-point tables, taken from the oracle (oracle.warp_tables: AB_BITS = 10,
    round delta 512 for NEAREST, 16 otherwise), X >> 5, saturate_cast<short>(X >> 5), fraction (Y & 31) * 32 + (X & 31);
  * weights: initInterTab1D / initInterTab2D(method, fixpt = true) -- interpolateCubic (A = -0.75),
    interpolateLanczos4 (libm sin / cos through Python's math module, float sums), the float 2-D product,
    saturate_cast<short>(v * 32768) and the sum fix on the central 2 x 2;
  * remapNearest / remapBilinear / remapBicubic / remapLanczos4 with FixedPtCast<int, uchar, 15>: each method's
    interior test (width - K + 1), its BORDER_TRANSPARENT rule, BORDER_CONSTANT's whole-window test and
    cv * ONE + sum (S - cv) w, and borderInterpolate (its loop for REFLECT / REFLECT_101) for the other modes.

Integer arithmetic is int64 throughout; float work is np.float32 scalar by scalar in OpenCV's operation order."""
import functools
import math

import numpy as np

from oracle import oracle as orc

F = np.float32
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT = 0, 1, 2, 3, 4, 5
INVERSE_MAP = 16
TAPS = {0: 1, 1: 2, 2: 4, 4: 8}
_PI = 3.1415926535897932384626433832795


def interpolate_cubic(x):
    A = F(-0.75)
    x1 = x + F(1)
    c0 = ((A * x1 - F(5) * A) * x1 + F(8) * A) * x1 - F(4) * A
    c1 = ((A + F(2)) * x - (A + F(3))) * x * x + F(1)
    om = F(1) - x
    c2 = ((A + F(2)) * om - (A + F(3))) * om * om + F(1)
    c3 = F(1) - c0 - c1 - c2
    return [F(c0), F(c1), F(c2), F(c3)]


def interpolate_lanczos4(x):
    s45 = 0.70710678118654752440084436210485
    cs = [(1, 0), (-s45, -s45), (0, 1), (s45, -s45), (-1, 0), (s45, s45), (0, -1), (-s45, s45)]
    if x < F(np.finfo(np.float32).eps):
        return [F(0), F(0), F(0), F(1), F(0), F(0), F(0), F(0)]
    y0 = float(-(x + F(3))) * _PI * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    co, sm = [], F(0)
    for i in range(8):
        y0_ = x + F(3) - F(i)
        if abs(y0_) >= F(1e-6):
            y = float(-y0_) * _PI * 0.25
            c = F((cs[i][0] * s0 + cs[i][1] * c0) / (y * y))
        else:
            c = F(1e30)
        sm = F(sm + c)
        co.append(c)
    sm = F(1) / sm
    return [F(c * sm) for c in co]


@functools.lru_cache(maxsize=None)
def coeff_table(interp):
    """[1024, K * K] int64: entry fy * 32 + fx, tap row * K + col (K = 1, 2, 4, 8 for interp 0, 1, 2, 4)"""
    K = TAPS[interp]
    if K == 1:
        return np.full((1024, 1), 32768, np.int64)
    if K == 2:
        f = np.arange(32)
        fy, fx = np.repeat(f, 32), np.tile(f, 32)
        return np.stack([(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32], 1).astype(np.int64)
    fn = interpolate_cubic if K == 4 else interpolate_lanczos4
    tab1 = [fn(F(i) * F(1.0 / 32)) for i in range(32)]
    out = np.zeros((1024, K * K), np.int64)
    for i in range(32):
        for j in range(32):
            it = [0] * (K * K)
            for k1 in range(K):
                vy = tab1[i][k1]
                for k2 in range(K):
                    v = F(vy * tab1[j][k2])
                    q = int(np.rint(float(F(v * F(32768)))))
                    it[k1 * K + k2] = max(-32768, min(32767, q))
            isum = sum(it)
            if isum != 32768:
                diff = isum - 32768
                k2_ = K // 2
                Mk1 = Mk2 = mk1 = mk2 = k2_
                for k1 in range(k2_, k2_ + 2):
                    for k2 in range(k2_, k2_ + 2):
                        if it[k1 * K + k2] < it[mk1 * K + mk2]:
                            mk1, mk2 = k1, k2
                        elif it[k1 * K + k2] > it[Mk1 * K + Mk2]:
                            Mk1, Mk2 = k1, k2
                if diff < 0:
                    it[Mk1 * K + Mk2] -= diff
                else:
                    it[mk1 * K + mk2] -= diff
            out[i * 32 + j] = it
    return out


def border_interpolate(p, n, mode):
    """borderInterpolate on an int64 array; -1 for BORDER_CONSTANT outside"""
    p = np.asarray(p, np.int64)
    out = p.copy()
    bad = (p < 0) | (p >= n)
    if not bad.any():
        return out
    if mode == CONSTANT:
        out[bad] = -1
    elif mode == REPLICATE:
        out[bad] = np.where(p[bad] < 0, 0, n - 1)
    elif mode in (REFLECT, REFLECT_101):
        if n == 1:
            out[bad] = 0
            return out
        d = 1 if mode == REFLECT_101 else 0
        q = p[bad]
        while True:
            m = (q < 0) | (q >= n)
            if not m.any():
                break
            q = np.where(q < 0, -q - 1 + d, np.where(q >= n, n - 1 - (q - n) - d, q))
        out[bad] = q
    elif mode == WRAP:
        q = p[bad]
        neg = q < 0
        a = q[neg] - n + 1  # C's truncating (p - len + 1) / len for p < 0
        q[neg] -= (-((-a) // n)) * n
        pos = q >= n
        q[pos] %= n
        out[bad] = q
    else:
        raise ValueError(mode)
    return out


def _sat16(v):
    return np.clip(v, -32768, 32767)


def remap(src3, Xf, Yf, interp, mode, cval):
    """(values [n, cn] uint8, keep [n] bool) of the destination pixels with fixed-point coordinates Xf, Yf (int64,
    round delta included)"""
    h, w, cn = src3.shape
    K = TAPS[interp]
    if K == 1:
        sx, sy = _sat16(Xf >> 10), _sat16(Yf >> 10)
        fxy = np.zeros_like(sx)
    else:
        X, Y = Xf >> 5, Yf >> 5
        sx, sy = _sat16(X >> 5), _sat16(Y >> 5)
        fxy = (Y & 31) * 32 + (X & 31)
    O = 0 if K == 1 else K // 2 - 1
    tx, ty = sx - O, sy - O
    interior = (tx >= 0) & (tx < max(w - K + 1, 0)) & (ty >= 0) & (ty < max(h - K + 1, 0))
    keep = np.ones(len(sx), bool)
    m = mode
    if mode == TRANSPARENT:
        if K <= 2:  # remapNearest: outside; remapBilinear: every pixel off the interior
            keep = interior
        else:       # remapBicubic / remapLanczos4: the centre tap outside
            keep = interior | ((sx >= 0) & (sx < w) & (sy >= 0) & (sy < h))
        m = REFLECT_101  # borderType1
    offs = np.arange(K)
    mx = border_interpolate(tx[:, None] + offs, w, m)
    my = border_interpolate(ty[:, None] + offs, h, m)
    valid = (my[:, :, None] >= 0) & (mx[:, None, :] >= 0)
    S = src3[np.maximum(my, 0)[:, :, None], np.maximum(mx, 0)[:, None, :]].astype(np.int64)  # [n, K, K, cn]
    cv = np.array(cval[:cn], np.int64)
    if K == 1:
        val = np.where(valid[..., None], S, cv)[:, 0, 0, :]
        return val.astype(np.uint8), keep
    wt = coeff_table(interp)[fxy].reshape(-1, K, K, 1)
    if mode == CONSTANT and K >= 4:
        s = cv * 32768 + (np.where(valid[..., None], S - cv, 0) * wt).sum(axis=(1, 2))
        all_out = (tx >= w) | (tx + K <= 0) | (ty >= h) | (ty + K <= 0)
    elif mode == CONSTANT:
        s = (np.where(valid[..., None], S, cv) * wt).sum(axis=(1, 2))
        all_out = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
    else:
        s = (S * wt).sum(axis=(1, 2))
        all_out = np.zeros(len(sx), bool)
    val = np.clip((s + (1 << 14)) >> 15, 0, 255)
    val[all_out] = cv
    return val.astype(np.uint8), keep


def rotate_geometry(rows, cols, angle, scale, clip):
    """rotate_mat's forward matrix and canvas (transfer.rs:472-519)"""
    if clip == 0:
        cx, cy = F(cols) / F(2), F(rows) / F(2)
        return orc.get_rotation_matrix_2d(float(cx), float(cy), angle, scale), rows, cols
    sn, cs = abs(math.sin(angle * _PI / 180.0)), abs(math.cos(angle * _PI / 180.0))
    rw = math.ceil(float(rows) * sn + float(cols) * cs)
    rh = math.ceil(float(cols) * sn + float(rows) * cs)
    M = orc.get_rotation_matrix_2d(float(F(math.ceil(rw / 2.0))), float(F(math.ceil(rh / 2.0))), angle, scale)
    M[2] += math.ceil((rw - float(cols)) / 2.0)
    M[5] += math.ceil((rh - float(rows)) / 2.0)
    return M, int(rh), int(rw)


def rotate_ex(src, angle, scale, flags, border_mode, border_value, clip, init=None, rows=None):
    """what omr_rotate_ex gives: the canvas, with `init` (default zeros) where BORDER_TRANSPARENT skips; `rows`
    restricts the computation to those destination rows (the others stay as `init`)"""
    a = np.ascontiguousarray(src, np.uint8)
    a3 = a if a.ndim == 3 else a[:, :, None]
    h, w, cn = a3.shape
    M, dr, dc = rotate_geometry(h, w, angle, scale, clip)
    interp = flags & 7
    if interp == 3:
        interp = 1
    Minv = M if flags & INVERSE_MAP else orc.invert_affine(M)
    ad, bd, X0, Y0 = orc.warp_tables(Minv, dc, dr, 512 if interp == 0 else 16)
    ad, bd, X0, Y0 = (v.astype(np.int64) for v in (ad, bd, X0, Y0))
    out = np.zeros((dr, dc, cn), np.uint8) if init is None else np.array(init, np.uint8).reshape(dr, dc, cn).copy()
    sel = np.arange(dr) if rows is None else np.asarray(rows)
    K = TAPS[interp]
    step = max(1, (1 << 21) // max(1, dc * K * K * cn))
    cval = [int(v) for v in border_value]
    for i in range(0, len(sel), step):
        rr = sel[i:i + step]
        Xf = (X0[rr][:, None] + ad[None, :]).ravel()
        Yf = (Y0[rr][:, None] + bd[None, :]).ravel()
        val, keep = remap(a3, Xf, Yf, interp, border_mode, cval)
        blk = out[rr].reshape(-1, cn)
        blk[keep] = val[keep]
        out[rr] = blk.reshape(len(rr), dc, cn)
    return out if a.ndim == 3 else out[:, :, 0]
