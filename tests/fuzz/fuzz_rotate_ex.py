"""Randomised parity run of omr_rotate_device_ex against the numpy restatement of warpAffine (tests/warp_ref.py):
random shapes (1..90 per side), channels 1..4, interpolations 0..4, border modes 0..5, WARP_INVERSE_MAP and
WARP_FILL_OUTLIERS, clip, angles in [-180, 180] (a third of them on the 90-degree grid) and scales in [0.2, 3]
(LDS-staged and global-fallback tiles), random per-channel border values, odd buffer offsets and pitches over a
sentinel canvas.  Every byte of the canvas is compared; bytes past each canvas row must stay untouched.
With a third argument `float64` (off by default: the cases and their checks are then exactly as without it) the cases
that interpolate (LINEAR, CUBIC, LANCZOS4) and write every pixel (not BORDER_TRANSPARENT) run on smooth content of the
drawn shape instead of the drawn noise, and the canvas is also held to tests/geom_exact.py's float64 warp within its
general bound.
Usage: python tests/fuzz/fuzz_rotate_ex.py [cases] [seed] [float64]"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

import warp_ref as wr
from oics import _lib

SENTINEL = 0x5A


def run_case(rng, float64=False):
    rows, cols, cn = int(rng.integers(1, 91)), int(rng.integers(1, 91)), int(rng.integers(1, 5))
    interp, mode, clip = int(rng.choice([0, 1, 2, 3, 4])), int(rng.integers(0, 6)), int(rng.integers(0, 2))
    flags = interp | (16 if rng.random() < 0.3 else 0) | (8 if rng.random() < 0.2 else 0)
    angle = float(rng.choice([0, 90, -90, 180])) if rng.random() < 0.33 else float(rng.uniform(-180, 180))
    scale = float(rng.uniform(0.2, 3.0))
    border = tuple(int(v) for v in rng.integers(0, 256, 4))
    a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    if rng.random() < 0.5:
        a[(np.add.outer(np.arange(rows), np.arange(cols)) % 2).astype(bool)] = 255
    float64 = float64 and interp != 0 and mode != wr.TRANSPARENT
    if float64:  # after every draw, so the stream of cases is the same with and without the option
        import geom_cases
        a = geom_cases.smooth(rows, cols, cn, seed=rows * 91 + cols)
    dr, dc = C.c_int32(), C.c_int32()
    assert _lib.lib().omr_rotate_size(rows, cols, angle, clip, C.byref(dr), C.byref(dc)) == 0
    dr, dc = dr.value, dc.value
    so, do = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    sp, dp = cols * cn + int(rng.integers(0, 5)), dc * cn + int(rng.integers(0, 5))
    sbuf = np.zeros(so + rows * sp + 4, np.uint8)
    sbuf[so:so + rows * sp].reshape(rows, sp)[:, :cols * cn] = a.reshape(rows, cols * cn)
    d_s = torch.from_numpy(sbuf).cuda()
    d_d = torch.full((do + dr * dp + 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = (C.c_uint8 * 4)(*border)
    rc = _lib.lib().omr_rotate_device_ex(C.c_void_p(d_s.data_ptr() + so), sp, rows, cols, cn, angle, scale, flags, mode,
                                         C.cast(b, _lib.u8p), clip, C.c_void_p(d_d.data_ptr() + do), dp, dr, dc, None)
    torch.cuda.synchronize()
    case = (rows, cols, cn, interp, flags, mode, clip, angle, scale)
    if rc != 0:
        return case, "rc %d" % rc
    out = d_d.cpu().numpy()
    grid = out[do:do + dr * dp].reshape(dr, dp)
    if (out[:do] != SENTINEL).any() or (out[do + dr * dp:] != SENTINEL).any() or (grid[:, dc * cn:] != SENTINEL).any():
        return case, "wrote outside the canvas"
    got = grid[:, :dc * cn].reshape(dr, dc, cn)
    exp = wr.rotate_ex(a, angle, scale, flags, mode, border, clip, init=np.full((dr, dc, cn), SENTINEL, np.uint8))
    if not np.array_equal(got, exp):
        return case, "%d bytes differ" % int((got != exp).sum())
    if float64:
        import geom_exact as gx
        M, er, ec = gx.rotate_geometry(rows, cols, angle, scale, clip, bool(flags & wr.INVERSE_MAP))
        if (er, ec) != (dr, dc):
            return case, "canvas %r, float64 geometry %r" % ((dr, dc), (er, ec))
        bad, at, _ = gx.worst(got, gx.warp(a, M, dr, dc, interp, mode, border), gx.general_warp_bound(interp, a, mode, border))
        if bad:
            return case, "%d pixels over the float64 bound, worst (index, got, exact, bound) %r" % (bad, at)
    return case, None


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    float64 = len(sys.argv) > 3 and sys.argv[3] == "float64"
    bad = []
    for _ in range(cases):
        case, err = run_case(rng, float64)
        if err:
            bad.append((case, err))
    print("cases", cases, "mismatches", len(bad), bad[:5])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
