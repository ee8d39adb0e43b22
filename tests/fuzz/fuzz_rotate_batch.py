"""Randomised parity run of omr_rotate_batch_device_ex against omr_rotate_device_ex, one call per image: random batch
sizes (1..9), shapes (1..90 per side), channels 1..4, interpolations 0..4, border modes 0..5, WARP_INVERSE_MAP and
WARP_FILL_OUTLIERS, clip, an angle per image in [-180, 180] (a third of them on the 90-degree grid), scales in [0.2, 3]
(LDS-staged and global-fallback tiles), random border values, slots larger than the largest canvas, random buffer
offsets, row pitches and image strides (half of the cases dword-aligned throughout: the dword staging) over a
pattern-filled block of slots.  The batch's block must equal, byte for byte, the block the per-call entry point
fills -- canvases, guard bytes and gaps -- and out_size must be omr_rotate_size's answers.
Usage: python tests/fuzz/fuzz_rotate_batch.py [cases] [seed]"""
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

from oics import _lib


def run_case(rng):
    L = _lib.lib()
    n = int(rng.integers(1, 10))
    rows, cols, cn = int(rng.integers(1, 91)), int(rng.integers(1, 91)), int(rng.integers(1, 5))
    interp, mode, clip = int(rng.choice([0, 1, 2, 3, 4])), int(rng.integers(0, 6)), int(rng.integers(0, 2))
    flags = interp | (16 if rng.random() < 0.3 else 0) | (8 if rng.random() < 0.2 else 0)
    angles = np.array([float(rng.choice([0, 90, -90, 180])) if rng.random() < 0.33 else float(rng.uniform(-180, 180))
                       for _ in range(n)])
    scale = float(rng.uniform(0.2, 3.0))
    border = (C.c_uint8 * 4)(*[int(v) for v in rng.integers(0, 256, 4)])
    case = (n, rows, cols, cn, flags, mode, clip, angles.tolist(), scale)
    mr, mc = C.c_int32(), C.c_int32()
    sizes = np.zeros(2 * n, np.int32)
    if L.omr_rotate_batch_canvas(rows, cols, angles.ctypes.data_as(_lib.f64p), n, clip, C.byref(mr), C.byref(mc),
                                 sizes.ctypes.data_as(_lib.i32p)) != 0:
        return case, "canvas refused"
    sr, sc = mr.value + int(rng.integers(0, 3)), mc.value + int(rng.integers(0, 3))
    if rng.random() < 0.5:  # dword-aligned throughout
        so = do = 0
        sp, dp = (cols * cn + 3) & ~3, (sc * cn + 3) & ~3
        ss, ds = rows * sp + 4 * int(rng.integers(0, 3)), sr * dp + 4 * int(rng.integers(0, 3))
    else:
        so, do = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        sp, dp = cols * cn + int(rng.integers(0, 5)), sc * cn + int(rng.integers(0, 5))
        ss, ds = rows * sp + int(rng.integers(0, 7)), sr * dp + int(rng.integers(0, 7))
    if rng.random() < 0.1:
        ss = 0  # one image, n angles
    sbuf = rng.integers(0, 256, so + (n - 1) * ss + rows * sp + 4, dtype=np.uint8)
    if rng.random() < 0.5:
        sbuf[::2] = 255
    d_s = torch.from_numpy(sbuf).cuda()
    pattern = torch.from_numpy(rng.integers(0, 256, do + n * ds + 4, dtype=np.uint8)).cuda()
    d_b, d_p = pattern.clone(), pattern.clone()
    torch.cuda.synchronize()
    got = np.zeros(2 * n, np.int32)
    rc = L.omr_rotate_batch_device_ex(C.c_void_p(d_s.data_ptr() + so), n, ss, sp, rows, cols, cn, angles.ctypes.data_as(_lib.f64p),
                                      scale, flags, mode, C.cast(border, _lib.u8p), clip, C.c_void_p(d_b.data_ptr() + do), ds, dp,
                                      sr, sc, got.ctypes.data_as(_lib.i32p), None)
    torch.cuda.synchronize()
    if rc != 0:
        return case, "batch rc %d" % rc
    if not np.array_equal(got, sizes):
        return case, "out_size differs"
    for i in range(n):
        dr, dc = C.c_int32(), C.c_int32()
        if L.omr_rotate_size(rows, cols, angles[i], clip, C.byref(dr), C.byref(dc)) != 0 or (dr.value, dc.value) != tuple(sizes[2 * i:2 * i + 2]):
            return case, "canvas %d is not omr_rotate_size's" % i
        rc = L.omr_rotate_device_ex(C.c_void_p(d_s.data_ptr() + so + i * ss), sp, rows, cols, cn, float(angles[i]), scale, flags,
                                    mode, C.cast(border, _lib.u8p), clip, C.c_void_p(d_p.data_ptr() + do + i * ds), dp, dr.value,
                                    dc.value, None)
        if rc != 0:
            return case, "per-call rc %d" % rc
    torch.cuda.synchronize()
    if not torch.equal(d_b, d_p):
        return case, "%d bytes differ" % int((d_b != d_p).sum())
    return case, None


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    bad = []
    for _ in range(cases):
        case, err = run_case(rng)
        if err:
            bad.append((case, err))
    print("cases", cases, "mismatches", len(bad), bad[:5])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
