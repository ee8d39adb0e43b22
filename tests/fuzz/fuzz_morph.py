"""Randomised parity run of omr_morph_device against the numpy restatement of erode / dilate (tests/morph_ref.py):
random shapes (1..90 per side), channels 1..4, both operations, the three element shapes, element sizes 1..40 per
side (every kernel of morph.hip: the rectangle chain, the LDS spans with fused and separate passes, the global
spans), any anchor, 0..6 iterations (18 now and then, past what one launch fuses), odd buffer offsets and pitches
over a sentinel canvas.  Every byte is compared; bytes past each row must stay untouched.  Stops at the first
mismatch, prints the case and exits 1.
Usage: python tests/fuzz/fuzz_morph.py [cases] [seed]"""
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

import morph_ref as mr
from oics import _lib

SENTINEL = 0x5A


def device_morph(a, op, shape, size, anchor, iterations, so=0, sp=None, do=0, dp=None):
    """a: (rows, cols, cn) u8 -> (rc, result or None, error text or None) of omr_morph_device on buffers that start
    `so` / `do` bytes into their allocations with pitches sp / dp, the destination filled with SENTINEL"""
    rows, cols, cn = a.shape
    sp = cols * cn if sp is None else sp
    dp = cols * cn if dp is None else dp
    sbuf = np.zeros(so + rows * sp + 4, np.uint8)
    sbuf[so:so + rows * sp].reshape(rows, sp)[:, :cols * cn] = a.reshape(rows, cols * cn)
    d_s = torch.from_numpy(sbuf).cuda()
    d_d = torch.full((do + rows * dp + 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = _lib.lib().omr_morph_device(C.c_void_p(d_s.data_ptr() + so), sp, rows, cols, cn, op, shape, size[0], size[1],
                                     anchor[0], anchor[1], iterations, C.c_void_p(d_d.data_ptr() + do), dp, None)
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, "rc %d: %s" % (rc, _lib.lib().omr_last_error().decode())
    out = d_d.cpu().numpy()
    grid = out[do:do + rows * dp].reshape(rows, dp)
    if (out[:do] != SENTINEL).any() or (out[do + rows * dp:] != SENTINEL).any() or (grid[:, cols * cn:] != SENTINEL).any():
        return rc, None, "wrote outside the image's rows"
    if (d_s.cpu().numpy() != sbuf).any():
        return rc, None, "wrote to the source"
    return rc, grid[:, :cols * cn].reshape(rows, cols, cn).copy(), None


def run_case(rng):
    rows, cols, cn = int(rng.integers(1, 91)), int(rng.integers(1, 91)), int(rng.integers(1, 5))
    op, shape = int(rng.integers(0, 2)), int(rng.integers(0, 3))
    big = rng.random() < 0.15
    kw, kh = (int(v) for v in rng.integers(1, 41 if big else 12, 2))
    anchor = (-1, -1) if rng.random() < 0.3 else (int(rng.integers(0, kw)), int(rng.integers(0, kh)))
    it = 18 if rng.random() < 0.05 else int(rng.integers(0, 7))
    if big and shape != mr.RECT:
        it = min(it, 2)  # the restatement walks every cell of the element in every pass
    a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    if rng.random() < 0.5:
        a[rng.random((rows, cols)) < 0.7] = 255 if op == mr.ERODE else 0  # sparse marks: long-range effects show
    so, do = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    sp, dp = cols * cn + int(rng.integers(0, 5)), cols * cn + int(rng.integers(0, 5))
    case = (rows, cols, cn, op, shape, kw, kh, anchor, it, so, sp, do, dp)
    rc, got, err = device_morph(a, op, shape, (kw, kh), anchor, it, so, sp, do, dp)
    if err:
        return case, err
    exp = mr.morph(a, op, shape, (kw, kh), anchor, it)
    if not np.array_equal(got, exp):
        return case, "%d bytes differ" % int((got != exp).sum())
    return case, None


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    for i in range(cases):
        case, err = run_case(rng)
        if err:
            print("case", i, case, "(rows, cols, cn, op, shape, kw, kh, anchor, it, so, sp, do, dp):", err)
            sys.exit(1)
    print("cases", cases, "mismatches 0")
    sys.exit(0)


if __name__ == "__main__":
    main()
