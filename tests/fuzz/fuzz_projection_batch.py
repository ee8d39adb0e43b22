"""Randomised parity run of omr_projection_batch_front_device / omr_projection_batch_run_device against the CPU oracle:
random batch sizes (1..4), shapes (8..160 per side), channels (1 or 3), resize scales (shrinks down to 0.05, integer
factors, 1.0, enlargements up to 2.2), sweeps (max_angle 1..6, step 0.25 / 0.5 / 1), random buffer offsets, row pitches
and scan strides (half of the cases dword-aligned throughout: the dword staging).  Every scan's working image must
equal oracle.scale_self's byte for byte inside a sentinel-filled destination whose other bytes survive, and its angle
(as f64 bits) and best index must be oracle.get_angle_with_projections'.
Usage: python tests/fuzz/fuzz_projection_batch.py [cases] [seed]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

from oics import _lib, projection
from oracle import oracle as orc


def run_case(rng):
    n = int(rng.integers(1, 5))
    rows, cols, cn = int(rng.integers(8, 161)), int(rng.integers(8, 161)), int(rng.choice([1, 3]))
    scale = float(rng.choice([rng.uniform(0.05, 1.0), 1.0 / int(rng.integers(2, 6)), 1.0, rng.uniform(1.0, 2.2)]))
    max_angle, step = int(rng.integers(1, 7)), float(rng.choice([0.25, 0.5, 1.0]))
    case = (n, rows, cols, cn, scale, max_angle, step)
    if int(rows * scale) < 2 or int(cols * scale) < 2:
        return case, None
    row = cols * cn
    if rng.random() < 0.5:  # dword-aligned throughout
        so, sp = 0, (row + 3) & ~3
        ss = rows * sp + 4 * int(rng.integers(0, 3))
    else:
        so, sp = int(rng.integers(0, 4)), row + int(rng.integers(0, 5))
        ss = rows * sp + int(rng.integers(0, 7))
    imgs = []
    sbuf = rng.integers(0, 256, so + (n - 1) * ss + (rows - 1) * sp + row, dtype=np.uint8)
    for i in range(n):
        a = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
        a[(np.arange(rows) % 9) < 2] //= 4  # dark rows: something for the sweep to find
        o = so + i * ss
        for y in range(rows):
            sbuf[o + y * sp:o + y * sp + row] = a[y].reshape(-1)
        imgs.append(a if cn == 3 else a[:, :, 0])
    d_s = torch.from_numpy(sbuf).cuda()
    try:
        pb = projection.ProjectionBatch(rows, cols, cn, max_angle, step, scale, n + int(rng.integers(0, 3)))
    except _lib.OmrError as e:
        return case, "create: %s" % e
    try:
        wr, wc = pb.wrows, pb.wcols
        wrow = wc * cn
        do, dp = int(rng.integers(0, 4)), wrow + int(rng.integers(0, 5))
        ds = wr * dp + int(rng.integers(0, 7))
        d = torch.full((do + n * ds + 4,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pb.front_device(d_s.data_ptr() + so, ss, sp, n, d.data_ptr() + do, ds, dp)
        ang, idx, _, _ = pb.run_device(d_s.data_ptr() + so, ss, sp, n)
    except _lib.OmrError as e:
        return case, "run: %s" % e
    finally:
        pb.close()
    got = d.cpu().numpy()
    inside = np.zeros(got.size, bool)
    for i, a in enumerate(imgs):
        o = do + i * ds
        inside[o:o + wr * dp].reshape(wr, dp)[:, :wrow] = True
        w = got[o:o + wr * dp].reshape(wr, dp)[:, :wrow]
        ref = orc.scale_self(a, scale).reshape(wr, wrow)
        if not (w == ref).all():
            return case, "scan %d: %d bytes of the working image differ" % (i, int((w != ref).sum()))
        oang, oidx = orc.get_angle_with_projections(a, max_angle, step, scale)
        if np.float64(ang[i]).view(np.uint64) != np.float64(oang).view(np.uint64) or idx[i] != oidx:
            return case, "scan %d: angle %r idx %d, oracle %r idx %d" % (i, ang[i], idx[i], oang, oidx)
    if not (got[~inside] == 0xA5).all():
        return case, "bytes outside the working images were written"
    if not (d_s.cpu().numpy() == sbuf).all():
        return case, "the source was written"
    return case, None


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    orc.build()
    bad = []
    for _ in range(cases):
        case, err = run_case(rng)
        if err:
            bad.append((case, err))
    print("cases", cases, "mismatches", len(bad), bad[:5])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
