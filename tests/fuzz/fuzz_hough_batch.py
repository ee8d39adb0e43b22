"""Randomised parity run of omr_hough_angles_batch_device against omr_get_angle_with_hough_ex, one call per scan: random
batch sizes (1..9), shapes (24..400 per side), channels 1 / 3 / 4, min_line_length and max_line_gap on both sides of
what the scans hold (so that batches mix scans with many, few and no segments), blank scans, random buffer offsets, row
pitches and strides of the scans and of the pictures (half of the cases dword-aligned throughout) over a pattern-filled
picture block.  Per scan the batch must give the per-call angle bit for bit, or -215 where the per-call form gives it;
every picture must be the per-call picture byte for byte, and every other byte of the picture block -- the slots of
scans without a segment, pitch padding, gaps -- must keep its pattern.  Half of the cases also run without pictures.
Usage: python tests/fuzz/fuzz_hough_batch.py [cases] [seed]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

from oics import _lib, hough, synth


def make_scan(rng, rows, cols, cn):
    kind = rng.random()
    if kind < 0.15:
        g = np.full((rows, cols), int(rng.integers(0, 256)), np.uint8)  # blank: no segment
    elif kind < 0.3:
        g = (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)   # noise: edges everywhere, short segments
    else:
        skew = None if rng.random() < 0.6 else float(rng.uniform(-45, 45))
        g = synth.make_card(rows, cols, int(rng.integers(0, 1 << 30)), skew)[0]
    if cn == 1:
        return g
    img = np.stack([g] * cn, axis=2).astype(np.int16)
    img[:, :, :3] += rng.integers(-12, 13, size=(rows, cols, 3), dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def run_case(rng):
    n = int(rng.integers(1, 10))
    rows, cols, cn = int(rng.integers(24, 401)), int(rng.integers(24, 401)), int(rng.choice([1, 3, 4]))
    mll = float(rng.choice([0.0, 5.0, 20.0, 0.3 * min(rows, cols), 0.6 * max(rows, cols), 1.5 * max(rows, cols)]))
    mlg = float(rng.choice([0.0, 1.0, 4.0, 10.0, 63.0, 64.0, 200.0]))
    case = (n, rows, cols, cn, mll, mlg)
    scans = [make_scan(rng, rows, cols, cn) for _ in range(n)]
    row = cols * cn
    if rng.random() < 0.5:  # dword-aligned throughout
        so = do = 0
        sp, dp = (row + 3) & ~3, (3 * cols + 3) & ~3
        ss, ds = rows * sp + 4 * int(rng.integers(0, 3)), rows * dp + 4 * int(rng.integers(0, 3))
    else:
        so, do = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        sp, dp = row + int(rng.integers(0, 5)), 3 * cols + int(rng.integers(0, 5))
        ss, ds = rows * sp + int(rng.integers(0, 7)), rows * dp + int(rng.integers(0, 7))
    sbuf = rng.integers(0, 256, so + n * ss + 4, dtype=np.uint8)
    for i, a in enumerate(scans):
        sbuf[so + i * ss: so + i * ss + rows * sp].reshape(rows, sp)[:, :row] = a.reshape(rows, row)
    d_s = torch.from_numpy(sbuf).cuda()
    pattern = rng.integers(0, 256, do + n * ds + 4, dtype=np.uint8)
    d_b = torch.from_numpy(pattern).cuda()
    try:
        ang, rc, nl = hough.hough_angles_batch_device(d_s.data_ptr() + so, n, ss, rows, cols, cn, sp, mll, mlg,
                                                      d_lined=d_b.data_ptr() + do, lined_stride_bytes=ds, lined_step=dp)
        if rng.random() < 0.5:
            ang2, rc2, nl2 = hough.hough_angles_batch_device(d_s.data_ptr() + so, n, ss, rows, cols, cn, sp, mll, mlg)
            if not (np.array_equal(ang.view(np.uint64), ang2.view(np.uint64)) and np.array_equal(rc, rc2) and np.array_equal(nl, nl2)):
                return case, "the call without pictures answers differently"
    except _lib.OmrError as e:
        return case, "batch rc %d: %s" % (e.code, e.message)
    want = pattern.copy()
    for i, a in enumerate(scans):
        try:
            e_ang, pic = hough.get_angle_with_hough(a, mll, mlg, want_picture=True)
        except _lib.OmrError as e:
            if e.code != -215:
                return case, "per-call rc %d" % e.code
            if rc[i] != -215 or ang[i] != 0.0 or nl[i] != 0:
                return case, "scan %d: no segment per call, batch rc %d, %d segments" % (i, rc[i], nl[i])
            continue
        if rc[i] != 0 or np.float64(ang[i]).view(np.uint64) != np.float64(e_ang).view(np.uint64) or nl[i] < 1:
            return case, "scan %d: angle %r rc %d, per call %r" % (i, ang[i], rc[i], e_ang)
        want[do + i * ds: do + i * ds + rows * dp].reshape(rows, dp)[:, : 3 * cols] = pic.reshape(rows, 3 * cols)
    got = d_b.cpu().numpy()
    if not np.array_equal(got, want):
        return case, "%d picture bytes differ" % int((got != want).sum())
    return case, None


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
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
