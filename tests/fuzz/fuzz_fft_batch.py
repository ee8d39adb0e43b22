"""Randomised parity run of omr_fft_angles_batch_device against omr_get_angle_with_fft_ex, one call per scan: random
batch sizes (1..19: up to two full launch groups of 8 and a short one), shapes (24..400 per side: powers of two, mixed
radix and chirp lengths as they fall), Canny thresholds, min_line_length and max_line_gap on both sides of what the
spectra hold (so that batches mix scans with many, few and no segments), blank scans, random buffer offsets, row pitches
and strides of the scans and of the pictures (half of the cases dword-aligned throughout) over a pattern-filled picture
block.  Per scan the batch must give the per-call angle bit for bit; every picture -- the bare edge picture of a scan
without a segment included -- must be the per-call picture byte for byte, and every other byte of the picture block
(pitch padding, gaps) must keep its pattern.  Half of the cases also run without pictures.
Usage: python tests/fuzz/fuzz_fft_batch.py [cases] [seed]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

from oics import _lib, fft, synth


def make_scan(rng, rows, cols):
    kind = rng.random()
    if kind < 0.15:
        return np.full((rows, cols), int(rng.integers(0, 256)), np.uint8)  # blank: a flat spectrum picture, no segment
    if kind < 0.3:
        return (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)   # noise
    skew = None if rng.random() < 0.6 else float(rng.uniform(-45, 45))
    return synth.make_card(rows, cols, int(rng.integers(0, 1 << 30)), skew)[0]


def run_case(rng):
    n = int(rng.integers(1, 20))
    rows, cols = int(rng.integers(24, 401)), int(rng.integers(24, 401))
    c1, c2 = [(50.0, 150.0), (30.0, 90.0), (150.0, 50.0), (10.0, 300.0)][int(rng.integers(0, 4))]
    mll = float(rng.choice([0.0, 5.0, 20.0, 40.0, 100.0, 0.6 * max(rows, cols)]))
    mlg = float(rng.choice([0.0, 1.0, 5.0, 15.0, 64.0]))
    case = (n, rows, cols, c1, c2, mll, mlg)
    scans = [make_scan(rng, rows, cols) for _ in range(n)]
    if rng.random() < 0.5:  # dword-aligned throughout
        so = do = 0
        sp, dp = (cols + 3) & ~3, (3 * cols + 3) & ~3
        ss, ds = rows * sp + 4 * int(rng.integers(0, 3)), rows * dp + 4 * int(rng.integers(0, 3))
    else:
        so, do = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        sp, dp = cols + int(rng.integers(0, 5)), 3 * cols + int(rng.integers(0, 5))
        ss, ds = rows * sp + int(rng.integers(0, 7)), rows * dp + int(rng.integers(0, 7))
    sbuf = rng.integers(0, 256, so + n * ss + 4, dtype=np.uint8)
    for i, a in enumerate(scans):
        sbuf[so + i * ss: so + i * ss + rows * sp].reshape(rows, sp)[:, :cols] = a
    d_s = torch.from_numpy(sbuf).cuda()
    pattern = rng.integers(0, 256, do + n * ds + 4, dtype=np.uint8)
    d_b = torch.from_numpy(pattern).cuda()
    try:
        ang, nl = fft.fft_angles_batch_device(d_s.data_ptr() + so, n, ss, rows, cols, sp, c1, c2, mll, mlg,
                                              d_lined=d_b.data_ptr() + do, lined_stride_bytes=ds, lined_step=dp)
        if rng.random() < 0.5:
            ang2, nl2 = fft.fft_angles_batch_device(d_s.data_ptr() + so, n, ss, rows, cols, sp, c1, c2, mll, mlg)
            if not (np.array_equal(ang.view(np.uint64), ang2.view(np.uint64)) and np.array_equal(nl, nl2)):
                return case, "the call without pictures answers differently"
    except _lib.OmrError as e:
        return case, "batch rc %d: %s" % (e.code, e.message)
    want = pattern.copy()
    for i, a in enumerate(scans):
        try:
            e_ang, pic = fft.get_angle_with_fft(a, c1, c2, mll, mlg, want_picture=True)
        except _lib.OmrError as e:
            return case, "per-call rc %d: %s" % (e.code, e.message)
        if np.float64(ang[i]).view(np.uint64) != np.float64(e_ang).view(np.uint64):
            return case, "scan %d: angle %r (%d segments), per call %r" % (i, ang[i], nl[i], e_ang)
        want[do + i * ds: do + i * ds + rows * dp].reshape(rows, dp)[:, : 3 * cols] = pic.reshape(rows, 3 * cols)
    got = d_b.cpu().numpy()
    if not np.array_equal(got, want):
        return case, "%d picture bytes differ" % int((got != want).sum())
    return case, (int((nl == 0).sum()), int((nl > 1).sum()))


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    bad, empty, voted = [], 0, 0
    for _ in range(cases):
        case, res = run_case(rng)
        if isinstance(res, str):
            bad.append((case, res))
        else:
            empty += res[0]
            voted += res[1]
    print("cases", cases, "scans without a segment", empty, "scans with two or more", voted, "mismatches", len(bad), bad[:5])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
