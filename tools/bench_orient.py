"""The orientation kernel and what it costs the files-to-files flow (development aid).

1. omr_orient_batch_device on 256 device-resident A4 colour images (3508 x 2480 x 3), every code 1..8: a host clock around
   the synchronous call (record upload, one launch, drain), `--reps` calls per code after a warm-up, median; bytes moved
   (one read plus one write of every image) over the time, and that over the 8 TB/s HBM roofline of DESIGN.md section 4.0.
2. omr_deskew_with_projections_batch_streams at the reference benchmark's parameters ((45, 0.2, 0.2), LINEAR, quality 100)
   on the dataset's sheets as gray JPEG, channels 3, `--n` files a call: as they are (no sheet to turn: the flow must not
   pay for the feature), and with every sheet tagged orientation 6 (scratch decode plus the turn).
--pkg DIR runs part 2 against another build of the package (a checkout of the parent commit, built), where the tagged
batch is skipped when that build refuses it.
Usage: python tools/bench_orient.py [--images N] [--reps R] [--n N] [--passes P] [--pkg DIR] [--flows-only] [--commit TEXT]
       [--out FILE]
Writes a markdown report (default profiles/r22_orient.md) and prints it."""
import argparse
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = (45, 0.2, 0.2)
HBM = 8e12
A4 = (3508, 2480, 3)


def tag(stream, code):
    """the JPEG stream with an EXIF orientation behind SOI (little-endian TIFF, one IFD entry)"""
    tiff = b"II*\x00" + struct.pack("<I", 8) + struct.pack("<H", 1) + struct.pack("<HHIHH", 0x0112, 3, 1, code, 0) + struct.pack("<I", 0)
    body = b"Exif\x00\x00" + tiff
    return stream[:2] + b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body + stream[2:]


def kernel_part(images, reps):
    import torch
    from oics import transfer
    rows, cols, cn = A4
    step = cols * cn
    stride = rows * step
    g = torch.Generator(device="cuda:0").manual_seed(1)
    src = torch.randint(0, 256, (images * stride,), dtype=torch.uint8, device="cuda:0", generator=g)
    dst = torch.empty(images * stride, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    moved = 2.0 * images * stride
    out = ["| code | ms (median of %d) | min .. max | TB/s moved | of the HBM roofline |" % reps, "|---|---|---|---|---|"]
    for code in range(1, 9):
        dr, dc = (cols, rows) if code >= 5 else (rows, cols)
        call = lambda: transfer.orient_batch_device(src.data_ptr(), stride, step, rows, cols, dst.data_ptr(), stride, dc * cn, dr, dc,  # noqa: E731
                                                    cn, None, [code] * images)
        call()
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t) * 1e3)
        med = float(np.median(ms))
        out.append("| %d | %.3f | %.3f .. %.3f | %.2f | %.2f |" % (code, med, min(ms), max(ms), moved / med / 1e9, moved / (med * 1e-3) / HBM))
    # one image against numpy, so that the table times a kernel that turns
    one = src[:stride].cpu().numpy().reshape(rows, cols, cn)
    got = dst[:stride].cpu().numpy().reshape(cols, rows, cn)          # the last code was 8: transpose, flip top-bottom
    assert (got == np.swapaxes(one, 0, 1)[::-1]).all()
    return out


def flow_part(n, passes):
    from oics import projection
    d = os.path.join(ROOT, "tests", "golden", "dataset")
    sheets = [open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")]
    plain = [sheets[i % len(sheets)] for i in range(n)]
    out = ["| batch | files | sheets/s, each pass | median |", "|---|---|---|---|"]
    for name, streams in (("as stored (no sheet to turn)", plain), ("every sheet tagged orientation 6", [tag(s, 6) for s in plain])):
        run = lambda: projection.deskew_streams(streams, *SWEEP, interp=1, quality=100, channels=3)  # noqa: E731
        ang, rc, outs = run()
        if (np.asarray(rc) != 0).any():
            out.append("| %s | %d | refused by this build (scan_rc %d) | - |" % (name, n, int(np.asarray(rc)[0])))
            continue
        rate = []
        for _ in range(passes):
            t = time.perf_counter()
            run()
            rate.append(n / (time.perf_counter() - t))
        out.append("| %s | %d | %s | %.0f |" % (name, n, ", ".join("%.0f" % r for r in rate), float(np.median(rate))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "omr-img-corrector_amd"))
    ap.add_argument("--flows-only", action="store_true")
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_orient.md"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    import oics
    if oics.lib().omr_device_count() < 1:
        raise SystemExit("bench_orient needs a GPU: there is nothing to time without one")
    lines = ["# EXIF orientation on the device (tools/bench_orient.py)", "", "Commit: %s.  Package: %s.  One MI355X." % (a.commit, a.pkg), ""]
    if not a.flows_only:
        lines += ["## omr_orient_batch_device, %d resident A4 colour images (%d x %d x %d) a call" % ((a.images,) + A4), "",
                  "Host clock around the synchronous call (record upload, one launch, drain).  Bytes moved = one read plus one "
                  "write of every image; roofline = 8 TB/s (DESIGN.md section 4.0).", ""] + kernel_part(a.images, a.reps) + [""]
    lines += ["## omr_deskew_with_projections_batch_streams, dataset sheets as gray JPEG, channels 3", "",
              "Sweep (%d, %g, %g), LINEAR, quality 100; a warm-up call, then %d timed calls." % (SWEEP + (a.passes,)), ""]
    lines += flow_part(a.n, a.passes) + [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
