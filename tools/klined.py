"""The detectors' line pictures of A4 edge maps (2480 x 3508): omr_lined_picture_batch_device on --n (64) resident edge
maps with the segments the Hough path finds on them -- omr_canny(50, 150) of a synthetic A4 sheet, omr_hough_lines_p(1,
pi/180, 0, --min-line-length, --max-line-gap) -- every picture with the same map and list in buffers of its own.
  default   times of whole calls between HIP events (median of --reps after 3 warm-up calls; a call holds the prepare
            kernel, the read-back of the end-point verdict, the drawing launch and the final synchronise), segments per
            picture, bytes/s against the compulsory traffic: rows x cols read + 3 x rows x cols written + 16 bytes a
            segment, per picture.  One picture is compared with tests/lined_ref.py.
  --trace   only --reps calls: the body of a `rocprofv3 --kernel-trace --stats` run, which gives the kernels' own times.
Usage: python tools/klined.py [--n 64] [--reps 10] [--md FILE] [--json FILE] [--trace]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

import lined_ref as lr
from oics import _lib, hough, synth

ROWS, COLS = 3508, 2480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--min-line-length", type=float, default=30.0)
    ap.add_argument("--max-line-gap", type=float, default=5.0)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _lib.lib()
    if lib.omr_device_count() < 1:
        sys.exit("klined needs a HIP device: a time from a CPU says nothing about the kernels")
    sheet = np.ascontiguousarray(synth.make_binary_card(ROWS, COLS, 2, skew=1.1)[0])
    edges = hough.canny(sheet, 50.0, 150.0)
    lines = hough.hough_lines_p(edges, 1.0, math.pi / 180.0, 0, args.min_line_length, args.max_line_gap)
    n, k, img = args.n, len(lines), ROWS * COLS
    d_e = torch.from_numpy(edges).cuda().reshape(1, img).repeat(n, 1).contiguous()
    d_l = torch.from_numpy(np.ascontiguousarray(lines).reshape(1, -1)).cuda().repeat(n, 1).contiguous()
    d_o = torch.empty((n, 3 * img), dtype=torch.uint8, device="cuda")
    off = (np.arange(n + 1) * k).astype(np.int32)
    bgr = (C.c_uint8 * 3)(*lr.COLOR)

    def call():
        rc = lib.omr_lined_picture_batch_device(C.c_void_p(d_e.data_ptr()), n, img, COLS, ROWS, COLS, C.c_void_p(d_l.data_ptr()),
                                                off.ctypes.data_as(_lib.i32p), bgr, C.c_void_p(d_o.data_ptr()), 3 * img,
                                                3 * COLS, None)
        assert rc == 0, lib.omr_last_error()

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    if args.trace:
        for _ in range(args.reps):
            call()
        torch.cuda.synchronize()
        print("traced %d calls, %d edge maps each, %d segments a picture" % (args.reps, n, k))
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(args.reps):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = float(np.median(ts))
    nbytes = n * (4 * img + 16 * k)
    r = {"rows": ROWS, "cols": COLS, "pictures": n, "segments_per_picture": k, "ms_per_call": round(ms, 4),
         "us_per_picture": round(ms * 1e3 / n, 2), "compulsory_MB": round(nbytes / 1e6, 1), "GBps": round(nbytes / ms / 1e6, 1),
         "share_8TBps": round(nbytes / ms / 1e6 / 8000, 4)}
    got = d_o[n - 1].cpu().numpy().reshape(ROWS, COLS, 3)
    r["equals_restatement"] = bool(np.array_equal(got, lr.lined_picture(edges, lines)))
    print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(r, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| pictures | segments / picture | ms / call | us / picture | compulsory MB | GB/s | share of 8 TB/s |\n"
                    "|---|---|---|---|---|---|---|\n")
            f.write("| %d | %d | %.4f | %.2f | %.1f | %.1f | %.4f |\n" % (n, k, ms, r["us_per_picture"], r["compulsory_MB"],
                                                                      r["GBps"], r["share_8TBps"]))


if __name__ == "__main__":
    main()
