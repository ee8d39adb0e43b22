"""erode on device-resident A4 sheets (2480 x 3508, gray and BGR) through omr_morph_device, one call at a time between
HIP events: the median of 30 calls after 5 warm-up calls per row.  Every row here is ONE launch (no intermediate
image), so a call's time is a kernel's time plus its launch.  GB/s counts the compulsory bytes (the image read once
and written once).  The yardstick row is omr_erode3_device, the front end's hard-wired 3 x 3 cross x 3, on the same
gray input in the same process; the general path's row for it is ELLIPSE 3 x 3 x 3.
Usage: python tools/bench_morph.py [--reps 30] [--md FILE] [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "omr-img-corrector_amd"))
import numpy as np
import torch

from oics import _lib, synth

ROWS, COLS = 3508, 2480
RECT, CROSS, ELLIPSE = 0, 1, 2
NAMES = {RECT: "RECT", CROSS: "CROSS", ELLIPSE: "ELLIPSE"}
# (shape, k, iterations): the elements scan clean-up uses, and the rectangles that show the separable path's cost
CASES = [(CROSS, 3, 1), (CROSS, 3, 3), (ELLIPSE, 3, 3), (ELLIPSE, 5, 1), (ELLIPSE, 15, 1), (RECT, 3, 1), (RECT, 31, 1), (RECT, 3, 15)]


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _lib.lib()
    if lib.omr_device_count() < 1:
        sys.exit("bench_morph needs a HIP device: a time from a CPU says nothing about the kernels")
    gray, _ = synth.make_card(ROWS, COLS, 2)
    rows = []

    def row(name, cn, ms):
        nbytes = 2 * ROWS * COLS * cn
        r = {"case": name, "channels": cn, "ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1),
             "share_8TBps": round(nbytes / ms / 1e6 / 8000, 4), "ns_per_pixel": round(ms * 1e6 / (ROWS * COLS), 4)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    for cn in (1, 3):
        host = gray if cn == 1 else np.repeat(gray[:, :, None], 3, axis=2).copy()
        src = torch.from_numpy(host).cuda()
        dst = torch.empty_like(src)
        if cn == 1:
            def yard():
                assert lib.omr_erode3_device(C.c_void_p(src.data_ptr()), COLS, ROWS, COLS, C.c_void_p(dst.data_ptr()), COLS, None) == 0
            row("omr_erode3_device (yardstick)", 1, timed(yard, args.reps))
        for shape, k, it in CASES:
            def call():
                rc = lib.omr_morph_device(C.c_void_p(src.data_ptr()), COLS * cn, ROWS, COLS, cn, 0, shape, k, k, -1, -1, it,
                                          C.c_void_p(dst.data_ptr()), COLS * cn, None)
                assert rc == 0, lib.omr_last_error()
            row("%s %d x %d x %d" % (NAMES[shape], k, k, it), cn, timed(call, args.reps))

    by = {(r["case"], r["channels"]): r["ms"] for r in rows}
    ratios = {"general ELLIPSE 3 x 3 x 3 over omr_erode3_device (gray)": by[("ELLIPSE 3 x 3 x 3", 1)] / by[("omr_erode3_device (yardstick)", 1)]}
    for cn in (1, 3):
        ratios["RECT 31 x 31 over RECT 3 x 3 (%d ch)" % cn] = by[("RECT 31 x 31 x 1", cn)] / by[("RECT 3 x 3 x 1", cn)]
    for k, v in ratios.items():
        print("%s: %.2f" % (k, v))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": ROWS, "cols": COLS, "reps": args.reps, "cases": rows, "ratios": ratios}, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| case | ch | ms / call | GB/s | share of 8 TB/s | ns / pixel |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %.4f | %.1f | %.4f | %.4f |\n" % (r["case"], r["channels"], r["ms"], r["GBps"], r["share_8TBps"], r["ns_per_pixel"]))
            f.write("\n")
            for k, v in ratios.items():
                f.write("* %s: %.2f\n" % (k, v))


if __name__ == "__main__":
    main()
