"""get_angle_with_hough on resident batches: omr_hough_angles_batch_device with and without the line pictures, beside
omr_edges_detection_batch_device on the same scans (the same Canny and HoughLinesP work, the omr.rs vote, no pictures)
and beside the per-call loop it replaces -- omr_get_angle_with_hough and omr_get_angle_with_hough_ex, one scan a call
from host memory -- taken from --baseline-lib (a libomrdeskew.so built from the parent commit; without it the loop
runs on this library, and the output says so).
  default   scans/s for 64 and 256 scans of 1240 x 1754 and of A4 (2480 x 3508): a host clock around calls that end in
            the library's own synchronise, one warm-up call per shape and size, then --reps timed calls; median, and the
            lowest and highest rate as the spread.  The batch holds --cards distinct synthetic cards, repeated; the
            per-call loop runs over the first --loop-scans scans of the batch.  Before anything is timed the batch's angles
            are compared with the per-call ones bit for bit.
  --trace   only --reps calls with pictures for --n scans of --shape: the body of a `rocprofv3 --kernel-trace --stats`
            run, which says where the time goes kernel by kernel.
Usage: python tools/bench_hough_batch.py [--baseline-lib FILE] [--reps 5] [--md FILE] [--json FILE]
       | --trace --shape a4|half --n 64 [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from oics import _lib, hough, omr, synth
from oics._lib import OmrImage, OmrImageOwned

SHAPES = {"half": (1754, 1240), "a4": (3508, 2480)}  # rows, cols
MLL, MLG = 150.0, 50.0  # the reference's protocol: packages/core/src/main.rs:103-110


def rates(fn, scans, reps):
    fn()  # warm-up: code objects, the block cache's first allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    r = sorted(scans / t for t in ts)
    return {"scans_per_s": round(float(np.median(r)), 1), "lowest": round(r[0], 1), "highest": round(r[-1], 1)}


def bind(path):
    L = C.CDLL(path)
    for name in ("omr_get_angle_with_hough", "omr_get_angle_with_hough_ex", "omr_image_free", "omr_last_error"):
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SYMBOLS[name]
    return L


def per_call_loop(L, cards, pictures):
    """one call per scan from host memory, as a caller without the batch form works"""
    out = []
    for a in cards:
        im = OmrImage(a.ctypes.data, a.shape[0], a.shape[1], 1, a.strides[0])
        ang, owned = C.c_double(), OmrImageOwned()
        if pictures:
            rc = L.omr_get_angle_with_hough_ex(C.byref(im), MLL, MLG, C.byref(ang), C.byref(owned))
            L.omr_image_free(C.byref(owned))
        else:
            rc = L.omr_get_angle_with_hough(C.byref(im), MLL, MLG, C.byref(ang))
        assert rc == 0, (rc, L.omr_last_error())
        out.append(ang.value)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cards", type=int, default=8)
    ap.add_argument("--loop-scans", type=int, default=16)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--shapes", default="half,a4")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--shape", default="a4")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if _lib.lib().omr_device_count() < 1:
        sys.exit("bench_hough_batch needs a HIP device: a time from a CPU says nothing about the kernels")
    base = bind(args.baseline_lib) if args.baseline_lib else bind(_lib.LIB_PATH)
    base_name = "parent commit's library" if args.baseline_lib else "THIS library (no --baseline-lib)"

    made = {}

    def resident(shape, n):
        rows, cols = SHAPES[shape]
        if shape not in made:
            made[shape] = [np.ascontiguousarray(synth.make_card(rows, cols, 300 + k)[0]) for k in range(args.cards)]
        cards = made[shape]
        d = torch.from_numpy(np.stack(cards)).cuda()
        d = d[torch.arange(n, device="cuda") % len(cards)].contiguous()
        return rows, cols, cards, d

    if args.trace:
        rows, cols, cards, d = resident(args.shape, args.n)
        pics = torch.empty((args.n, rows, cols * 3), dtype=torch.uint8, device="cuda")
        for _ in range(args.reps):
            hough.hough_angles_batch_device(d.data_ptr(), args.n, rows * cols, rows, cols, 1, cols, MLL, MLG, d_lined=pics.data_ptr(),
                                            lined_stride_bytes=rows * cols * 3, lined_step=cols * 3)
        print("traced %d calls with pictures, %d scans of %d x %d each" % (args.reps, args.n, cols, rows))
        return

    out = []
    for shape in args.shapes.split(","):
        rows, cols, cards, _ = resident(shape, 1)
        loop = [cards[i % len(cards)] for i in range(args.loop_scans)]
        want = per_call_loop(base, cards, False)
        for pictures in (False, True):
            r = rates(lambda: per_call_loop(base, loop, pictures), len(loop), max(2, args.reps // 2))
            r.update(shape=shape, cols=cols, rows=rows, scans=len(loop), what="per-call loop, " + ("_ex (pictures)" if pictures else "no pictures"),
                     library=base_name)
            out.append(r)
            print(json.dumps(r), flush=True)
        for n in [int(s) for s in args.sizes.split(",")]:
            _, _, _, d = resident(shape, n)
            pics = torch.empty((n, rows, cols * 3), dtype=torch.uint8, device="cuda")
            img = rows * cols

            def batch(with_pictures):
                return hough.hough_angles_batch_device(d.data_ptr(), n, img, rows, cols, 1, cols, MLL, MLG,
                                                       d_lined=pics.data_ptr() if with_pictures else None,
                                                       lined_stride_bytes=3 * img, lined_step=3 * cols)

            ang, rc, nl = batch(True)
            assert (rc == 0).all(), rc
            got = np.asarray(ang[: len(cards)]).view(np.uint64)
            assert np.array_equal(got, np.asarray(want, np.float64).view(np.uint64)), "the batch's angles are not the per-call ones"
            cases = (("omr_edges_detection_batch_device", lambda: omr.edges_detection_batch_device(d.data_ptr(), n, img, rows, cols, 1, cols, MLL, MLG)),
                     ("omr_hough_angles_batch_device, no pictures", lambda: batch(False)),
                     ("omr_hough_angles_batch_device, pictures", lambda: batch(True)))
            for what, fn in cases:
                r = rates(fn, n, args.reps)
                r.update(shape=shape, cols=cols, rows=rows, scans=n, what=what, library="this commit",
                         segments_per_scan=round(float(np.mean(nl)), 1))
                out.append(r)
                print(json.dumps(r), flush=True)
            del d, pics
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"min_line_length": MLL, "max_line_gap": MLG, "reps": args.reps, "cases": out}, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| scan (cols x rows) | scans a call | what | library | scans/s (median) | lowest | highest |\n|---|---|---|---|---|---|---|\n")
            for r in out:
                f.write("| %d x %d | %d | %s | %s | %.1f | %.1f | %.1f |\n" % (r["cols"], r["rows"], r["scans"], r["what"], r["library"],
                                                                          r["scans_per_s"], r["lowest"], r["highest"]))


if __name__ == "__main__":
    main()
