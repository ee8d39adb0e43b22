"""get_angle_with_fft on resident batches: omr_fft_angles_batch_device with and without the line pictures, beside the
per-call loop it replaces -- omr_get_angle_with_fft and omr_get_angle_with_fft_ex, one scan a call from host memory.
The per-call functions are the same code on the parent commit, so one library serves both sides.
  default   scans/s for 64 and 256 A4 scans (2480 x 3508): a host clock around calls that end in the library's own
            synchronise, one warm-up call per size, then --reps timed calls; median, and the lowest and highest rate as
            the spread.  The batch holds --cards distinct synthetic cards, repeated; the per-call loop runs over the first
            --loop-scans scans of the batch.  Before anything is timed the batch's angles are compared with the per-call
            ones bit for bit.
  --trace   only --reps calls with pictures for --n scans of --shape: the body of a `rocprofv3 --kernel-trace --stats`
            run, which says where the time goes kernel by kernel.
Usage: python tools/bench_fft_batch.py [--reps 5] [--md FILE] [--json FILE] | --trace --shape a4|half --n 64 [--reps 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from oics import _lib, fft, synth

SHAPES = {"half": (1754, 1240), "a4": (3508, 2480)}  # rows, cols
P = (50.0, 150.0, 100.0, 15.0)  # canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap


def rates(fn, scans, reps):
    fn()  # warm-up: code objects, the axis tables, the block cache's first allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    r = sorted(scans / t for t in ts)
    return {"scans_per_s": round(float(np.median(r)), 1), "lowest": round(r[0], 1), "highest": round(r[-1], 1)}


def per_call_loop(cards, pictures):
    """one call per scan from host memory, as a caller without the batch form works"""
    return [fft.get_angle_with_fft(a, *P, want_picture=True)[0] if pictures else fft.get_angle_with_fft(a, *P) for a in cards]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cards", type=int, default=8)
    ap.add_argument("--loop-scans", type=int, default=16)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--shapes", default="a4")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--shape", default="a4")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if _lib.lib().omr_device_count() < 1:
        sys.exit("bench_fft_batch needs a HIP device: a time from a CPU says nothing about the kernels")

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
            fft.fft_angles_batch_device(d.data_ptr(), args.n, rows * cols, rows, cols, cols, *P, d_lined=pics.data_ptr(),
                                        lined_stride_bytes=rows * cols * 3, lined_step=cols * 3)
        print("traced %d calls with pictures, %d scans of %d x %d each" % (args.reps, args.n, cols, rows))
        return

    out = []
    for shape in args.shapes.split(","):
        rows, cols, cards, _ = resident(shape, 1)
        loop = [cards[i % len(cards)] for i in range(args.loop_scans)]
        want = per_call_loop(cards, False)
        for pictures in (False, True):
            r = rates(lambda: per_call_loop(loop, pictures), len(loop), max(2, args.reps // 2))
            r.update(shape=shape, cols=cols, rows=rows, scans=len(loop),
                     what="per-call loop, " + ("omr_get_angle_with_fft_ex (pictures)" if pictures else "omr_get_angle_with_fft"))
            out.append(r)
            print(json.dumps(r), flush=True)
        for n in [int(s) for s in args.sizes.split(",")]:
            _, _, _, d = resident(shape, n)
            pics = torch.empty((n, rows, cols * 3), dtype=torch.uint8, device="cuda")
            img = rows * cols

            def batch(with_pictures):
                return fft.fft_angles_batch_device(d.data_ptr(), n, img, rows, cols, cols, *P,
                                                   d_lined=pics.data_ptr() if with_pictures else None,
                                                   lined_stride_bytes=3 * img, lined_step=3 * cols)

            ang, nl = batch(True)
            got = np.asarray(ang[: len(cards)]).view(np.uint64)
            assert np.array_equal(got, np.asarray(want, np.float64).view(np.uint64)), "the batch's angles are not the per-call ones"
            for what, fn in (("omr_fft_angles_batch_device, no pictures", lambda: batch(False)),
                             ("omr_fft_angles_batch_device, pictures", lambda: batch(True))):
                r = rates(fn, n, args.reps)
                r.update(shape=shape, cols=cols, rows=rows, scans=n, what=what, segments_per_scan=round(float(np.mean(nl)), 1))
                out.append(r)
                print(json.dumps(r), flush=True)
            del d, pics
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"params": P, "reps": args.reps, "cases": out}, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| scan (cols x rows) | scans a call | what | scans/s (median) | lowest | highest |\n|---|---|---|---|---|---|\n")
            for r in out:
                f.write("| %d x %d | %d | %s | %.1f | %.1f | %.1f |\n" % (r["cols"], r["rows"], r["scans"], r["what"], r["scans_per_s"],
                                                                      r["lowest"], r["highest"]))


if __name__ == "__main__":
    main()
