"""Colour (BGR) batches at A4 (development aid): 512 colour scans of 2480 x 3508 resident in HBM, +-10 deg @ 0.05 deg, one
set_lanes(512) launch per step, bench.py's warm-up and step counts.  Prints images/s, one JSON line per leg:
  gray        the gray sweep (omr_batch_run_device on 512 gray scans), the reference point
  color       the colour sweep (omr_batch_run_device_cn, channels = 3)
  deskew_nn   colour deskew, NEAREST (omr_batch_deskew_device_cn)
  deskew_lin  colour deskew, LINEAR
  workaround  what a caller had to do before: omr_rgb_to_gray_device per scan, the gray batch, the winners copied to the
              host, omr_rotate_device(channels = 3) per scan (LINEAR)
  warp        the colour warp alone: 8 A4 scans per launch, the context synchronised after each call (read the kernel's
              duration from `rocprofv3 --kernel-trace --stats`)
Every leg can run in a process of its own (--leg NAME), so that each GPU step gets a time limit of its own.
Usage: python tools/bench_color.py [--leg NAME] [--steps K] [--warmup W] [--scans S]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "omr-img-corrector_amd"))
import numpy as np
import torch

import oics
from oics import projection, synth
from oics._lib import check

ROWS, COLS = 3508, 2480
LEGS = ("gray", "color", "deskew_nn", "deskew_lin", "workaround", "warp")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS + ("all",), default="all")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scans", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20, help="warp leg: launches of 8 scans")
    args = ap.parse_args()
    legs = LEGS if args.leg == "all" else (args.leg,)
    dev = torch.device("cuda:0")
    base = [synth.make_color_card(ROWS, COLS, 3 + i)[0] for i in range(8)]
    n = args.scans if legs != ("warp",) else 8
    d8 = torch.from_numpy(np.stack(base)).to(dev)
    scans = d8[[i % 8 for i in range(n)]].contiguous()
    del d8
    S, P = ROWS * COLS * 3, COLS * 3
    b = projection.Batch(ROWS, COLS, 10, 0.05, device=0, n_streams=2)
    A, N, step = b.A, b.N, b.step
    best = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    L = oics.lib()

    def report(leg, elapsed, steps, imgs, **extra):
        rec = {"leg": leg, "scans": imgs, "steps": steps, "ms_per_step": elapsed / steps * 1e3,
               "images_per_s": imgs * steps / elapsed}
        rec.update(extra)
        print(json.dumps(rec), flush=True)

    if "warp" in legs:
        b.set_group(8)
        dr, dc = b.deskew_canvas()
        out = torch.empty((8, dr, dc * 3), dtype=torch.uint8, device=dev)
        for name, interp in (("nearest", 0), ("linear", 1)):
            def one():
                b.deskew_device_cn(scans.data_ptr(), S, P, 3, 8, 127, interp, (255, 255, 255), out.data_ptr(), dr * dc * 3,
                                   dc * 3, None, best.data_ptr())
                b.sync()
            el = timed(one, args.reps, 2)
            report("warp_" + name, el, args.reps, 8, canvas=[dr, dc],
                   moved_bytes_per_launch=8 * (ROWS * COLS * 3 + dr * dc * 3))
        legs = tuple(x for x in legs if x != "warp")
        if not legs:
            return
    b.set_lanes(n)
    if "gray" in legs:
        g = torch.empty((n, ROWS, COLS), dtype=torch.uint8, device=dev)
        for i in range(n):
            check(L.omr_rgb_to_gray_device(scans[i].data_ptr(), P, ROWS, COLS, 3, g[i].data_ptr(), COLS, None))
        torch.cuda.synchronize()

        def one():
            b.run_device(g.data_ptr(), ROWS * COLS, COLS, n, 127, best.data_ptr())
        el = timed(lambda: (one(), b.sync()), args.steps, args.warmup)
        report("gray", el, args.steps, n)
        gbest = best.cpu().numpy().copy()
        del g
    if "color" in legs:
        el = timed(lambda: (b.run_device_cn(scans.data_ptr(), S, P, 3, n, 127, best.data_ptr()), b.sync()), args.steps, args.warmup)
        report("color", el, args.steps, n)
        if "gray" in legs:
            assert (best.cpu().numpy() == gbest).all(), "colour winners differ from the gray path's"
    dr, dc = b.deskew_canvas()
    if "deskew_nn" in legs or "deskew_lin" in legs or "workaround" in legs:
        out = torch.empty((n, dr, dc * 3), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
    for leg, interp in (("deskew_nn", 0), ("deskew_lin", 1)):
        if leg not in legs:
            continue

        def one():
            b.deskew_device_cn(scans.data_ptr(), S, P, 3, n, 127, interp, (255, 255, 255), out.data_ptr(), dr * dc * 3, dc * 3,
                               None, best.data_ptr())
            b.sync()
        el = timed(one, args.steps, args.warmup)
        report(leg, el, args.steps, n)
    if "workaround" in legs:
        g = torch.empty((n, ROWS, COLS), dtype=torch.uint8, device=dev)
        border = (C.c_uint8 * 4)(255, 255, 255, 0)
        sizes = {}

        def one():
            for i in range(n):
                check(L.omr_rgb_to_gray_device(scans[i].data_ptr(), P, ROWS, COLS, 3, g[i].data_ptr(), COLS, None))
            torch.cuda.synchronize()  # (the batch's streams do not wait for the null stream)
            b.run_device(g.data_ptr(), ROWS * COLS, COLS, n, 127, best.data_ptr())
            b.sync()
            h = best.cpu().numpy()
            for i in range(n):
                angle = (int(h[i]) - N) * step
                if angle not in sizes:
                    r, c = C.c_int32(), C.c_int32()
                    check(L.omr_rotate_size(ROWS, COLS, angle, 1, C.byref(r), C.byref(c)))
                    sizes[angle] = (r.value, c.value)
                r, c = sizes[angle]
                check(L.omr_rotate_device(scans[i].data_ptr(), P, ROWS, COLS, 3, angle, 1.0, 1, border, 1,
                                               out[i].data_ptr(), dc * 3, r, c, None))
        el = timed(one, args.steps, args.warmup)
        report("workaround", el, args.steps, n)
    b.close()


if __name__ == "__main__":
    main()
