"""correct_default for batches (development aid): sheets/s of omr_correct_batch_run_device, omr_correct_default_batch and
the per-call omr_correct_default, on two shapes:
  dataset  1150 x 1240 BGR, the dataset pin's inputs (tests/dataset_pin.py: skew injection + JPEG q100), 32 cases -- 31
           Believed and 1 that falls back to Hough -- repeated to fill a batch
  a4       1754 x 1240 BGR synth.make_color_card sheets (fractional shrink, scale 0.1311), 32 of them repeated
Legs (one JSON line each; every leg can run in a process of its own with --leg, so each GPU step gets its own time limit):
  percall_t{1,4,16}[_noimg]  omr_correct_default from T host threads, with / without the rotated image
  batch_n{256,1024,4096}     omr_correct_batch_run_device, inputs and canvases resident in HBM
  host                       omr_correct_default_batch from host memory (256 sheets, rotated images returned)
Usage: python tools/bench_correct.py [--shape dataset|a4] [--leg NAME] [--steps K] [--warmup W]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "omr-img-corrector_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from oics import omr, synth

PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)
LEGS = ("percall_t1", "percall_t4", "percall_t16", "percall_t1_noimg", "percall_t4_noimg", "percall_t16_noimg",
        "batch_n256", "batch_n1024", "batch_n4096", "host")


def sheets(shape):
    if shape == "a4":
        return [synth.make_color_card(1754, 1240, 900 + i, skew=float((i * 37) % 200 - 100) / 10)[0] for i in range(32)]
    import dataset_pin as dp
    from oracle import oracle as orc
    orc.build()
    exp = dp.load_expected()["cases"]
    # the sheets of the dataset's 1150 x 1240 shape; 31 Believed cases and one that falls back to Hough
    shape_of = {s: dp.imread_color(s).shape[:2] for s in sorted({c["sheet"] for c in exp})}
    cases = [c for c in exp if shape_of[c["sheet"]] == (1150, 1240)]
    pick = [c for c in cases if c["proj_status"] == 0][::7][:31] + [c for c in cases if c["proj_status"] != 0][:1]
    return [dp.inject(dp.imread_color(c["sheet"]), c["idx"] * 0.1, orc) for c in pick]


def percall(src, threads, want_image, steps, warmup):
    calls = 64 * threads

    def one(i):
        omr.correct_default(src[i % len(src)], *PARAMS, want_image=want_image)

    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, range(warmup * threads)))
        t0 = time.perf_counter()
        for _ in range(steps):
            list(ex.map(one, range(calls)))
        dt = time.perf_counter() - t0
    return steps * calls / dt


def batch(src, n, steps, warmup):
    rows, cols = src[0].shape[:2]
    cb = omr.CorrectBatch(rows, cols, 3, *PARAMS, max_scans=n)
    R, Cc = cb.canvas
    uniq = torch.from_numpy(np.stack(src)).to("cuda:0")
    d_in = uniq.repeat((n + len(src) - 1) // len(src), 1, 1, 1)[:n].contiguous()
    out_step, out_stride = Cc * 3, Cc * 3 * R
    d_out = torch.empty((n, out_stride), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    stride, step = rows * cols * 3, cols * 3

    def run():
        return cb.run_device(d_in.data_ptr(), stride, step, n, d_out.data_ptr(), out_stride, out_step)

    for _ in range(warmup):
        run()
    t0 = time.perf_counter()
    for _ in range(steps):
        ang, chk, rc, _ = run()
    dt = time.perf_counter() - t0
    cb.close()
    return steps * n / dt, int((rc != 0).sum())


def host(src, steps, warmup, n=256):
    lst = [src[i % len(src)] for i in range(n)]
    for _ in range(warmup):
        omr.correct_default_batch(lst, *PARAMS)
    t0 = time.perf_counter()
    for _ in range(steps):
        omr.correct_default_batch(lst, *PARAMS)
    return steps * n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("dataset", "a4"), default="dataset")
    ap.add_argument("--leg", choices=LEGS + ("all",), default="all")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    src = sheets(a.shape)
    for leg in LEGS if a.leg == "all" else (a.leg,):
        rec = {"shape": a.shape, "leg": leg, "rows": int(src[0].shape[0]), "cols": int(src[0].shape[1])}
        if leg.startswith("percall"):
            t = int(leg.split("_")[1][1:])
            rec["sheets_per_s"] = round(percall(src, t, not leg.endswith("noimg"), a.steps, a.warmup), 1)
        elif leg.startswith("batch"):
            n = int(leg[len("batch_n"):])
            rate, failed = batch(src, n, a.steps, a.warmup)
            rec.update(n=n, sheets_per_s=round(rate, 1), failed_sheets=failed)
        else:
            rec["sheets_per_s"] = round(host(src, a.steps, a.warmup), 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
