"""The projection pictures of A4 sheets (2480 x 3508, one channel): omr_projection_pictures_device on one resident
sheet and omr_projection_pictures_batch_device on 64, both pictures and each alone.
  default   per-call times between HIP events (median of --reps calls after 5 warm-up calls; a call that draws the
            vertical picture ends in the library's own synchronise), GB/s over the compulsory bytes (rows x cols read
            plus rows x cols written per picture), then the wall time of omr_projection_pictures from host memory
            beside tests/projpic_ref.py's vectorised closed form on the same sheet.
  --trace   only --reps calls for both pictures of --n sheets: the body of a `rocprofv3 --kernel-trace --stats` run,
            which gives the time of each of the three kernels.
Usage: python tools/bench_projection_pictures.py [--reps 30] [--md FILE] [--json FILE] | --trace --n 1|64 [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

import projpic_ref as pr
from oics import _lib, synth, transfer

ROWS, COLS = 3508, 2480


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
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _lib.lib()
    if lib.omr_device_count() < 1:
        sys.exit("bench_projection_pictures needs a HIP device: a time from a CPU says nothing about the kernels")
    sheet = np.ascontiguousarray(synth.make_binary_card(ROWS, COLS, 2, skew=1.1)[0])
    img = ROWS * COLS

    def buffers(n):
        src = torch.from_numpy(sheet).cuda().reshape(1, img).repeat(n, 1).contiguous()
        return src, torch.empty_like(src), torch.empty_like(src)

    def caller(n, src, h, v, want_h, want_v):
        ph = C.c_void_p(h.data_ptr()) if want_h else None
        pv = C.c_void_p(v.data_ptr()) if want_v else None

        def call():
            if n == 1:
                rc = lib.omr_projection_pictures_device(C.c_void_p(src.data_ptr()), COLS, ROWS, COLS, ph, COLS, pv, COLS, None)
            else:
                rc = lib.omr_projection_pictures_batch_device(C.c_void_p(src.data_ptr()), n, img, COLS, ROWS, COLS, ph, img,
                                                              COLS, pv, img, COLS, None)
            assert rc == 0, lib.omr_last_error()
        return call

    if args.trace:
        src, h, v = buffers(args.n)
        call = caller(args.n, src, h, v, True, True)
        for _ in range(args.reps):
            call()
        torch.cuda.synchronize()
        assert np.array_equal(h[0].cpu().numpy().reshape(ROWS, COLS), pr.horizontal(sheet))
        assert np.array_equal(v[args.n - 1].cpu().numpy().reshape(ROWS, COLS), pr.vertical(sheet))
        print("traced %d calls, %d sheets each, both pictures" % (args.reps, args.n))
        return

    rows = []
    for n in (1, 64):
        src, h, v = buffers(n)
        for name, want_h, want_v in (("both", True, True), ("horizontal", True, False), ("vertical", False, True)):
            ms = timed(caller(n, src, h, v, want_h, want_v), args.reps)
            nbytes = 2 * img * n * (int(want_h) + int(want_v))
            r = {"sheets": n, "pictures": name, "ms_per_call": round(ms, 4), "us_per_sheet": round(ms * 1e3 / n, 2),
                 "compulsory_MB": round(nbytes / 1e6, 1), "GBps": round(nbytes / ms / 1e6, 1),
                 "share_8TBps": round(nbytes / ms / 1e6 / 8000, 4)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del src, h, v

    host = {}
    for _ in range(3):
        transfer.projection_pictures(sheet)
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        gh, gv = transfer.projection_pictures(sheet)
        t.append(time.perf_counter() - t0)
    host["omr_projection_pictures_ms"] = round(1e3 * float(np.median(t)), 3)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        eh, ev = pr.horizontal(sheet), pr.vertical(sheet)
        t.append(time.perf_counter() - t0)
    host["numpy_closed_form_ms"] = round(1e3 * float(np.median(t)), 3)
    assert np.array_equal(gh.get_mat(), eh) and np.array_equal(gv.get_mat(), ev)
    print(json.dumps(host), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": ROWS, "cols": COLS, "reps": args.reps, "cases": rows, "host": host}, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| sheets | pictures | ms / call | us / sheet | compulsory MB | GB/s | share of 8 TB/s |\n|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %d | %s | %.4f | %.2f | %.1f | %.1f | %.4f |\n" % (r["sheets"], r["pictures"], r["ms_per_call"],
                                                                            r["us_per_sheet"], r["compulsory_MB"], r["GBps"], r["share_8TBps"]))
            f.write("\n* omr_projection_pictures from host memory, both pictures: %.3f ms a call\n" % host["omr_projection_pictures_ms"])
            f.write("* tests/projpic_ref.py closed form (numpy) on the same sheet: %.3f ms\n" % host["numpy_closed_form_ms"])


if __name__ == "__main__":
    main()
