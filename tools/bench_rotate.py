"""rotate_mat with every interpolation on the device (omr_rotate_device_ex) on an A4 sheet (2480 x 3508, angle 3.3,
CONTAIN; 1 and 3 channels unless --channels says otherwise), BORDER_CONSTANT and BORDER_REPLICATE, with omr_rotate_device
(NEAREST / LINEAR, CONSTANT) on the same geometry as the anchor.  Device-resident buffers, HIP events around `--iters`
calls after a warm-up.  Per case: ms per call, GB/s of the compulsory bytes (source read once + canvas written once),
their share of 8 TB/s, and tap multiply-adds per second (canvas pixels x channels x K^2).
Usage: python tools/bench_rotate.py [--iters N] [--channels 1,3] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "omr-img-corrector_amd")]
import torch  # noqa: E402  (first: the library then shares torch's HIP runtime)

from oics import _lib  # noqa: E402

NAMES = {0: "NEAREST", 1: "LINEAR", 2: "CUBIC", 4: "LANCZOS4"}
TAPS = {0: 1, 1: 4, 2: 16, 4: 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--channels", default="1,3", help="comma-separated channel counts, each 1..4")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = _lib.lib()
    rows, cols, angle, clip = 3508, 2480, 3.3, 1
    dr, dc = C.c_int32(), C.c_int32()
    assert lib.omr_rotate_size(rows, cols, angle, clip, C.byref(dr), C.byref(dc)) == 0
    dr, dc = dr.value, dc.value
    b = (C.c_uint8 * 4)(255, 255, 255, 0)
    bp = C.cast(b, _lib.u8p)
    g = torch.Generator().manual_seed(1)
    out = []
    for cn in [int(c) for c in args.channels.split(",")]:
        src = torch.randint(0, 256, (rows, cols * cn), dtype=torch.uint8, generator=g).cuda()
        dst = torch.empty((dr, dc * cn), dtype=torch.uint8, device="cuda")
        cases = [("omr_rotate_device", i, 0) for i in (0, 1)]
        cases += [("omr_rotate_device_ex", i, m) for i in (0, 1, 2, 4) for m in (0, 1)]
        for fn, interp, mode in cases:
            def call():
                if fn == "omr_rotate_device":
                    rc = lib.omr_rotate_device(C.c_void_p(src.data_ptr()), cols * cn, rows, cols, cn, angle, 1.0, interp,
                                               bp, clip, C.c_void_p(dst.data_ptr()), dc * cn, dr, dc, None)
                else:
                    rc = lib.omr_rotate_device_ex(C.c_void_p(src.data_ptr()), cols * cn, rows, cols, cn, angle, 1.0,
                                                  interp, mode, bp, clip, C.c_void_p(dst.data_ptr()), dc * cn, dr, dc,
                                                  None)
                assert rc == 0, lib.omr_last_error()
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            nbytes = rows * cols * cn + dr * dc * cn
            r = {"fn": fn, "cn": cn, "interp": NAMES[interp], "border": ("CONSTANT", "REPLICATE")[mode], "ms": round(ms, 4),
                 "GBps": round(nbytes / ms / 1e6, 1), "share_8TBps": round(nbytes / ms / 1e6 / 8000, 4),
                 "Gmac_per_s": round(dr * dc * cn * TAPS[interp] / ms / 1e6, 1)}
            out.append(r)
            print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": rows, "cols": cols, "angle": angle, "canvas": [dr, dc], "cases": out}, f, indent=1)


if __name__ == "__main__":
    main()
