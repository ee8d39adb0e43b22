"""rotate_mat for a batch with an angle per image (omr_rotate_batch_device_ex) against a loop of omr_rotate_device_ex
calls doing the same work: A4 sheets (2480 x 3508), CONTAIN, white, angles uniform in +-10 degrees (fixed seed), NEAREST
and LINEAR, 1 channel (n up to 512) and 3 channels (n up to 64), every image into its slot of one block.  Times are HIP
events around the whole call or loop on the null stream (so the loop's launch gaps and the batch's table upload
count), after 2 warm-up runs, 9 repetitions: median, min and max in microseconds per image.
--lib PATH times the loop through another build of the library (the batch rows are skipped when it has no batch entry
point), so the per-call numbers of an older commit can be taken on the same GPU.
Usage: python tools/bench_rotate_batch.py [--lib PATH] [--quick]; one JSON line per case."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omr-img-corrector_amd"))
import numpy as np
import torch

from oics import _lib, synth

ROWS, COLS = 3508, 2480
WARM, REPS = 2, 9


def load(path):
    if not path:
        return _lib.lib(), True
    L = C.CDLL(path)
    have = hasattr(L, "omr_rotate_batch_device_ex")
    for name in ("omr_rotate_size", "omr_rotate_device_ex") + (("omr_rotate_batch_canvas", "omr_rotate_batch_device_ex") if have else ()):
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SYMBOLS[name]
    return L, have


def timed(fn):
    ts = []
    for k in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= WARM:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return ts


def main():
    args = sys.argv[1:]
    path = args[args.index("--lib") + 1] if "--lib" in args else None
    quick = "--quick" in args
    L, have_batch = load(path)
    white = (C.c_uint8 * 4)(255, 255, 255, 0)
    wp = C.cast(white, _lib.u8p)
    cards = [synth.make_card(ROWS, COLS, 3 + i)[0] for i in range(4)]
    for cn, ns in ((1, (1, 2, 8, 64, 512)), (3, (1, 2, 8, 64))):
        nmax = ns[-1] if not quick else 8
        base = np.stack([cards[i % 4] for i in range(8)])
        if cn == 3:
            base = np.repeat(base[..., None], 3, axis=3)
        d_src = torch.from_numpy(base).cuda().repeat((nmax // 8,) + (1,) * (base.ndim - 1)) if nmax >= 8 else torch.from_numpy(base).cuda()
        angles_all = np.random.Generator(np.random.PCG64(10)).uniform(-10.0, 10.0, 512)
        sstep, sstride = COLS * cn, ROWS * COLS * cn
        for n in [v for v in ns if v <= nmax]:
            angles = np.ascontiguousarray(angles_all[:n])
            sizes = []
            for a in angles:
                dr, dc = C.c_int32(), C.c_int32()
                assert L.omr_rotate_size(ROWS, COLS, float(a), 1, C.byref(dr), C.byref(dc)) == 0
                sizes.append((dr.value, dc.value))
            mr, mc = max(s[0] for s in sizes), max(s[1] for s in sizes)
            dstep = (mc * cn + 3) & ~3
            dstride = mr * dstep
            d_dst = torch.empty(n * dstride, dtype=torch.uint8, device="cuda")
            for interp in (0, 1):
                def loop():
                    for i in range(n):
                        rc = L.omr_rotate_device_ex(C.c_void_p(d_src.data_ptr() + i * sstride), sstep, ROWS, COLS, cn, float(angles[i]),
                                                    1.0, interp, 0, wp, 1, C.c_void_p(d_dst.data_ptr() + i * dstride), dstep,
                                                    sizes[i][0], sizes[i][1], None)
                        assert rc == 0

                def batch():
                    rc = L.omr_rotate_batch_device_ex(C.c_void_p(d_src.data_ptr()), n, sstride, sstep, ROWS, COLS, cn,
                                                      angles.ctypes.data_as(_lib.f64p), 1.0, interp, 0, wp, 1,
                                                      C.c_void_p(d_dst.data_ptr()), dstride, dstep, mr, mc, None, None)
                    assert rc == 0
                for name, fn in (("loop", loop),) + ((("batch", batch),) if have_batch else ()):
                    ts = np.array(timed(fn)) / n
                    print(json.dumps({"lib": path or "this", "form": name, "channels": cn, "n": n, "interp": ("NEAREST", "LINEAR")[interp],
                                      "us_per_image_median": round(float(np.median(ts)), 2), "min": round(float(ts.min()), 2),
                                      "max": round(float(ts.max()), 2)}), flush=True)
            del d_dst
        del d_src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
