"""Usage: python tools/bench_projection_batch.py [all|device|host|profile] [n]
512 device-resident A4 BGR scans at (45, 0.2, 0.2): the parent's best (loop of omr_resize_area_device + one
omr_batch_run_device_cn) against omr_projection_batch_run_device; host images: 16-thread per-call loop against the host form."""
import ctypes as C, os, sys, time, json
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
from oics import _lib, projection

L = _lib.lib()
MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 512
rows, cols, cn = 3508, 2480, 3
rng = np.random.Generator(np.random.PCG64(5))
yy, xx = np.mgrid[:rows, :cols]
g = np.where(((xx % 61) < 6) | ((yy % 83) < 7), 40, 230).astype(np.uint8)
base = np.ascontiguousarray(np.stack([g, g, g], 2))
base[::7, ::5, 1] //= 2
res = {"n": N}

def dev_batch(n):
    b = torch.from_numpy(base).cuda()
    out = torch.empty((n, rows, cols, cn), dtype=torch.uint8, device="cuda")
    for i in range(n):
        out[i] = torch.roll(b, (i * 3) % 97, 0)
    torch.cuda.synchronize()
    return out

if MODE in ("all", "device", "profile"):
    d = dev_batch(N)
    step, stride = cols * cn, rows * cols * cn
    pb = projection.ProjectionBatch(rows, cols, cn, 45, 0.2, 0.2, N)
    wr, wc = pb.wrows, pb.wcols
    reps = 1 if MODE == "profile" else 3
    ang = None
    ts = []
    for r in range(reps + (0 if MODE == "profile" else 1)):
        t0 = time.perf_counter()
        ang, idx, _, _ = pb.run_device(d.data_ptr(), stride, step, N)
        ts.append(time.perf_counter() - t0)
    res["batch_run_device_s"] = ts
    res["batch_scans_per_s"] = N / min(ts)
    # front end alone, wall clock
    small = torch.empty((N, wr, wc * cn), dtype=torch.uint8, device="cuda")
    if MODE != "profile":
        t0 = time.perf_counter()
        pb.front_device(d.data_ptr(), stride, step, N, small.data_ptr(), wr * wc * cn, wc * cn)
        res["front_device_wall_s_incl_copies"] = time.perf_counter() - t0
    pb.close()
    if MODE != "profile":
        # the parent's best: per-image omr_resize_area_device into a packed buffer, then one colour batch sweep
        b = projection.Batch(wr, wc, 45, 0.2)
        b.set_group(64)
        A = 2 * projection.candidate_count(45, 0.2)[0]
        d_best = torch.zeros(N, dtype=torch.int32, device="cuda")
        wstep = wc * cn
        tb = []
        for r in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(N):
                rc = L.omr_resize_area_device(d.data_ptr() + i * stride, step, rows, cols, cn, small.data_ptr() + i * wr * wstep, wstep, wr, wc, None)
                assert rc == 0
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            b.run_device_cn(small.data_ptr(), wr * wstep, wstep, cn, N, 127, d_best.data_ptr())
            b.sync()
            best = d_best.cpu().numpy()
            tb.append((time.perf_counter() - t0, t1 - t0))
        b.close()
        res["parent_loop_s(total,resize)"] = tb
        res["parent_scans_per_s"] = N / min(t[0] for t in tb)
        res["same_answers"] = bool((best == idx).all())
    del d

if MODE in ("all", "host"):
    M = min(N, 256)
    uniq = [np.ascontiguousarray(np.roll(base, (i * 3) % 97, 0)) for i in range(32)]
    imgs = [uniq[i % 32] for i in range(M)]
    def one(a):
        return projection.get_angle_with_projections(a, 45, 0.2, 0.2, 1)
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, imgs[:32]))  # warm
        t0 = time.perf_counter()
        ref = list(ex.map(one, imgs))
        t_loop = time.perf_counter() - t0
    projection.get_angles_with_projections(imgs[:32], 45, 0.2, 0.2)  # warm: context
    t0 = time.perf_counter()
    got = projection.get_angles_with_projections(imgs, 45, 0.2, 0.2)
    t_batch = time.perf_counter() - t0
    res["host_m"] = M
    res["host_threaded_per_call_scans_per_s"] = M / t_loop
    res["host_form_scans_per_s"] = M / t_batch
    res["host_same_answers"] = bool((np.asarray(ref).view(np.uint64) == got.view(np.uint64)).all())

print(json.dumps(res))


