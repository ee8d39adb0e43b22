"""Usage: python tools/bench_projection_deskew.py [all|device|percall] [n]
       python tools/bench_projection_deskew.py warp <degrees> [n] [library]
The reference benchmark's flow (core/src/main.rs:68-95: get_angle_with_projections(45, 0.2, 0.2), then rotate_mat LINEAR,
white border, CONTAIN of the full-size original) on n (256) device-resident A4 colour scans:
  device    omr_projection_batch_deskew_device against the two-call form it replaces: omr_projection_batch_run_device,
            then omr_rotate_batch_device_ex by the returned angles (its matrix upload included)
  percall   omr_get_angle_with_projections + omr_rotate on host images from 16 threads
  warp      for a kernel trace: n (8) scans turned by <degrees>, the new call five times with NEAREST and five times
            with LINEAR; the time of deskew_warp3_kernel is read from the profiler's kernel statistics.  [library]: another
            build of libomrdeskew.so to load instead of the package's (an A/B of two builds)
Prints one JSON line."""
import ctypes as C, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
from oics import _lib, projection, transfer
from oics.types import RotateClipStrategy

MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
if MODE == "warp" and len(sys.argv) > 4:
    _lib.LIB_PATH = os.path.abspath(sys.argv[4])
L = _lib.lib()
rows, cols, cn = 3508, 2480, 3
MAX_ANGLE, STEP, SCALE, LINEAR, NEAREST = 45, 0.2, 0.2, 1, 0
WHITE = (255, 255, 255)
REPS = 20 if MODE != "warp" else 5


def ruled_sheet(angle):
    """an A4 sheet of dark rules and boxes on white, turned by `angle` degrees about the centre"""
    yy, xx = np.mgrid[:rows, :cols].astype(np.float32)
    t = np.deg2rad(angle)
    x, y = xx - cols / 2.0, yy - rows / 2.0
    u = x * np.cos(t) + y * np.sin(t)
    v = -x * np.sin(t) + y * np.cos(t)
    dark = (np.mod(v, 160.0) < 50.0) & (np.abs(u) < 0.42 * cols) & (np.abs(v) < 0.42 * rows)
    for bu, bv in ((-0.3, -0.25), (0.1, 0.05), (0.28, 0.3)):
        d = np.maximum(np.abs(u - bu * cols), np.abs(v - bv * rows))
        dark |= (d < 150.0) & (d >= 110.0)
    a = np.full((rows, cols, 3), 255, np.uint8)
    a[dark] = (25, 60, 40)
    return a


def spread(ts, n):
    return {"scans_per_s_best": n / min(ts), "scans_per_s_median": n / statistics.median(ts), "scans_per_s_worst": n / max(ts),
            "seconds": [round(t, 4) for t in ts]}


def resident(angles, n):
    uniq = [torch.from_numpy(ruled_sheet(a)).cuda() for a in angles]
    d = torch.empty((n, rows, cols, cn), dtype=torch.uint8, device="cuda")
    for i in range(n):
        d[i] = uniq[i % len(uniq)]
    torch.cuda.synchronize()
    return d


res = {"mode": MODE}
step_b, stride_b = cols * cn, rows * cols * cn

if MODE == "warp":
    deg = float(sys.argv[2])
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    d = resident([deg, -deg, deg + 1.3, -deg - 0.7], n)
    pb = projection.ProjectionBatch(rows, cols, cn, MAX_ANGLE, STEP, SCALE, n)
    DR, DC = pb.deskew_canvas()
    out = torch.empty((n, DR, DC * cn), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for interp in (NEAREST, LINEAR):
        for r in range(REPS):
            ang, _, _ = pb.deskew_device(d.data_ptr(), stride_b, step_b, n, interp, WHITE, out.data_ptr(), DR * DC * cn, DC * cn)
    pb.close()
    res.update(n=n, turned_by=deg, winners=[float(a) for a in ang])

if MODE in ("all", "device"):
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    d = resident([-7.0, 0.0, 4.5, 2.2, -1.4, 9.0, -3.3, 0.6], n)
    pb = projection.ProjectionBatch(rows, cols, cn, MAX_ANGLE, STEP, SCALE, n)
    DR, DC = pb.deskew_canvas()
    ostep, ostride = DC * cn, DR * DC * cn
    out = torch.empty((n, DR, DC * cn), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bw = (C.c_uint8 * 4)(*WHITE, 0)
    size2 = np.zeros(2 * n, np.int32)

    def new_call():
        return pb.deskew_device(d.data_ptr(), stride_b, step_b, n, LINEAR, WHITE, out.data_ptr(), ostride, ostep)

    def two_calls():
        ang, idx, _, _ = pb.run_device(d.data_ptr(), stride_b, step_b, n)
        rc = L.omr_rotate_batch_device_ex(d.data_ptr(), n, stride_b, step_b, rows, cols, cn, ang.ctypes.data_as(_lib.f64p), 1.0, LINEAR, 0,
                                          bw, 1, out.data_ptr(), ostride, ostep, DR, DC, size2.ctypes.data_as(_lib.i32p), None)
        assert rc == 0, L.omr_last_error()
        return ang, idx, size2.reshape(n, 2).copy()

    t_new, t_two = [], []
    new_call(), two_calls()  # warm: tables, tile records
    for r in range(REPS):  # alternating, so that both see the same clocks
        t0 = time.perf_counter(); a1, i1, s1 = new_call(); t_new.append(time.perf_counter() - t0)
        probe = out[:, ::97, ::89].clone()
        t0 = time.perf_counter(); a2, i2, s2 = two_calls(); t_two.append(time.perf_counter() - t0)
    same = bool((a1.view(np.uint64) == a2.view(np.uint64)).all() and (s1 == s2).all() and torch.equal(probe, out[:, ::97, ::89]))
    pb.close()
    res.update(n=n, new_call=spread(t_new, n), two_calls=spread(t_two, n), same_answers=same,
               winners=sorted(set(float(a) for a in a1)))
    del d, out

if MODE in ("all", "percall"):
    M = 64
    uniq = [ruled_sheet(a) for a in (-7.0, 0.0, 4.5, 2.2)]
    imgs = [uniq[i % 4] for i in range(M)]

    def one(a):
        ang = projection.get_angle_with_projections(a, MAX_ANGLE, STEP, SCALE, 1)
        return ang, transfer.rotate_mat(a, ang, 1.0, LINEAR, 0, WHITE + (0,), RotateClipStrategy.CONTAIN).get_mat().shape

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, imgs[:16]))  # warm
        ts = []
        for r in range(3):
            t0 = time.perf_counter(); list(ex.map(one, imgs)); ts.append(time.perf_counter() - t0)
    res["per_call_16_threads_host_images"] = dict(spread(ts, M), m=M)
    projection.get_angles_and_deskew(imgs[:8], MAX_ANGLE, STEP, SCALE)  # warm: context
    ts = []
    for r in range(3):
        t0 = time.perf_counter(); projection.get_angles_and_deskew(imgs, MAX_ANGLE, STEP, SCALE); ts.append(time.perf_counter() - t0)
    res["host_form"] = dict(spread(ts, M), m=M)

print(json.dumps(res))
