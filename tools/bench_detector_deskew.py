"""The Hough and FFT legs of the reference's benchmark as batch flows (development aid), with the reference's arguments
(core/src/main.rs:96-170: Hough 125 / 15; FFT 125 / 150 / 150 / 75; rotate_mat LINEAR, white border, CONTAIN; JPEG quality
100), each against the baseline it replaces, built from the entry points the library had before these flows:
  gray     omr_rgb_to_gray_batch_device on resident A4 colour scans: time (HIP events), bytes moved and the fraction of the
           8 TB/s roofline, beside the loop of omr_rgb_to_gray_device calls it replaces;
  device   omr_hough_deskew_batch_device / omr_fft_deskew_batch_device on resident A4 colour scans + the batch JPEG encoder,
           against the per-call gray loop + the batch detector + omr_rotate_batch_device_ex + the same encoder;
  files    omr_deskew_with_hough_batch_streams / omr_deskew_with_fft_batch_streams on the dataset's sheets, against Pillow's
           decode + the per-call pair (omr_rgb_to_gray, detector, omr_rotate_ex) + Pillow's save on 16 threads.
A warm-up of every leg, then alternating passes; medians and the spread.  Wall clocks on the host except the gray kernel.
Usage: python tools/bench_detector_deskew.py [--resident N] [--n N] [--runs R] [--skip hough|fft] [--commit TEXT] [--out FILE]
Writes a markdown report (default profiles/r23_detector_deskew.md) and prints it."""
import argparse
import ctypes as C
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HOUGH = (125.0, 15.0)
FFT = (125.0, 150.0, 150.0, 75.0)
LINEAR, CONTAIN, QUALITY, WHITE = 1, 1, 100, (255, 255, 255, 0)
ROWS, COLS = 3508, 2480
ROOFLINE = 8e12


def fmt(v, unit=""):
    return "%.1f%s (%.1f .. %.1f)" % (float(np.median(v)), unit, min(v), max(v))


def resident_cards(n):
    import torch
    from oics import synth
    cards = [synth.make_color_card(ROWS, COLS, 40 + i, skew=float(2 * i - 7))[0] for i in range(8)]
    stride = (ROWS * COLS * 3 + 255) & ~255
    d = torch.empty(n * stride, dtype=torch.uint8, device="cuda:0")
    for i in range(n):
        d[i * stride: i * stride + ROWS * COLS * 3] = torch.from_numpy(cards[i % 8].reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    return d, stride


def gray_section(d, stride, n, runs):
    import torch
    from oics import _lib, transfer
    L = _lib.lib()
    img = ROWS * COLS
    g = torch.empty(n * img, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream

    def batch():
        transfer.rgb_to_gray_batch(d.data_ptr(), n, stride, COLS * 3, ROWS, COLS, 3, g.data_ptr(), img, COLS, stream=s)

    def loop():
        for i in range(n):
            L.omr_rgb_to_gray_device(C.c_void_p(d.data_ptr() + i * stride), COLS * 3, ROWS, COLS, 3, C.c_void_p(g.data_ptr() + i * img), COLS,
                                     C.c_void_p(s))

    ms = {"batch": [], "loop": []}
    for k in range(runs + 1):
        for name, fn in (("batch", batch), ("loop", loop)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k:
                ms[name].append(e0.elapsed_time(e1))
    moved = n * img * 4.0
    b, lp = float(np.median(ms["batch"])), float(np.median(ms["loop"]))
    return ["## The gray kernel alone", "",
            "%d resident A4 colour scans (%d x %d x 3, packed rows), HIP events on the stream, median (min .. max) of %d passes "
            "after a warm-up.  Bytes moved: 3 read + 1 written per pixel, %.2f GB." % (n, COLS, ROWS, runs, moved / 1e9), "",
            "| leg | ms | GB/s | of the 8 TB/s roofline |", "|---|---|---|---|",
            "| omr_rgb_to_gray_batch_device, one launch | %s | %.0f | %.2f |" % (fmt(ms["batch"]), moved / b / 1e6, moved / b / 1e6 / (ROOFLINE / 1e9)),
            "| %d omr_rgb_to_gray_device calls (host time to enqueue included) | %s | %.0f | %.2f |" % (n, fmt(ms["loop"]), moved / lp / 1e6, moved / lp / 1e6 / (ROOFLINE / 1e9)),
            ""]


def device_section(which, d, stride, n, runs):
    import torch
    from oics import _lib, fft, hough, jpeg, transfer
    L = _lib.lib()
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    mr, mc = transfer.detector_deskew_canvas(ROWS, COLS, CONTAIN)
    ostep = mc * 3
    ostride = ostep * mr
    bound = (jpeg.bound(mr, mc, 3) + 255) & ~255
    out = torch.empty(n * ostride, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(n * bound, dtype=torch.uint8, device="cuda:0")
    img = ROWS * COLS
    g = torch.empty(n * img, dtype=torch.uint8, device="cuda:0")

    def encode(sizes):
        return jpeg.encode_batch_device(out.data_ptr(), ostride, ostep, mr, mc, 3, sizes, n, QUALITY, dst.data_ptr(), bound)

    def new():
        ang, rc, nl, sizes = mod.deskew_device(d.data_ptr(), n, stride, ROWS, COLS, 3, COLS * 3, *args, LINEAR, 0, WHITE, CONTAIN, out.data_ptr(),
                                               ostride, ostep)
        return ang, rc, encode(sizes)

    def old():
        for i in range(n):
            L.omr_rgb_to_gray_device(C.c_void_p(d.data_ptr() + i * stride), COLS * 3, ROWS, COLS, 3, C.c_void_p(g.data_ptr() + i * img), COLS, None)
        if which == "hough":
            ang, rc, nl = hough.hough_angles_batch_device(g.data_ptr(), n, img, ROWS, COLS, 1, COLS, *args)
        else:
            ang, nl = fft.fft_angles_batch_device(g.data_ptr(), n, img, ROWS, COLS, COLS, *args)
            rc = np.zeros(n, np.int32)
        assert (rc == 0).all(), "the baseline rotates every scan: a card without a segment is not part of this workload"
        sizes = transfer.rotate_batch_device_ex(d.data_ptr(), n, stride, COLS * 3, ROWS, COLS, 3, ang, 1.0, LINEAR, 0, WHITE, CONTAIN, out.data_ptr(),
                                                ostride, ostep, mr, mc)
        return ang, rc, encode(sizes)

    a_new, rc_new, len_new = new()
    a_old, rc_old, len_old = old()
    assert (np.asarray(a_new).view(np.uint64) == np.asarray(a_old).view(np.uint64)).all() and (np.asarray(len_new) == np.asarray(len_old)).all()
    rate = {"new": [], "old": []}
    for _ in range(runs):
        for name, fn in (("new", new), ("old", old)):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rate[name].append(n / (time.perf_counter() - t))
    r = float(np.median(rate["new"])) / float(np.median(rate["old"]))
    return "| %s, device-resident, %d A4 colour scans a call | %s | %s | %s%.2f x%s |" % (
        which, n, fmt(rate["new"]), fmt(rate["old"]), "**" if r < 1 else "", r, "**" if r < 1 else "")


def pillow_decode(stream):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))[..., ::-1])


def pillow_jpeg(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img[..., ::-1] if img.ndim == 3 else img).save(b, format="JPEG", quality=QUALITY)
    return b.getvalue()


def files_section(which, streams, runs):
    from oics import _lib, fft, hough, transfer
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    n = len(streams)

    def new():
        return mod.deskew_streams(streams, *args, flags=LINEAR, border_value=WHITE, clip_strategy=CONTAIN, level=QUALITY)

    def one(s):
        img = pillow_decode(s)
        gray = transfer.transfer_rgb_image_to_gray_image(img).matrix
        try:
            ang = hough.get_angle_with_hough(gray, *args) if which == "hough" else fft.get_angle_with_fft(gray, *args)
        except _lib.OmrError:
            return None, None
        return ang, pillow_jpeg(transfer.rotate_mat(img, ang, 1.0, LINEAR, 0, WHITE, CONTAIN).get_mat())

    def old():
        with ThreadPoolExecutor(16) as ex:
            return list(ex.map(one, streams))

    ang, rc, out = new()
    base = old()
    for i in range(n):
        assert (rc[i] != 0) == (base[i][0] is None) and (rc[i] != 0 or ang[i] == base[i][0]), "the legs' angles differ"
    rate = {"new": [], "old": []}
    for _ in range(runs):
        for name, fn in (("new", new), ("old", old)):
            t = time.perf_counter()
            fn()
            rate[name].append(n / (time.perf_counter() - t))
    r = float(np.median(rate["new"])) / float(np.median(rate["old"]))
    return "| %s, files to files, %d dataset sheets (%d without a segment) | %s | %s | %s%.2f x%s |" % (
        which, n, int((rc != 0).sum()), fmt(rate["new"]), fmt(rate["old"]), "**" if r < 1 else "", r, "**" if r < 1 else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resident", type=int, default=256)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip", action="append", default=[])
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_detector_deskew.md"))
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    import oics
    if oics.lib().omr_device_count() < 1:
        raise SystemExit("bench_detector_deskew needs a GPU: there is nothing to time without one")
    lines = ["# Deskew with the Hough and FFT detectors, in batches (tools/bench_detector_deskew.py)", "",
             "Commit: %s.  One MI355X.  Hough (%g, %g), FFT (%g, %g, %g, %g), rotate_mat LINEAR, white border, CONTAIN, JPEG "
             "quality %d: the reference benchmark's arguments.  `new` is the flow of this section of DESIGN.md (4.24), `baseline` "
             "what a caller had to assemble before it; %d alternating passes after a warm-up of both, in which their angles (f64 "
             "bits) and stream lengths are compared; median (min .. max) scans/s on a host clock." % ((a.commit,) + HOUGH + FFT + (QUALITY, a.runs)), ""]
    d, stride = resident_cards(a.resident)
    lines += gray_section(d, stride, a.resident, max(a.runs, 3))
    print("\n".join(lines), file=sys.stderr, flush=True)
    table = ["## The flows", "",
             "Device-resident: the flow + omr_jpeg_encode_batch_device against a loop of omr_rgb_to_gray_device calls + the batch "
             "detector + omr_rotate_batch_device_ex + the same encoder.  Files to files: the _streams form against Pillow's decode "
             "+ omr_rgb_to_gray + the per-call detector + omr_rotate_ex + Pillow's save, 16 threads.", "",
             "| flow | new | baseline | new / baseline |", "|---|---|---|---|"]
    ds = os.path.join(ROOT, "tests", "golden", "dataset")
    sheets = [open(os.path.join(ds, f), "rb").read() for f in sorted(os.listdir(ds)) if f.lower().endswith(".jpg")]
    streams = [sheets[i % len(sheets)] for i in range(a.n)]
    for which in ("hough", "fft"):
        if which in a.skip:
            continue
        table.append(device_section(which, d, stride, a.resident, a.runs))
        print(table[-1], file=sys.stderr, flush=True)
        table.append(files_section(which, streams, a.runs))
        print(table[-1], file=sys.stderr, flush=True)
    text = "\n".join(lines + table + [""])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
