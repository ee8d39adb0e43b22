"""Deskew with projections from file contents to file contents (development aid): scans/s of
omr_deskew_with_projections_batch_streams at (45, 0.2, 0.2), LINEAR, white border, quality 100 -- the reference benchmark's
parameters, core/src/main.rs:68-95 -- against two baselines on the same machine in the same run:
  (a) Pillow's decode on 16 threads, omr_deskew_with_projections_batch, Pillow's JPEG save on 16 threads;
  (b) the per-call pair omr_get_angle_with_projections + omr_rotate from 16 threads with Pillow on both ends.
Workloads: the dataset's sheets as gray JPEG (channels 3 and 1) and as RGB PNG, A4 colour cards as JPEG at quality 100
and 95.  A warm-up of every leg, then alternating passes; the median and the spread of each leg are reported.  Then the
stage times of one chunk: the three phases of a run (decode, context run, encode + download) repeated with the public
device entry points on the same streams, a wall clock around each, with the decoders' own counters beside them.
Usage: python tools/bench_projection_streams.py [--n N] [--a4 N] [--runs R] [--commit TEXT] [--out FILE]
Writes a markdown report (default profiles/r21_projection_streams.md) and prints it."""
import argparse
import io
import os
import re
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SWEEP = (45, 0.2, 0.2)   # core/src/main.rs:68
LINEAR, QUALITY, WHITE = 1, 100, (255, 255, 255)
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def pillow_decode(stream, channels):
    from PIL import Image
    im = Image.open(io.BytesIO(stream))
    if channels == 1:
        return np.ascontiguousarray(np.asarray(im.convert("L")))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def pillow_jpeg(img, q=QUALITY):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img[..., ::-1] if img.ndim == 3 else img).save(b, format="JPEG", quality=q)
    return b.getvalue()


def pillow_png(stream):
    from PIL import Image
    b = io.BytesIO()
    Image.open(io.BytesIO(stream)).convert("RGB").save(b, format="PNG")
    return b.getvalue()


def workloads(n, a4):
    """[(name, streams, channels)]"""
    from oics import synth
    d = os.path.join(ROOT, "tests", "golden", "dataset")
    sheets = [open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")]
    gray = [sheets[i % len(sheets)] for i in range(n)]
    with ThreadPoolExecutor(16) as ex:
        as_png = list(ex.map(pillow_png, sheets))
    out = [("dataset sheets, gray JPEG, channels 3", gray, 3), ("dataset sheets, gray JPEG, channels 1", gray, 1),
           ("dataset sheets, RGB PNG, channels 3", [as_png[i % len(as_png)] for i in range(n)], 3)]
    cards = [synth.make_color_card(3508, 2480, 40 + i, skew=float(2 * i - 7))[0] for i in range(8)]
    for q in (100, 95):
        s = [pillow_jpeg(c, q) for c in cards]
        out.append(("A4 colour cards 2480 x 3508, JPEG quality %d, channels 3" % q, [s[i % len(s)] for i in range(a4)], 3))
    return out


def legs(streams, channels):
    from oics import projection, transfer
    from oics.types import RotateClipStrategy
    border = WHITE if channels == 3 else (255,)

    def from_streams():
        return projection.deskew_streams(streams, *SWEEP, interp=LINEAR, border=border, quality=QUALITY, channels=channels)

    def host_batch():   # (a)
        with ThreadPoolExecutor(16) as ex:
            imgs = list(ex.map(lambda s: pillow_decode(s, channels), streams))
            ang, rot = projection.get_angles_and_deskew(imgs, *SWEEP, interp=LINEAR, border=border)
            return ang, list(ex.map(pillow_jpeg, rot))

    def one(s):
        img = pillow_decode(s, channels)
        ang = projection.get_angle_with_projections(img, SWEEP[0], SWEEP[1], SWEEP[2], 1)
        rot = transfer.rotate_mat(img, ang, 1.0, LINEAR, 0, tuple(border) + (0,) * (4 - len(border)), RotateClipStrategy.CONTAIN)
        return ang, pillow_jpeg(rot.get_mat())

    def per_call():     # (b)
        with ThreadPoolExecutor(16) as ex:
            return list(ex.map(one, streams))

    return [("streams", from_streams), ("a", host_batch), ("b", per_call)]


def deskew_chunk():
    src = open(os.path.join(ROOT, "omr-img-corrector_amd", "csrc", "flow_frame.hpp")).read()
    return int(re.search(r"const int kDeskewChunk = (\d+);", src).group(1))


def stage_times(streams, channels, runs):
    """one chunk of one shape through the public device entry points -> ms per phase (medians), decoder counters"""
    import torch
    from oics import jpeg, png, projection
    is_png = streams[0][:8] == PNG_SIGNATURE
    info = png.info if is_png else jpeg.info
    rows, cols = info(streams[0])[:2]
    chunk = [s for s in streams if info(s)[:2] == (rows, cols)][:deskew_chunk()]
    z, row = len(chunk), cols * channels
    in_stride = (row * rows + 255) & ~255
    pb = projection.ProjectionBatch(rows, cols, channels, SWEEP[0], SWEEP[1], SWEEP[2], z)
    R, C = pb.deskew_canvas()
    out_step, out_stride = C * channels, C * channels * R
    bound = (jpeg.bound(R, C, channels) + 255) & ~255
    din = torch.empty(z * in_stride, dtype=torch.uint8, device="cuda:0")
    dout = torch.empty(z * out_stride, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(z * bound, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    decode = png.decode_batch_device if is_png else jpeg.decode_batch
    stats = png.stats if is_png else jpeg.decode_stats
    ms = {"decode": [], "context run": [], "encode + download": []}
    counters = None
    for k in range(runs + 1):
        stats(True)
        t0 = time.perf_counter()
        _, rc = decode(chunk, channels, din.data_ptr(), in_stride, row, rows, cols)
        t1 = time.perf_counter()
        counters = stats(False)
        assert (rc == 0).all()
        _, _, size = pb.deskew_device(din.data_ptr(), in_stride, row, z, LINEAR, WHITE, dout.data_ptr(), out_stride, out_step)
        t2 = time.perf_counter()
        lens = jpeg.encode_batch_device(dout.data_ptr(), out_stride, out_step, R, C, channels, size, z, QUALITY, dst.data_ptr(), bound)
        got = [dst[i * bound: i * bound + int(lens[i])].cpu() for i in range(z)]
        t3 = time.perf_counter()
        if k:   # the first pass warms up
            for key, v in zip(ms, (t1 - t0, t2 - t1, t3 - t2)):
                ms[key].append(v * 1e3)
        del got
    pb.close()
    return z, rows, cols, {k: float(np.median(v)) for k, v in ms.items()}, counters, is_png


def fmt(v):
    return "%.0f (%.0f .. %.0f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--a4", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_projection_streams.md"))
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    import oics
    from oics import jpeg, png
    if oics.lib().omr_device_count() < 1:
        raise SystemExit("bench_projection_streams needs a GPU: there is nothing to time without one")
    lines = ["# Deskew with projections from files to files (tools/bench_projection_streams.py)", "",
             "Commit: %s.  One MI355X, sweep (%d, %g, %g), LINEAR, white border, JPEG quality %d out; %d alternating passes "
             "after a warm-up of every leg; median (min .. max) scans/s.  `streams` is "
             "omr_deskew_with_projections_batch_streams, file contents in and out.  (a) is Pillow's decode on 16 threads, "
             "omr_deskew_with_projections_batch, Pillow's JPEG save on 16 threads.  (b) is the per-call pair "
             "omr_get_angle_with_projections + omr_rotate from 16 threads with Pillow on both ends.  The angles of the three "
             "legs are compared." % ((a.commit,) + SWEEP + (QUALITY, a.runs)), "",
             "| workload | n | MB in | streams | (a) host-image batch | (b) per-call pair | streams / (a) | streams / (b) |",
             "|---|---|---|---|---|---|---|---|"]
    stage = ["", "## Stage times of one chunk", "",
             "The three phases of a run of the streams form, repeated with the public device entry points on one chunk of one "
             "shape (omr_jpeg_decode_batch_device or omr_png_decode_batch_device, omr_projection_batch_deskew_device, "
             "omr_jpeg_encode_batch_device into slots of omr_jpeg_bound and a copy of each stream to the host), a wall clock "
             "around each; median ms of %d passes.  The decoder's own counters (omr_jpeg_decode_stats / omr_png_decode_stats) "
             "are device time per stage of the same decode." % a.runs, "",
             "| workload | scans | shape | decode | context run | encode + download | sum | scans/s of the sum | decoder's counters, ms |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, streams, channels in workloads(a.n, a.a4):
        n = len(streams)
        print("..", name, file=sys.stderr, flush=True)
        run = legs(streams, channels)
        res = {k: fn() for k, fn in run}   # warm-up, and the answers
        ang = res["streams"][0]
        assert (res["streams"][1] == 0).all()
        assert (np.asarray(res["a"][0]) == ang).all() and [t[0] for t in res["b"]] == list(ang), "the legs' angles differ"
        del res
        rate = {k: [] for k, _ in run}
        for _ in range(a.runs):
            for k, fn in run:
                t = time.perf_counter()
                fn()
                rate[k].append(n / (time.perf_counter() - t))
        med = {k: float(np.median(v)) for k, v in rate.items()}
        lines.append("| %s | %d | %.1f | %s | %s | %s | %s%.2f x%s | %s%.2f x%s |" % (
            name, n, sum(len(s) for s in streams) / 1e6, fmt(rate["streams"]), fmt(rate["a"]), fmt(rate["b"]),
            "**" if med["streams"] < med["a"] else "", med["streams"] / med["a"], "**" if med["streams"] < med["a"] else "",
            "**" if med["streams"] < med["b"] else "", med["streams"] / med["b"], "**" if med["streams"] < med["b"] else ""))
        z, rows, cols, ms, counters, is_png = stage_times(streams, channels, a.runs)
        names = png.STAGES if is_png else jpeg.STAGES
        own = counters[1] if is_png else counters[3]
        total = sum(ms.values())
        stage.append("| %s | %d | %d x %d | %.1f | %.1f | %.1f | %.1f | %.0f | %s |" % (
            name, z, rows, cols, ms["decode"], ms["context run"], ms["encode + download"], total, z / total * 1e3,
            ", ".join("%s %.1f" % (k, v) for k, v in zip(names, own))))
    text = "\n".join(lines + stage + [""])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
