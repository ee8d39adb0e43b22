"""The device Group 4 TIFF encoder (development aid): images/s of omr_tiff_encode_batch_device at n device-resident
canvases a call -- A4 thresholded cards and the dataset's sheets, gray and BGR, one strip and RowsPerStrip 64 -- its stage
times (omr_tiff_encode_stats), and Pillow's save(format="TIFF", compression="group4") of the same pictures, already
bilevel, from 16 threads of the same machine.  Then the flow from files: omr_deskew_with_projections_batch_streams_tiff on
Group 4 inputs against the same flow with JPEG outputs.
Usage: python tools/bench_tiff_encode.py [--n N] [--files-n N] [--runs R] [--commit TEXT] [--out FILE]
Writes a markdown report (default profiles/r26_tiff_encode.md) and prints it."""
import argparse
import io
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SETS = ["A4 cards thresholded, gray", "A4 cards thresholded, BGR", "dataset sheets, gray", "dataset sheets, BGR"]
PROJ = (45, 0.2, 0.2)


def images(k):
    """-> distinct images of one shape"""
    from PIL import Image
    from oics import synth
    if k < 2:
        ims = [synth.make_card(3508, 2480, 40 + i)[0] for i in range(4)]
        ims = [np.where(i > 127, 255, 0).astype(np.uint8) for i in ims]
    else:
        d = os.path.join(ROOT, "tests", "golden", "dataset")
        files = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")][:8]
        ims = [np.asarray(Image.open(f).convert("L")) for f in files]
        r, c = min(i.shape[0] for i in ims), min(i.shape[1] for i in ims)
        ims = [np.ascontiguousarray(i[:r, :c]) for i in ims]
    if k & 1:
        ims = [np.ascontiguousarray(np.repeat(i[..., None], 3, 2)) for i in ims]
    return ims


def pillow_g4(img1, rps):
    b = io.BytesIO()
    img1.save(b, format="TIFF", compression="group4", **({"tiffinfo": {278: rps}} if rps else {}))
    return b.getvalue()


def fmt(v):
    return "%.0f (%.0f .. %.0f)" % (float(np.median(v)), min(v), max(v))


def bench_encode(k, n, runs, rps):
    import torch
    from PIL import Image
    import tiff_ref
    from oics import tiff
    ims = images(k)
    idx = [i % len(ims) for i in range(n)]
    rows, cols = ims[0].shape[:2]
    cn = 1 if ims[0].ndim == 2 else 3
    step = cols * cn
    distinct = torch.from_numpy(np.stack([im.reshape(-1) for im in ims])).to("cuda:0")
    src = distinct[torch.tensor(idx, device="cuda:0")].contiguous()
    del distinct
    bound = tiff.bound(rows, cols, rps)
    out = torch.empty((n, bound), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lens = []

    def device():
        lens[:] = tiff.encode_batch_device(src.data_ptr(), rows * step, step, rows, cols, cn, None, n, out.data_ptr(), bound, 127, rps, 300)

    bilevel = [Image.fromarray(np.where((im if cn == 1 else im[..., 0]) > 127, 255, 0).astype(np.uint8)).convert("1") for im in ims]

    def threads16():
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda i: pillow_g4(bilevel[i], rps), idx))

    device(), threads16()
    first = out[0, : int(lens[0])].cpu().numpy().tobytes()
    assert tiff_ref.strips_of(first) == tiff_ref.strips_of(pillow_g4(bilevel[0], rps)) or tiff_ref.parse(pillow_g4(bilevel[0], rps))["photometric"] != 0, \
        "the strips are not libtiff's"
    assert (tiff_ref.pillow_read(first) == np.asarray(bilevel[0].convert("L"))).all()
    rate = {"device": [], "t16": []}
    for _ in range(runs):
        for name, fn in (("device", device), ("t16", threads16)):
            t = time.perf_counter()
            fn()
            rate[name].append(n / (time.perf_counter() - t))
    tiff.encode_stats(True)
    device()
    groups, ms = tiff.encode_stats(False)
    del src, out
    torch.cuda.empty_cache()
    return dict(rate=rate, groups=groups, ms=ms, bytes=int(lens[0]), bound=bound, pixels=rows * cols)


def bench_files(n, runs):
    import torch  # noqa: F401
    import tiff_ref
    from oics import projection
    ims = images(0)
    streams = [tiff_ref.pillow_tiff(im == 0) for im in ims]
    streams = [streams[i % len(streams)] for i in range(n)]
    legs = {"TIFF out (Group 4, one strip)": lambda: projection.deskew_streams_tiff(streams, *PROJ),
            "TIFF out, gray (channels = 1)": lambda: projection.deskew_streams_tiff(streams, *PROJ, channels=1),
            "JPEG out, quality 100": lambda: projection.deskew_streams(streams, *PROJ, quality=100),
            "JPEG out, quality 100, gray (channels = 1)": lambda: projection.deskew_streams(streams, *PROJ, quality=100, channels=1)}
    res = {}
    for name, fn in legs.items():
        r = fn()
        assert all(int(c) == 0 for c in r[1])
        size = sum(len(s) for s in r[2]) / n
        rate = []
        for _ in range(runs):
            t = time.perf_counter()
            fn()
            rate.append(n / (time.perf_counter() - t))
        res[name] = (rate, size)
    return res, sum(len(s) for s in streams) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--files-n", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_tiff_encode.md"))
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True).strip() + " + working tree"
        except Exception:
            commit = "unknown"
    from oics import tiff
    lines = ["# Group 4 TIFF encoding on the device (tools/bench_tiff_encode.py)", "",
             "Commit: %s.  %d device-resident canvases a call, threshold 127, dpi 300, %d timed calls after one warm-up; median "
             "(min .. max) images/s.  The device leg is omr_tiff_encode_batch_device into device slots, its one synchronisation "
             "and the host's placing included.  Pillow: save(format=\"TIFF\", compression=\"group4\") of the same pictures, "
             "already converted to mode \"1\", from 16 threads." % (commit, a.n, a.runs), "",
             "| set | RowsPerStrip | device | Pillow x 16 | ratio | bytes a file | bits a pixel | bound a file |", "|---|---|---|---|---|---|---|---|"]
    stage = ["", "## Device time per stage", "", "One further call with omr_tiff_encode_stats on, ms (%s)." % ", ".join(tiff.STAGES_ENC), "",
             "| set | RowsPerStrip | groups | " + " | ".join(tiff.STAGES_ENC) + " | bounds it |", "|---|---|---|" + "---|" * (len(tiff.STAGES_ENC) + 1)]
    for k in range(len(SETS)):
        for rps in (0, 64):
            r = bench_encode(k, a.n, a.runs, rps)
            d, p = float(np.median(r["rate"]["device"])), float(np.median(r["rate"]["t16"]))
            lines.append("| %s | %s | %s | %s | %.1f x | %d | %.3f | %d |" % (SETS[k], rps or "one strip", fmt(r["rate"]["device"]), fmt(r["rate"]["t16"]),
                                                                           d / p, r["bytes"], 8.0 * r["bytes"] / r["pixels"], r["bound"]))
            worst = tiff.STAGES_ENC[int(np.argmax(r["ms"]))]
            stage.append("| %s | %s | %d | %s | %s |" % (SETS[k], rps or "one strip", r["groups"], " | ".join("%.2f" % v for v in r["ms"]), worst))
            print(lines[-1], flush=True)
    files, in_size = bench_files(a.files_n, a.runs)
    flow = ["", "## From files to files", "",
            "omr_deskew_with_projections_batch_streams* at (45, 0.2, 0.2), LINEAR, %d Group 4 A4 cards a call (%.0f bytes a file "
            "in), files/s and bytes a file out." % (a.files_n, in_size), "", "| outputs | files/s | bytes a file |", "|---|---|---|"]
    for name, (rate, size) in files.items():
        flow.append("| %s | %s | %.0f |" % (name, fmt(rate), size))
    text = "\n".join(lines + stage + flow) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
