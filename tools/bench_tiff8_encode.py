"""The device 8-bit TIFF encoder (development aid): images/s of omr_tiff8_encode_batch_device at n device-resident
canvases a call -- A4 gray and colour pages with paper noise (bench_tiff8_decode.py's), thresholded A4 cards and the
dataset's sheets; LZW with Predictor 1 and 2 and uncompressed; default strips and one strip a page -- its stage times
(omr_tiff8_encode_stats), the files' sizes as a share of the raw data beside Pillow's, and Pillow's
save(compression="tiff_lzw") of the same pictures (--host-n of them a call) from 16 threads of the same machine.  Then the flow from files:
projection.deskew_streams_tiff8 on gray LZW A4 sheets against the same flow's PNG outputs.
Usage: python tools/bench_tiff8_encode.py [--n N] [--host-n N] [--files-n N] [--runs R] [--sets 0,1,2,3] [--commit TEXT] [--out FILE]
Writes a markdown report (default profiles/r28_tiff8_encode.md) and prints it."""
import argparse
import io
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

SETS = ["A4 pages with paper noise, gray", "A4 pages with paper noise, BGR", "A4 cards thresholded, gray", "dataset sheets, gray"]
MODES = [("LZW", 5, 1), ("LZW, Predictor 2", 5, 2), ("uncompressed", 1, 1)]
PROJ = (45, 0.2, 0.2)


_IMAGES = {}


def images(k):
    """-> distinct images of one shape, made once"""
    if k not in _IMAGES:
        _IMAGES[k] = _images(k)
    return _IMAGES[k]


def _images(k):
    from PIL import Image
    from bench_tiff8_decode import page
    from oics import synth
    if k < 2:
        return [np.ascontiguousarray(page(i, k == 1)) for i in range(4)]
    if k == 2:
        return [np.where(synth.make_card(3508, 2480, 40 + i)[0] > 127, 255, 0).astype(np.uint8) for i in range(4)]
    d = os.path.join(ROOT, "tests", "golden", "dataset")
    files = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")][:8]
    ims = [np.asarray(Image.open(f).convert("L")) for f in files]
    r, c = min(i.shape[0] for i in ims), min(i.shape[1] for i in ims)
    return [np.ascontiguousarray(i[:r, :c]) for i in ims]


def pillow_lzw(img, comp, pred, rps):
    b = io.BytesIO()
    info = {}
    if rps:
        info[278] = rps
    if pred == 2:
        info[317] = 2
    img.save(b, format="TIFF", compression="tiff_lzw" if comp == 5 else "raw", **({"tiffinfo": info} if info else {}))
    return b.getvalue()


def fmt(v):
    return "%.0f (%.0f .. %.0f)" % (float(np.median(v)), min(v), max(v))


def bench_encode(k, n, host_n, runs, comp, pred, one_strip):
    import torch
    from PIL import Image
    import tiff8_ref
    from oics import tiff
    ims = images(k)
    idx = [i % len(ims) for i in range(n)]
    rows, cols = ims[0].shape[:2]
    cn = 1 if ims[0].ndim == 2 else 3
    rps = rows if one_strip else 0
    step = cols * cn
    distinct = torch.from_numpy(np.stack([im.reshape(-1) for im in ims])).to("cuda:0")
    src = distinct[torch.tensor(idx, device="cuda:0")].contiguous()
    del distinct
    bound = tiff.bound8(rows, cols, cn, comp, rps)
    out = torch.empty((n, bound), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lens = []

    def device():
        lens[:] = tiff.encode8_batch_device(src.data_ptr(), rows * step, step, rows, cols, cn, None, n, out.data_ptr(), bound, comp, pred, rps, 300)

    pil = [Image.fromarray(im if cn == 1 else np.ascontiguousarray(im[..., ::-1])) for im in ims]

    def threads16():
        with ThreadPoolExecutor(16) as ex:
            return list(ex.map(lambda i: len(pillow_lzw(pil[i], comp, pred, rps)), idx[:host_n]))

    device()
    pil_bytes = threads16()[0]
    first = out[0, : int(lens[0])].cpu().numpy().tobytes()
    assert (tiff8_ref.pillow_read(first) == np.asarray(pil[0])).all(), "the file does not decode to the canvas"
    rate = {"device": [], "t16": []}
    for _ in range(runs):
        for name, fn in (("device", device), ("t16", threads16)):
            t = time.perf_counter()
            fn()
            rate[name].append((n if name == "device" else min(n, host_n)) / (time.perf_counter() - t))
    tiff.encode8_stats(True)
    device()
    groups, ms = tiff.encode8_stats(False)
    del src, out
    torch.cuda.empty_cache()
    return dict(rate=rate, groups=groups, ms=ms, bytes=int(lens[0]), pil_bytes=pil_bytes, raw=rows * cols * cn,
                strips=len(tiff8_ref.parse(first)["strips"]))


def bench_files(n, runs):
    import torch  # noqa: F401
    import tiff8_ref
    from oics import projection
    ims = images(0)
    streams = [tiff8_ref.pillow_tiff(im, "tiff_lzw") for im in ims]
    streams = [streams[i % len(streams)] for i in range(n)]
    legs = {"8-bit TIFF out, LZW": lambda: projection.deskew_streams_tiff8(streams, *PROJ, channels=1),
            "8-bit TIFF out, LZW with Predictor 2": lambda: projection.deskew_streams_tiff8(streams, *PROJ, channels=1, predictor=2),
            "8-bit TIFF out, uncompressed": lambda: projection.deskew_streams_tiff8(streams, *PROJ, channels=1, compression=1),
            "PNG out, level 1": lambda: projection.deskew_streams(streams, *PROJ, png=True, quality=1, channels=1)}
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
    ap.add_argument("--host-n", type=int, default=64, help="pictures a call of the Pillow leg")
    ap.add_argument("--files-n", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sets", default="0,1,2,3")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_tiff8_encode.md"))
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True).strip() + " + working tree"
        except Exception:
            commit = "unknown"
    from oics import tiff
    lines = ["# 8-bit gray and RGB TIFF encoding on the device (tools/bench_tiff8_encode.py)", "",
             "Commit: %s.  %d device-resident canvases a call, dpi 300, %d timed calls after one warm-up; median (min .. max) "
             "images/s.  The device leg is omr_tiff8_encode_batch_device into device slots, its one synchronisation and the "
             "host's placing included.  Pillow: save(format=\"TIFF\", compression=\"tiff_lzw\" or \"raw\") of the same pictures "
             "with the same RowsPerStrip and Predictor, %d of them a call, from 16 threads.  A ratio below 1 (bold) is a set "
             "that does not beat the host.  Share of raw: the file's bytes over rows x cols x channels; ours never clears the table on a poor "
             "ratio as libtiff's writer does." % (commit, a.n, a.runs, min(a.n, a.host_n)), "",
             "| set | mode | strips a page | device | Pillow x 16 | ratio | share of raw | Pillow's share |", "|---|---|---|---|---|---|---|---|"]
    stage = ["", "## Device time per stage", "", "One further call with omr_tiff8_encode_stats on, ms (%s)." % ", ".join(tiff.STAGES_ENC8), "",
             "| set | mode | strips a page | groups | " + " | ".join(tiff.STAGES_ENC8) + " |", "|---|---|---|---|" + "---|" * len(tiff.STAGES_ENC8)]
    for k in [int(v) for v in a.sets.split(",") if v != ""]:
        for name, comp, pred in MODES:
            for one_strip in (False, True):
                r = bench_encode(k, a.n, a.host_n, a.runs, comp, pred, one_strip)
                d, p = float(np.median(r["rate"]["device"])), float(np.median(r["rate"]["t16"]))
                lines.append("| %s | %s | %d | %s | %s | %s | %.3f | %.3f |" % (SETS[k], name, r["strips"], fmt(r["rate"]["device"]), fmt(r["rate"]["t16"]),
                                                                           ("%.2f x" if d >= p else "**%.2f x**") % (d / p), r["bytes"] / r["raw"],
                                                                           r["pil_bytes"] / r["raw"]))
                stage.append("| %s | %s | %d | %d | %s |" % (SETS[k], name, r["strips"], r["groups"], " | ".join("%.2f" % v for v in r["ms"])))
                print(lines[-1], flush=True)
                print(stage[-1], flush=True)
    flow = []
    if a.files_n > 0:
        files, in_size = bench_files(a.files_n, a.runs)
        flow = ["", "## From files to files", "",
                "projection.deskew_streams* at (45, 0.2, 0.2), LINEAR, channels = 1, %d gray LZW A4 sheets a call (%.0f bytes a file "
                "in), files/s and bytes a file out, measured in this same session." % (a.files_n, in_size), "", "| outputs | files/s | bytes a file |",
                "|---|---|---|"]
        for name, (rate, size) in files.items():
            flow.append("| %s | %s | %.0f |" % (name, fmt(rate), size))
            print(flow[-1], flush=True)
    text = "\n".join(lines + stage + flow) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
