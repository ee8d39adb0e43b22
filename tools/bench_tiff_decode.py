"""The device TIFF decoder (development aid): images/s of omr_tiff_decode_batch_device at 256 streams a call -- host streams
in, device-resident BGR images out, headers, upload and the final synchronise included -- against Pillow (libtiff) decoding
the same streams to contiguous BGR arrays from 16 threads.  Stream sets: the A4 card of oics.synth thresholded, as Group 4
in one strip, Group 4 in Pillow's default strips, PackBits and uncompressed; the dataset's sheets (tests/golden/dataset)
thresholded to Group 4.  A warm-up of every leg, then alternating passes; the median and the spread of each leg are
reported, and the stage times of one further call with omr_tiff_decode_stats on.  Then the flow from files:
omr_deskew_with_projections_batch_streams on Group 4 inputs against Pillow's decode on 16 threads followed by
omr_deskew_with_projections_batch and the device JPEG encoder, outputs compared.

Every step that uses the GPU is a child process under a `timeout` of its own; the steps are chained, and the first one that
fails ends the run.
Usage: python tools/bench_tiff_decode.py [--n N] [--files-n N] [--runs R] [--commit TEXT] [--out FILE] [--step-seconds S]
Writes a markdown report (default profiles/r24_tiff_decode.md) and prints it."""
import argparse
import io
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SWEEP = (10, 0.5, 0.5)
SETS = ["A4 sheets 2480 x 3508, Group 4, one strip", "A4 sheets, Group 4, Pillow's default strips", "A4 sheets, PackBits",
        "A4 sheets, uncompressed", "dataset sheets thresholded, Group 4"]


def pillow_bgr(stream):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))[..., ::-1])


def as_tiff(im, compression, rps=None):
    b = io.BytesIO()
    kw = {"tiffinfo": {278: rps}} if rps else {}
    im.save(b, format="TIFF", compression=compression, **kw)
    return b.getvalue()


def workload(k, n):
    from PIL import Image
    from oics import synth, tiff
    if k == 4:
        d = os.path.join(ROOT, "tests", "golden", "dataset")
        files = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")]
        ims = [Image.open(f).convert("L").point(lambda v: 255 * (v > 127)).convert("1") for f in files[:min(len(files), n)]]
        s = [as_tiff(im, "group4") for im in ims]
    else:
        ims = [Image.fromarray(synth.make_binary_card(3508, 2480, 40 + i, skew=float(i - 3))[0]).convert("1") for i in range(min(8, n))]
        comp = ("group4", "group4", "packbits", "raw")[k]
        s = [as_tiff(im, comp, 3508 if k == 0 else None) for im in ims]
    streams = [s[i % len(s)] for i in range(n)]
    sizes = [tiff.info(x) for x in s]
    return streams, max(t[0] for t in sizes), max(t[1] for t in sizes), max(t[5] for t in sizes)


def fmt(v):
    return "%.0f (%.0f .. %.0f)" % (float(np.median(v)), min(v), max(v))


def step_decode(k, n, runs):
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    from oics import tiff
    streams, rows, cols, strips = workload(k, n)
    step = cols * 3
    out = torch.empty((n, rows * step), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def device():
        _, rc = tiff.decode_batch_device(streams, 3, out.data_ptr(), rows * step, step, rows, cols)
        assert (rc == 0).all(), rc

    def threads16():
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(pillow_bgr, streams))

    legs = [("device", device), ("t16", threads16)]
    rate = {name: [] for name, _ in legs}
    for _, fn in legs:
        fn()
    got = out[:2].cpu().numpy()
    for i in range(min(2, n)):
        r, c = tiff.info(streams[i])[:2]
        assert (got[i].reshape(rows, step)[:r, :c * 3].reshape(r, c, 3) == pillow_bgr(streams[i])).all(), "differs from Pillow"
    for _ in range(runs):
        for name, fn in legs:
            t = time.perf_counter()
            fn()
            rate[name].append(n / (time.perf_counter() - t))
    tiff.stats(True)
    device()
    groups, ms = tiff.stats(False)
    print(json.dumps({"set": k, "n": n, "rate": rate, "groups": groups, "ms": ms, "strips": strips,
                      "mb_in": sum(len(s) for s in streams) / 1e6, "mb_out": n * rows * cols * 3 / 1e6}), flush=True)


def step_files(k, n, runs):
    import torch  # noqa: F401
    from oics import jpeg, projection
    streams, _, _, _ = workload(k, n)

    def from_streams():
        return projection.deskew_streams(streams, *SWEEP, interp=1, quality=95)

    def parent():
        with ThreadPoolExecutor(16) as ex:
            imgs = list(ex.map(pillow_bgr, streams))
        ang, rot = projection.get_angles_and_deskew(imgs, *SWEEP, interp=1)
        return ang, [jpeg.encode(r, 95) for r in rot]

    g, w = from_streams(), parent()
    assert (np.asarray(g[0]).view(np.uint64) == np.asarray(w[0]).view(np.uint64)).all() and list(g[-1]) == w[1], "the two flows differ"
    rate = {"s": [], "p": []}
    for _ in range(runs):
        for name, fn in (("s", from_streams), ("p", parent)):
            t = time.perf_counter()
            fn()
            rate[name].append(n / (time.perf_counter() - t))
    print(json.dumps({"set": k, "n": n, "rate": rate}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--files-n", type=int, default=64, help="sheets a call of the files-to-files legs")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_tiff_decode.md"))
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--step", default=None, help="internal: decode:K or files:K")
    a = ap.parse_args()
    if a.step:
        kind, k = a.step.split(":")
        return (step_decode if kind == "decode" else step_files)(int(k), a.n, a.runs)
    steps = [("decode:4", a.n), ("decode:0", a.n), ("decode:1", a.n), ("decode:2", a.n), ("decode:3", a.n), ("files:4", a.files_n),
             ("files:0", a.files_n)]
    results, failed = {}, None
    for name, n in steps:   # chained: a step that fails, faults or runs into its limit ends the run
        print("..", name, file=sys.stderr, flush=True)
        p = subprocess.run(["timeout", "-k", "10", str(a.step_seconds), sys.executable, os.path.abspath(__file__), "--step", name,
                            "--n", str(n), "--runs", str(a.runs)], capture_output=True, text=True)
        if p.returncode != 0:   # no further step starts; the report holds what was measured and names this one
            failed = "step %s (%d streams) ended with %d and is not in the tables; no further step was started" % (name, n, p.returncode)
            print(failed + ":\n" + p.stderr[-2000:], file=sys.stderr, flush=True)
            break
        results[name] = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    from oics import tiff
    lines = ["# Bilevel TIFF decoding on the device (tools/bench_tiff_decode.py)", "",
             "Commit: %s.  One MI355X, %d streams a call, %d alternating passes after a warm-up of every leg; median (min .. max) "
             "images/s.  The device leg is omr_tiff_decode_batch_device from host streams to device-resident BGR slots: IFD "
             "walk, upload and the final synchronise included.  Pillow (libtiff) decodes the same streams to contiguous BGR "
             "arrays from 16 threads of the same machine." % (a.commit, a.n, a.runs), "",
             "| streams | n | strips a page | MB in | MB out | device | Pillow, 16 threads | device / 16 threads |",
             "|---|---|---|---|---|---|---|---|"]
    stage = ["", "## Device time per stage", "",
             "One further call of the same streams with omr_tiff_decode_stats on (events between the stages), ms.", "",
             "| streams | groups | " + " | ".join(tiff.STAGES) + " | sum |", "|---|---|" + "---|" * 5]
    for k in (4, 0, 1, 2, 3):
        if "decode:%d" % k not in results:
            continue
        r = results["decode:%d" % k]
        rate = r["rate"]
        ratio = np.median(rate["device"]) / np.median(rate["t16"])
        lines.append("| %s | %d | %d | %.1f | %.0f | %s | %s | %s |" % (
            SETS[k], r["n"], r["strips"], r["mb_in"], r["mb_out"], fmt(rate["device"]), fmt(rate["t16"]),
            "%.2f x" % ratio if ratio >= 1 else "**%.2f x: the device path does not win**" % ratio))
        stage.append("| %s | %d | %s | %.1f |" % (SETS[k], r["groups"], " | ".join("%.2f" % v for v in r["ms"]), sum(r["ms"])))
    lines += stage
    lines += ["", "## Deskew with projections from files to files", "",
              "omr_deskew_with_projections_batch_streams on Group 4 inputs (file contents in, JPEG file contents out, quality 95, "
              "sweep %s) against Pillow's decode of the same files to BGR on 16 threads, omr_deskew_with_projections_batch and "
              "omr_jpeg_encode of every canvas, all inside the timed region.  Sheets/s, alternating passes; the angles and the "
              "outputs of the two are compared and equal." % (SWEEP,), "",
              "| sheets | n | from streams | Pillow on 16 threads + host-image flow | streams / parent |", "|---|---|---|---|---|"]
    for name in ("files:4", "files:0"):
        if name not in results:
            continue
        r = results[name]
        ratio = np.median(r["rate"]["s"]) / np.median(r["rate"]["p"])
        lines.append("| %s | %d | %s | %s | %s |" % (SETS[r["set"]], r["n"], fmt(r["rate"]["s"]), fmt(r["rate"]["p"]),
                                                    "%.2f x" % ratio if ratio >= 1 else "**%.2f x: the device path does not win**" % ratio))
    if failed:
        lines += ["", "Not measured: " + failed + "."]
    lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
