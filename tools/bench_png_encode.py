"""The device PNG encoder (development aid): images/s of omr_png_encode_batch_device at n device-resident canvases a call,
its stage times (omr_png_encode_stats), Pillow's save(format="PNG", compress_level=1) of the same images on one core and
from 16 threads in alternating passes, and the stream sizes against tests/png_ref.py's write(filters=1, level=1,
strategy=Z_RLE) -- what imwrite(.., PNG) writes with OpenCV 4.6's defaults -- and against zlib level 6 with Paeth.
Image sets: the dataset's sheets (tests/golden/dataset) as gray and as colour, the A4 colour card of oics.synth, the same
card thresholded.  Then the flow from files: omr_correct_default_batch_streams_png against omr_correct_default_batch
followed by Pillow's PNG save on 16 threads.

Every step that uses the GPU is a child process under a `timeout` of its own; the steps are chained, and the first one that
fails ends the run.
Usage: python tools/bench_png_encode.py [--n N] [--a4-n N] [--runs R] [--commit TEXT] [--out FILE] [--step-seconds S]
Writes a markdown report (default profiles/r20_png_encode.md) and prints it."""
import argparse
import io
import json
import os
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)   # correct_default's, lib.rs:192-205
SETS = ["dataset sheets, gray", "dataset sheets, colour", "A4 colour cards 2480 x 3508", "A4 cards thresholded, gray"]


def pillow_png(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img[..., ::-1] if img.ndim == 3 else img).save(b, format="PNG", compress_level=1)
    return b.getvalue()


def images(k, n):
    """-> (distinct images of one shape, n indices into them)"""
    from PIL import Image
    from oics import synth
    if k < 2:
        d = os.path.join(ROOT, "tests", "golden", "dataset")
        files = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")][:8]
        ims = [np.asarray(Image.open(f).convert("L" if k == 0 else "RGB")) for f in files]
        r, c = min(i.shape[0] for i in ims), min(i.shape[1] for i in ims)
        ims = [np.ascontiguousarray(i[:r, :c] if k == 0 else i[:r, :c, ::-1]) for i in ims]
    else:
        ims = [synth.make_color_card(3508, 2480, 40 + i)[0] for i in range(4)]
        if k == 3:
            ims = [np.ascontiguousarray(((i.astype(np.int32).sum(2) // 3 > 127) * 255).astype(np.uint8)) for i in ims]
    return ims, [i % len(ims) for i in range(n)]


def step_encode(k, n, runs):
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    import png_ref
    from oics import png
    ims, idx = images(k, n)
    rows, cols = ims[0].shape[:2]
    cn = 1 if ims[0].ndim == 2 else 3
    step = cols * cn
    distinct = torch.from_numpy(np.stack([im.reshape(-1) for im in ims])).to("cuda:0")   # n canvases, gathered on the device
    src = distinct[torch.tensor(idx, device="cuda:0")].contiguous()
    del distinct
    bound = png.bound(rows, cols, cn)
    out = torch.empty((n, bound), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lens = []

    def device():
        lens[:] = png.encode_batch_device(src.data_ptr(), rows * step, step, rows, cols, cn, None, n, 1, out.data_ptr(), bound)

    sub = idx[: max(n // 16, 1)]

    def one_core():
        for i in sub:
            pillow_png(ims[i])

    def threads16():
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda i: pillow_png(ims[i]), idx))

    legs = [("device", device, n), ("one", one_core, len(sub)), ("t16", threads16, n)]
    rate = {name: [] for name, _, _ in legs}
    for _, fn, _ in legs:
        fn()
    from PIL import Image
    first = out[0, : int(lens[0])].cpu().numpy().tobytes()
    dec = np.asarray(Image.open(io.BytesIO(first)))
    assert (dec == (ims[0] if cn == 1 else ims[0][..., ::-1])).all(), "the stream does not decode to the image"
    for _ in range(runs):
        for name, fn, cnt in legs:
            t = time.perf_counter()
            fn()
            rate[name].append(cnt / (time.perf_counter() - t))
    png.encode_stats(True)
    device()
    groups, ms = png.encode_stats(False)
    raw = rows * (1 + step)
    a = ims[0] if cn == 1 else ims[0][..., ::-1]
    imwrite_like = len(png_ref.write(a, 0 if cn == 1 else 2, filters=1, level=1, strategy=zlib.Z_RLE))
    paeth6 = len(png_ref.write(a, 0 if cn == 1 else 2, filters=4, level=6))
    print(json.dumps({"set": k, "n": n, "rate": rate, "groups": groups, "ms": ms, "raw": raw, "device_bytes": int(lens[0]),
                      "pillow_bytes": len(pillow_png(ims[0])), "imwrite_bytes": imwrite_like, "paeth6_bytes": paeth6}), flush=True)


def step_files(k, n, runs):
    import torch  # noqa: F401
    from PIL import Image
    from oics import omr
    ims, idx = images(k, n)
    streams = []
    for im in ims:
        b = io.BytesIO()
        Image.fromarray(im[..., ::-1] if im.ndim == 3 else im).save(b, format="PNG")
        streams.append(b.getvalue())
    streams = [streams[i] for i in idx]
    bgr = [ims[i] if ims[i].ndim == 3 else np.repeat(ims[i][..., None], 3, 2) for i in idx]

    def from_streams():
        return omr.correct_default_batch_streams_png(streams, *PARAMS)

    def host_save():
        res = omr.correct_default_batch(bgr, *PARAMS)
        with ThreadPoolExecutor(16) as ex:
            return list(ex.map(lambda r: pillow_png(r[2]) if r[3] == 0 else None, res))

    from_streams(), host_save()
    rate = {"s": [], "p": []}
    for _ in range(runs):
        for name, fn in (("s", from_streams), ("p", host_save)):
            t = time.perf_counter()
            fn()
            rate[name].append(n / (time.perf_counter() - t))
    print(json.dumps({"set": k, "n": n, "rate": rate}), flush=True)


def fmt(v):
    return "%.0f (%.0f .. %.0f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--a4-n", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_png_encode.md"))
    ap.add_argument("--step-seconds", type=int, default=420)   # 256 A4 colour cards: Pillow alone takes 26 s a pass
    ap.add_argument("--step", default=None, help="internal: encode:K or files:K")
    a = ap.parse_args()
    if a.step:
        kind, k = a.step.split(":")
        return (step_encode if kind == "encode" else step_files)(int(k), a.n, a.runs)
    steps = [("encode:0", a.n), ("encode:1", a.n), ("encode:3", a.a4_n), ("encode:2", a.a4_n), ("files:0", a.n), ("files:1", a.n)]
    results, failed = {}, None
    for name, n in steps:   # chained: a step that fails, faults or runs into its limit ends the run
        print("..", name, file=sys.stderr, flush=True)
        p = subprocess.run(["timeout", "-k", "10", str(a.step_seconds), sys.executable, os.path.abspath(__file__), "--step", name,
                            "--n", str(n), "--runs", str(a.runs)], capture_output=True, text=True)
        if p.returncode != 0:
            failed = "step %s (%d images) ended with %d and is not in the tables; no further step was started" % (name, n, p.returncode)
            print(failed + ":\n" + p.stderr[-2000:], file=sys.stderr, flush=True)
            break
        results[name] = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    from oics import png
    lines = ["# PNG encoding on the device (tools/bench_png_encode.py)", "",
             "Commit: %s.  One MI355X, n device-resident canvases a call, compression 1, %d alternating passes after a warm-up of "
             "every leg; median (min .. max) images/s.  The device leg is omr_png_encode_batch_device into device slots, its "
             "host round trip for the lengths included.  Pillow saves the same images with compress_level=1 on the same "
             "machine's cores (the GPU machine allows 16)." % (a.commit, a.runs), "",
             "| images | n | device | Pillow, 1 core | Pillow, 16 threads | device / 16 threads |", "|---|---|---|---|---|---|"]
    stage = ["", "## Device time per stage", "", "One further call with omr_png_encode_stats on, ms.", "",
             "| images | groups | " + " | ".join(png.STAGES_ENC) + " | sum |", "|---|---|" + "---|" * 7]
    size = ["", "## Stream sizes", "",
            "Bytes of the first image's stream as a share of its raw data, rows x (1 + row bytes).  imwrite's defaults: Sub "
            "filter, zlib level 1, Z_RLE (tests/png_ref.py); zlib 6: Paeth filter, default strategy.", "",
            "| images | raw | device | imwrite's defaults | Pillow level 1 | zlib 6 with Paeth |", "|---|---|---|---|---|---|"]
    for k in range(4):
        r = results.get("encode:%d" % k)
        if not r:
            continue
        rate = r["rate"]
        lines.append("| %s | %d | %s | %s | %s | %.2f x |" % (SETS[k], r["n"], fmt(rate["device"]), fmt(rate["one"]), fmt(rate["t16"]),
                                                            np.median(rate["device"]) / np.median(rate["t16"])))
        stage.append("| %s | %d | %s | %.1f |" % (SETS[k], r["groups"], " | ".join("%.2f" % v for v in r["ms"]), sum(r["ms"])))
        size.append("| %s | %d | %.3f | %.3f | %.3f | %.3f |" % (SETS[k], r["raw"], r["device_bytes"] / r["raw"], r["imwrite_bytes"] / r["raw"],
                                                             r["pillow_bytes"] / r["raw"], r["paeth6_bytes"] / r["raw"]))
    lines += stage + size
    lines += ["", "## correct_default from files to PNG files", "",
              "omr_correct_default_batch_streams_png on PNG inputs against omr_correct_default_batch on decoded sheets followed "
              "by Pillow's PNG save (compress_level=1) of the canvases on 16 threads.  Sheets/s, alternating passes.", "",
              "| sheets | n | streams_png | batch + Pillow save on 16 threads | ratio |", "|---|---|---|---|---|"]
    for name in ("files:0", "files:1"):
        r = results.get(name)
        if r:
            lines.append("| %s | %d | %s | %s | %.2f x |" % (SETS[r["set"]], r["n"], fmt(r["rate"]["s"]), fmt(r["rate"]["p"]),
                                                            np.median(r["rate"]["s"]) / np.median(r["rate"]["p"])))
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
