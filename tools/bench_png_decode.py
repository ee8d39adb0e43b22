"""The device PNG decoder (development aid): images/s of omr_png_decode_batch_device at 256 streams a call -- host
streams in, device-resident BGR images out, headers, CRC, upload and the final synchronise included -- against Pillow
decoding the same streams to contiguous BGR arrays on one core and from 16 threads.  Stream sets: the dataset's sheets
(tests/golden/dataset) re-written by Pillow as 8-bit gray PNG and as RGB PNG, the A4 colour card of oics.synth as RGB PNG,
the same card thresholded to a 1-bit PNG.  A warm-up of every leg, then alternating passes; the median and the spread of
each leg are reported, and the stage times of one further call with omr_png_decode_stats on.  Then the flow from files:
omr_correct_default_batch_streams on PNG inputs against omr_correct_default_batch_jpeg with Pillow's decode of the same
files on 16 threads inside the timed region, outputs compared.

Every step that uses the GPU is a child process under a `timeout` of its own; the steps are chained, and the first one that
fails ends the run.
Usage: python tools/bench_png_decode.py [--n N] [--a4-n N] [--a4-sheets N] [--runs R] [--commit TEXT] [--out FILE] [--step-seconds S]
Writes a markdown report (default profiles/r19_png_decode.md) and prints it."""
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

PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)   # correct_default's, lib.rs:192-205
SETS = ["dataset sheets as 8-bit gray PNG", "dataset sheets as RGB PNG", "A4 colour cards 2480 x 3508 as RGB PNG",
        "A4 cards thresholded to 1-bit PNG"]


def pillow_bgr(stream):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))[..., ::-1])


def as_png(im):
    b = io.BytesIO()
    im.save(b, format="PNG")
    return b.getvalue()


def workload(k, n):
    from PIL import Image
    from oics import png, synth
    if k < 2:
        d = os.path.join(ROOT, "tests", "golden", "dataset")
        files = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")]
        s = [as_png(Image.open(f).convert("L" if k == 0 else "RGB")) for f in files[:min(len(files), n)]]
    else:
        cards = [synth.make_color_card(3508, 2480, 40 + i)[0] for i in range(min(8, n))]
        ims = [Image.fromarray(c[..., ::-1]) for c in cards]
        s = [as_png(im if k == 2 else im.convert("L").point(lambda v: 255 * (v > 127)).convert("1")) for im in ims]
    streams = [s[i % len(s)] for i in range(n)]
    sizes = [png.info(x)[:2] for x in s]
    return streams, max(r for r, _ in sizes), max(c for _, c in sizes)


def fmt(v):
    return "%.0f (%.0f .. %.0f)" % (float(np.median(v)), min(v), max(v))


def step_decode(k, n, runs):
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    from oics import png
    streams, rows, cols = workload(k, n)
    step = cols * 3
    out = torch.empty((n, rows * step), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def device():
        _, rc = png.decode_batch_device(streams, 3, out.data_ptr(), rows * step, step, rows, cols)
        assert (rc == 0).all(), rc

    sub = streams[: max(n // 16, 1)]   # one core is slow: a sixteenth of the streams, scaled

    def one_core():
        for s in sub:
            pillow_bgr(s)

    def threads16():
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(pillow_bgr, streams))

    legs = [("device", device, n), ("one", one_core, len(sub)), ("t16", threads16, n)]
    rate = {name: [] for name, _, _ in legs}
    for _, fn, _ in legs:
        fn()
    got = out[:2].cpu().numpy()
    for i in range(min(2, n)):
        r, c = png.info(streams[i])[:2]
        assert (got[i].reshape(rows, step)[:r, :c * 3].reshape(r, c, 3) == pillow_bgr(streams[i])).all(), "differs from Pillow"
    for _ in range(runs):
        for name, fn, cnt in legs:
            t = time.perf_counter()
            fn()
            rate[name].append(cnt / (time.perf_counter() - t))
    png.stats(True)
    device()
    groups, ms = png.stats(False)
    print(json.dumps({"set": k, "n": n, "rate": rate, "groups": groups, "ms": ms, "mb_in": sum(len(s) for s in streams) / 1e6,
                      "mb_out": n * rows * cols * 3 / 1e6}), flush=True)


def step_files(k, n, runs):
    import torch  # noqa: F401
    from oics import omr
    streams, _, _ = workload(k, n)

    def from_streams():
        return omr.correct_default_batch_streams(streams, *PARAMS)

    def parent():
        with ThreadPoolExecutor(16) as ex:
            imgs = list(ex.map(pillow_bgr, streams))
        return omr.correct_default_batch_jpeg(imgs, *PARAMS)

    g, w = from_streams(), parent()
    assert g == w and all(t[3] == 0 for t in g), "the two flows differ"
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_png_decode.md"))
    ap.add_argument("--a4-n", type=int, default=256, help="streams a call of the two A4 sets")
    ap.add_argument("--a4-sheets", type=int, default=64)
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--step", default=None, help="internal: decode:K or files:K")
    a = ap.parse_args()
    if a.step:
        kind, k = a.step.split(":")
        return (step_decode if kind == "decode" else step_files)(int(k), a.n, a.runs)
    # the long-running A4 colour steps last: a step that runs into its limit ends the run
    steps = [("decode:0", a.n), ("decode:1", a.n), ("decode:3", a.a4_n), ("files:0", a.n), ("files:1", a.n), ("decode:2", a.a4_n),
             ("files:2", a.a4_sheets)]
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
    from oics import png
    lines = ["# PNG decoding on the device (tools/bench_png_decode.py)", "",
             "Commit: %s.  One MI355X, n streams a call (%d unless the row says otherwise), %d alternating passes after a warm-up of every leg; median "
             "(min .. max) images/s.  The device leg is omr_png_decode_batch_device from host streams to device-resident BGR "
             "slots: chunk walk, CRC, upload and the final synchronise included.  Pillow decodes the same streams to "
             "contiguous BGR arrays on the same machine's cores (the GPU machine allows 16)." % (a.commit, a.n, a.runs), "",
             "| streams | n | MB in | MB out | device | Pillow, 1 core | Pillow, 16 threads | device / 16 threads |",
             "|---|---|---|---|---|---|---|---|"]
    stage = ["", "## Device time per stage", "",
             "One further call of the same streams with omr_png_decode_stats on (events between the stages), ms.", "",
             "| streams | groups | " + " | ".join(png.STAGES) + " | sum |", "|---|---|" + "---|" * 5]
    for k in range(4):
        if "decode:%d" % k not in results:
            continue
        r = results["decode:%d" % k]
        rate = r["rate"]
        lines.append("| %s | %d | %.1f | %.0f | %s | %s | %s | %.2f x |" % (
            SETS[k], r["n"], r["mb_in"], r["mb_out"], fmt(rate["device"]), fmt(rate["one"]), fmt(rate["t16"]),
            np.median(rate["device"]) / np.median(rate["t16"])))
        stage.append("| %s | %d | %s | %.1f |" % (SETS[k], r["groups"], " | ".join("%.2f" % v for v in r["ms"]), sum(r["ms"])))
    lines += stage
    lines += ["", "## correct_default from files", "",
              "omr_correct_default_batch_streams on PNG inputs (file contents in, JPEG file contents out, quality 100) against "
              "omr_correct_default_batch_jpeg with Pillow's decode of the same files to BGR on 16 threads inside the timed "
              "region -- what a caller of the parent commit does.  Sheets/s, alternating passes; the outputs of the two are "
              "compared and equal.", "",
              "| sheets | n | from streams | Pillow on 16 threads + batch_jpeg | streams / parent |", "|---|---|---|---|---|"]
    for name in ("files:0", "files:1", "files:2"):
        if name not in results:
            continue
        r = results[name]
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
