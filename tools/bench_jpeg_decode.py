"""The device JPEG decoder (development aid): images/s of omr_jpeg_decode_batch_device at 256 streams a call -- host
streams in, device-resident BGR images out -- against Pillow (libjpeg-turbo) decoding the same streams to BGR on one core
and from 16 threads, for the dataset's sheets (tests/golden/dataset, gray baseline streams) and A4 colour cards at quality
100 and 95 (4:2:0).  A warm-up of every leg, then alternating passes; the median and the spread of each leg are reported.
With the decoder's own counters (omr_jpeg_decode_stats): synchronisation rounds and device time per stage.  --libs: the
same device leg in a fresh process per library built with another subsequence length (-DOMR_JDEC_SUB_BITS=..
-DOMR_JDEC_LANES=..).  Then the flow from files: omr_correct_default_batch_streams against omr_correct_default_batch_jpeg
with Pillow's decode of its inputs, on 16 threads, inside the timed region.
Usage: python tools/bench_jpeg_decode.py [--n N] [--runs R] [--commit TEXT] [--out FILE] [--libs A.so B.so ..]
Writes a markdown report (default profiles/r18_jpeg_decode.md) and prints it."""
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


def pillow_bgr(stream):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))[..., ::-1])


def pillow_encode(img, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img[..., ::-1]).save(b, format="JPEG", quality=q)
    return b.getvalue()


PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)   # correct_default's, lib.rs:192-205


def workloads(n):
    from oics import jpeg, synth
    d = os.path.join(ROOT, "tests", "golden", "dataset")
    sheets = [open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.lower().endswith(".jpg")]
    out = [("dataset sheets (gray streams, about 1150 x 1240)", [sheets[i % len(sheets)] for i in range(n)])]
    cards = [synth.make_color_card(3508, 2480, 40 + i)[0] for i in range(8)]
    for q in (100, 95):
        s = [pillow_encode(c, q) for c in cards]
        out.append(("A4 colour cards 2480 x 3508, quality %d, 4:2:0" % q, [s[i % len(s)] for i in range(n)]))
    res = []
    for name, streams in out:
        sizes = [jpeg.info(s)[:2] for s in streams]
        res.append((name, streams, max(r for r, _ in sizes), max(c for _, c in sizes)))
    return res


def device_leg(streams, rows, cols, runs):
    """-> (images/s per pass, stats of a further pass with the collection on), the output checked against Pillow"""
    import torch
    from oics import jpeg
    n, step = len(streams), cols * 3
    out = torch.empty((n, rows * step), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def device():
        _, rc = jpeg.decode_batch(streams, 3, out.data_ptr(), rows * step, step, rows, cols)
        assert (rc == 0).all()

    device()
    rate = []
    for _ in range(runs):
        t = time.perf_counter()
        device()
        rate.append(n / (time.perf_counter() - t))
    jpeg.decode_stats(True)
    device()
    stats = jpeg.decode_stats(False)
    got = out[:2].cpu().numpy()
    for i in range(2):
        r, c = jpeg.info(streams[i])[:2]
        assert (got[i].reshape(rows, step)[:r, :c * 3].reshape(r, c, 3) == pillow_bgr(streams[i])).all()
    return out, device, rate, stats


def fmt(v):
    return "%.0f (%.0f .. %.0f)" % (float(np.median(v)), min(v), max(v))


def child(a):
    """--child: the device leg alone with the library given, one JSON line per workload"""
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    from oics import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
    for name, streams, rows, cols in workloads(a.n):
        out, _, rate, stats = device_leg(streams, rows, cols, a.runs)
        print(json.dumps({"name": name, "rate": rate, "bits": stats[0], "rounds": stats[2], "ms": stats[3]}), flush=True)
        del out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_jpeg_decode.md"))
    ap.add_argument("--libs", nargs="*", default=[])
    ap.add_argument("--lib")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--a4-sheets", type=int, default=64)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch  # noqa: F401  (before the library: the two share one HIP runtime, torch's)
    import oics
    from oics import jpeg, omr
    if oics.lib().omr_device_count() < 1:
        raise SystemExit("bench_jpeg_decode needs a GPU: there is nothing to time without one")
    lines = ["# JPEG decoding on the device (tools/bench_jpeg_decode.py)", "",
             "Commit: %s.  One MI355X, %d streams a call, %d alternating passes after a warm-up of every leg; median "
             "(min .. max) images/s.  The device leg is omr_jpeg_decode_batch_device from host streams to device-resident "
             "BGR slots, header parsing, upload and the final synchronise included.  Pillow decodes the same streams to "
             "contiguous BGR arrays on the same machine's cores (the GPU machine allows 16)." % (a.commit, a.n, a.runs), "",
             "| streams | MB in | MB out | device | Pillow, 1 core | Pillow, 16 threads | device / 16 threads |",
             "|---|---|---|---|---|---|---|"]
    stage_lines = ["", "## Rounds and device time per stage", "",
                   "One further call of the same %d streams with omr_jpeg_decode_stats on (events between the stages; the "
                   "round trips of the synchronisation loop count into its stage).  Subsequences of %%d bits." % a.n, "",
                   "| streams | groups | rounds | " + " | ".join(jpeg.STAGES) + " | sum, ms |", "|---|---|---|" + "---|" * 7]
    own = {}
    loads = workloads(a.n)
    for name, streams, rows, cols in loads:
        n = len(streams)
        print("..", name, file=sys.stderr, flush=True)
        out, device, _, _ = device_leg(streams, rows, cols, 1)
        sub = streams[: max(n // 16, 1)]   # one core is slow: a sixteenth of the streams, scaled

        def one_core():
            for s in sub:
                pillow_bgr(s)

        def threads16():
            with ThreadPoolExecutor(16) as ex:
                list(ex.map(pillow_bgr, streams))

        legs = [("device", device, n), ("one", one_core, len(sub)), ("t16", threads16, n)]
        rate = {k: [] for k, _, _ in legs}
        for _, fn, _ in legs[1:]:
            fn()
        for _ in range(a.runs):
            for k, fn, cnt in legs:
                t = time.perf_counter()
                fn()
                rate[k].append(cnt / (time.perf_counter() - t))
        jpeg.decode_stats(True)
        device()
        bits, groups, rounds, ms = jpeg.decode_stats(False)
        own[name] = rate["device"]
        lines.append("| %s | %.1f | %.0f | %s | %s | %s | %.1f x |" % (
            name, sum(len(s) for s in streams) / 1e6, n * rows * cols * 3 / 1e6, fmt(rate["device"]), fmt(rate["one"]),
            fmt(rate["t16"]), np.median(rate["device"]) / np.median(rate["t16"])))
        stage_lines.append("| %s | %d | %d | %s | %.1f |" % (name, groups, rounds, " | ".join("%.2f" % v for v in ms), sum(ms)))
        del out
    stage_lines[3] = stage_lines[3] % bits
    lines += stage_lines
    if a.libs:
        lines += ["", "## Subsequence lengths", "",
                  "The device leg alone, a fresh process per library; the first row is the library as committed, measured in "
                  "the same way.  images/s, and the rounds of the synchronisation loop.  The rows of this table come from "
                  "processes that run the device leg alone and are faster than the device column of the first table, whose "
                  "passes alternate with Pillow's on the same cores and memory; compare rows of this table with each other "
                  "only.", "",
                  "| bits | " + " | ".join(name.split(",")[0].split(" (")[0] + (" q" + name.split("quality ")[1][:3].strip(",") if "quality" in name else "")
                                           for name, _, _, _ in loads) + " |", "|---|" + "---|" * len(loads)]
        for lib in [oics._lib.LIB_PATH] + list(a.libs):
            print("..", lib, file=sys.stderr, flush=True)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--n", str(a.n), "--runs",
                                str(a.runs)], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("the device leg with %s ended with %d:\n%s" % (lib, p.returncode, p.stderr[-2000:]))
            rows_ = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
            lines.append("| %d | " % rows_[0]["bits"] + " | ".join("%s, %d rounds" % (fmt(r["rate"]), r["rounds"]) for r in rows_) + " |")
    # the flow from files
    lines += ["", "## correct_default from files", "",
              "omr_correct_default_batch_streams (file contents in, file contents out, quality 100) against "
              "omr_correct_default_batch_jpeg with Pillow's decode of the same files to BGR on 16 threads inside the timed "
              "region -- what a caller of the parent commit does.  Sheets/s, alternating passes; the outputs of the two "
              "are compared.", "",
              "| sheets | n | from streams | Pillow on 16 threads + batch_jpeg | streams / parent |", "|---|---|---|---|---|"]
    for (name, streams, rows, cols), n in zip(loads[:2], (a.n, a.a4_sheets)):
        streams = streams[:n]
        print(".. from files:", name, file=sys.stderr, flush=True)

        def from_streams():
            return omr.correct_default_batch_streams(streams, *PARAMS)

        def parent():
            with ThreadPoolExecutor(16) as ex:
                imgs = list(ex.map(pillow_bgr, streams))
            return omr.correct_default_batch_jpeg(imgs, *PARAMS)

        g, w = from_streams(), parent()
        assert g == w and all(t[3] == 0 for t in g), "the two flows differ"
        rate = {"s": [], "p": []}
        for _ in range(a.runs):
            for k, fn in (("s", from_streams), ("p", parent)):
                t = time.perf_counter()
                fn()
                rate[k].append(n / (time.perf_counter() - t))
        lines.append("| %s | %d | %s | %s | %.1f x |" % (name, n, fmt(rate["s"]), fmt(rate["p"]),
                                                        np.median(rate["s"]) / np.median(rate["p"])))
    lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
