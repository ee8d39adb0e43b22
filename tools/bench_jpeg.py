"""The device JPEG encoder (development aid): images/s and MB per stream of omr_jpeg_encode_batch_device on resident
colour canvases (A4 synthetic cards; the dataset's 1150 x 1240 sheets, tests/golden/dataset) against Pillow (libjpeg-turbo)
-- one thread, and 16 host threads on BGR views and on contiguous RGB copies made beforehand -- and
omr_correct_default_batch_jpeg against the two flows that gave the same files before it: omr_correct_default_batch +
Pillow on 16 threads, and the per-call loop on 16 threads + Pillow.
Usage: python tools/bench_jpeg.py [encoder|composite|all] [--n N] [--runs R]
Prints one line per measurement; every timed call is preceded by an untimed one of the same kind."""
import argparse
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

PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)


def pillow(img, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img[..., ::-1]).save(b, format="JPEG", quality=q)
    return b.getvalue()


def pillow_rgb(rgb, q):
    """contiguous RGB in: nothing but Pillow's own encode is timed"""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format="JPEG", quality=q)
    return b.getvalue()


def dataset_sheets():
    """the reference's 104 test sheets as imread(IMREAD_COLOR) gives them (gray JPEGs -> three equal channels)"""
    from PIL import Image
    d = os.path.join(ROOT, "tests", "golden", "dataset")
    out = []
    for f in sorted(os.listdir(d)):
        if f.lower().endswith(".jpg"):
            g = np.array(Image.open(os.path.join(d, f)).convert("L"))
            out.append(np.ascontiguousarray(np.stack([g, g, g], axis=2)))
    return out


def pillow_16(imgs, q):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda a: pillow(a, q), imgs))


def timed(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return out


def encoder_set(name, distinct, n, runs):
    import torch
    from oics import jpeg
    rows, cols = distinct[0].shape[:2]
    k = len(distinct)
    host = np.stack([distinct[i % k] for i in range(n)])
    d = torch.from_numpy(host).to("cuda:0")
    bound = jpeg.bound(rows, cols, 3)
    out = torch.empty((n, bound), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    some = [distinct[i % k] for i in range(32)]
    rgb = [np.ascontiguousarray(a[..., ::-1]) for a in some]
    for q in (100, 95):
        lens = [None]

        def run():
            lens[0] = jpeg.encode_batch_device(d.data_ptr(), rows * cols * 3, cols * 3, rows, cols, 3, None, n, q, out.data_ptr(), bound)
        ts = timed(run, runs)
        first = bytes(out[0, : int(lens[0][0])].cpu().numpy())
        assert first == pillow(distinct[0], q), "stream differs from Pillow"
        print("encoder  %-14s q %3d  n %d: %s images/s  (%.2f MB per stream)" % (
            name, q, n, " / ".join("%.0f" % (n / t) for t in ts), lens[0].mean() / 1e6))
        t1 = timed(lambda: [pillow_rgb(a, q) for a in rgb[:4]], runs)
        print("pillow   1 thread, contiguous RGB      q %3d: %s images/s" % (q, " / ".join("%.1f" % (4 / t) for t in t1)))
        tp = timed(lambda: pillow_16(some, q), runs)
        print("pillow   16 threads, BGR views         q %3d: %s images/s" % (q, " / ".join("%.1f" % (32 / t) for t in tp)))

        def rgb16():
            with ThreadPoolExecutor(16) as ex:
                return list(ex.map(lambda a: pillow_rgb(a, q), rgb))
        tr = timed(rgb16, runs)
        print("pillow   16 threads, contiguous RGB    q %3d: %s images/s" % (q, " / ".join("%.1f" % (32 / t) for t in tr)))
    del d, out
    torch.cuda.empty_cache()


def encoder(n, runs):
    from oics import synth
    cards = [synth.make_color_card(3508, 2480, 50 + i, skew=0.7 * i - 2)[0] for i in range(8)]
    encoder_set("A4 cards", cards, n, runs)
    data = [a for a in dataset_sheets() if a.shape == (1150, 1240, 3)]  # the resident batch is one slot shape
    encoder_set("dataset sheets", data, n, runs)


def composite(n, runs):
    from oics import omr, synth
    data = dataset_sheets()
    a4 = [synth.make_color_card(3508, 2480, 900 + i, skew=[2.0, -4.5, 7.25, -0.4][i % 4])[0] for i in range(8)]
    for name, pool, m in (("dataset sheets (four shapes)", data, n), ("A4 cards 3508x2480", a4, max(n // 4, 16))):
        rows, cols = pool[0].shape[:2]
        sheets = [pool[i % len(pool)] for i in range(m)]

        def new():
            return omr.correct_default_batch_jpeg(sheets, *PARAMS, quality=100)

        def parent():
            res = omr.correct_default_batch(sheets, *PARAMS)
            return pillow_16([r[2] for r in res if r[2] is not None], 100)

        def one(sheet):
            try:
                return pillow(omr.correct_default(sheet, *PARAMS)[2], 100)
            except Exception:  # a sheet the function fails on has no file in any of the flows
                return None

        def per_call():
            with ThreadPoolExecutor(16) as ex:
                return list(ex.map(one, sheets))
        a = new()
        b = parent()
        assert [x[2] for x in a if x[2] is not None] == b, "streams differ from batch + Pillow"
        rates = {"batch_jpeg": [], "batch + pillow16": [], "per-call16 + pillow": []}
        for _ in range(runs):  # alternating
            for kind, fn in (("batch_jpeg", new), ("batch + pillow16", parent), ("per-call16 + pillow", per_call)):
                t = time.perf_counter()
                fn()
                rates[kind].append(m / (time.perf_counter() - t))
        for kind, r in rates.items():
            print("composite %s n %d  %-20s %s sheets/s" % (name, m, kind, " / ".join("%.1f" % x for x in r)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    if a.what in ("encoder", "all"):
        encoder(a.n, a.runs)
    if a.what in ("composite", "all"):
        composite(a.n, a.runs)
