"""Fuzz of the device PNG decoder (omr_png_decode_batch_device) against Pillow, byte for byte: random shapes 1..150 x
1..150, every colour type / depth the decoder takes, filter choices per row, contents (noise, flat, ruled), deflate forms
(stored, fixed, dynamic, full flushes, small windows), IDAT cuts, several streams of mixed sizes per call in one slot shape
with a pitch, slack bytes checked untouched.
Usage: python tests/fuzz/fuzz_png_decode.py [cases] [seed]"""
import io
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import png_ref as P  # noqa: E402

DEFLATE_FORMS = [dict(level=0), dict(strategy=zlib.Z_FIXED), dict(), dict(flush_every=150), dict(wbits=9), dict(level=9, wbits=12)]


def pillow_decode(stream, channels):
    """the arbiter: (rows, cols) for channels = 1, else BGR"""
    from PIL import Image
    im = Image.open(io.BytesIO(stream))
    if channels == 1:
        return np.asarray(im.convert("L"))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def decode_on_device(streams, rows, cols, channels, pitch_pad=0, base_offset=0, fill=0xA5):
    """-> (images, out_size, rc); asserts that every byte of a slot outside its image still holds `fill`"""
    import torch
    from oics import png
    n = len(streams)
    step = cols * channels + pitch_pad
    stride = rows * step + pitch_pad
    out = torch.full((base_offset + max(n, 1) * stride + 8,), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    size, rc = png.decode_batch_device(streams, channels, out.data_ptr() + base_offset, stride, step, rows, cols)
    got = out.cpu().numpy()
    assert (got[:base_offset] == fill).all() and (got[base_offset + n * stride:] == fill).all()
    imgs = []
    for i in range(n):
        slot = got[base_offset + i * stride: base_offset + (i + 1) * stride]
        body = slot[:rows * step].reshape(rows, step)
        r, c = (int(size[i, 0]), int(size[i, 1])) if rc[i] == 0 else (0, 0)
        if rc[i] == -215:   # the content of a slot whose data is damaged is unspecified, inside its image
            h = P.parse(streams[i])[1]
            mask = np.ones((rows, step), bool)
            mask[:h.rows, :h.cols * channels] = False
        else:
            mask = np.ones((rows, step), bool)
            mask[:r, :c * channels] = False
        assert (body[mask] == fill).all() and (slot[rows * step:] == fill).all(), "slot %d written outside its image" % i
        im = body[:r, :c * channels].copy()
        imgs.append(im.reshape(r, c) if channels == 1 else im.reshape(r, c, 3))
    return imgs, size, rc


def content(rng, rows, cols, color_type, depth):
    top, n = 1 << depth, P.SAMPLES[color_type]
    shape = (rows, cols) if n == 1 else (rows, cols, n)
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return rng.integers(0, top, shape).astype(np.uint8)
    a = np.full(shape, int(rng.integers(0, top)), np.uint8)
    if kind == 2:
        a[::int(rng.integers(2, 9))] = 0
        a[:, ::int(rng.integers(2, 9))] = top - 1
    return a


def one_case(rng):
    rows, cols = int(rng.integers(1, 151)), int(rng.integers(1, 151))
    channels = int(rng.choice([1, 3]))
    taken = [t for t in P.TAKEN if channels == 3 or t[0] in (0, 4)]
    streams = []
    for i in range(int(rng.integers(1, 6))):
        r, c = (rows, cols) if i == 0 else (int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1)))
        ct, depth = taken[int(rng.integers(0, len(taken)))]
        pal = rng.integers(0, 256, (1 << depth, 3)).astype(np.uint8) if ct == 3 else None
        filters = [int(v) for v in rng.integers(0, 5, r)] if rng.integers(0, 2) else int(rng.integers(0, 5))
        cuts = [None, 1, 100, [0, 3, 0]][int(rng.integers(0, 4))]
        streams.append(P.write(content(rng, r, c, ct, depth), ct, depth, pal, filters=filters, cuts=cuts,
                               **DEFLATE_FORMS[int(rng.integers(0, len(DEFLATE_FORMS)))]))
    imgs, size, rc = decode_on_device(streams, rows, cols, channels, pitch_pad=int(rng.integers(0, 6)),
                                      base_offset=int(rng.integers(0, 4)))
    for i, s in enumerate(streams):
        want = pillow_decode(s, channels)
        if rc[i] != 0 or imgs[i].shape != want.shape or not (imgs[i] == want).all():
            return "rows %d cols %d channels %d stream %d (%s): rc %d" % (rows, cols, channels, i, want.shape, rc[i])
    return None


def run(cases, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in range(cases):
        err = one_case(rng)
        if err:
            return "case %d: %s" % (k, err)
    return None


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    err = run(cases, seed)
    print(err or "fuzz_png_decode: %d cases identical to Pillow" % cases)
    sys.exit(1 if err else 0)
