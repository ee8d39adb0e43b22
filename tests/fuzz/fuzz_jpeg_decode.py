"""Fuzz of the device JPEG decoder (omr_jpeg_decode_batch_device) against Pillow (libjpeg-turbo), byte for byte: random
shapes 1..200 x 1..200, content classes (noise, a card, flat, checkerboard, gradient), qualities 1..100, stream variants
(gray, 4:4:4 / 4:2:2 / 4:2:0, optimised tables, restart intervals in blocks and rows), both output forms, several streams
of mixed sizes and variants per call in one slot shape with a pitch, slack bytes checked untouched.
Usage: python tests/fuzz/fuzz_jpeg_decode.py [cases] [seed]"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import fuzz_jpeg  # noqa: E402

VARIANTS = [dict(gray=True), dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, optimize=True),
            dict(gray=True, optimize=True), dict(subsampling=2, restart_marker_blocks=1), dict(subsampling=1, restart_marker_blocks=3),
            dict(subsampling=0, restart_marker_rows=1), dict(gray=True, restart_marker_blocks=3)]


def make_stream(img, quality, gray=False, **kw):
    """Pillow's stream of a BGR (or gray) image; gray=True converts a colour image first"""
    from PIL import Image
    im = Image.fromarray(img[..., ::-1] if img.ndim == 3 else img)
    if gray and img.ndim == 3:
        im = im.convert("L")
    b = io.BytesIO()
    im.save(b, format="JPEG", quality=int(quality), **kw)
    return b.getvalue()


def pillow_decode(stream, channels):
    """the arbiter: (rows, cols) for channels = 1 (libjpeg's JCS_GRAYSCALE for a colour stream), else BGR"""
    from PIL import Image
    im = Image.open(io.BytesIO(stream))
    if channels == 1:
        if im.mode != "L":
            im.draft("L", im.size)
        a = np.asarray(im)
        assert a.ndim == 2
        return a
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def decode_on_device(streams, rows, cols, channels, pitch_pad=0, base_offset=0, fill=0xA5):
    """-> (images, out_size, rc); asserts that every byte of a slot outside its image still holds `fill`"""
    import torch
    from oics import jpeg
    n = len(streams)
    step = cols * channels + pitch_pad
    stride = rows * step + pitch_pad
    out = torch.full((base_offset + max(n, 1) * stride + 8,), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    size, rc = jpeg.decode_batch(streams, channels, out.data_ptr() + base_offset, stride, step, rows, cols)
    got = out.cpu().numpy()
    assert (got[:base_offset] == fill).all() and (got[base_offset + n * stride:] == fill).all()
    imgs = []
    for i in range(n):
        slot = got[base_offset + i * stride: base_offset + (i + 1) * stride]
        body = slot[:rows * step].reshape(rows, step)
        r, c = (int(size[i, 0]), int(size[i, 1])) if rc[i] == 0 else (0, 0)
        mask = np.ones((rows, step), bool)
        mask[:r, :c * channels] = False
        if rc[i] != -215:   # the content of a slot whose entropy data failed is unspecified, inside its image
            assert (body[mask] == fill).all() and (slot[rows * step:] == fill).all(), "slot %d written outside its image" % i
        im = body[:r, :c * channels].copy()
        imgs.append(im.reshape(r, c) if channels == 1 else im.reshape(r, c, 3))
    return imgs, size, rc


def one_case(rng):
    rows, cols = int(rng.integers(1, 201)), int(rng.integers(1, 201))
    channels = int(rng.choice([1, 3]))
    n = int(rng.integers(1, 6))
    streams = []
    for i in range(n):
        r, c = (rows, cols) if i == 0 else (int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1)))
        img = fuzz_jpeg.content(rng, r, c, 3, int(rng.integers(0, 5)))
        q = int(rng.choice([100, 95, 90, 75, 50, 25, 1, int(rng.integers(1, 101))]))
        streams.append(make_stream(img, q, **VARIANTS[int(rng.integers(0, len(VARIANTS)))]))
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
    print(err or "fuzz_jpeg_decode: %d cases identical to Pillow" % cases)
    sys.exit(1 if err else 0)
