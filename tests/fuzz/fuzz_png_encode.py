"""Fuzz of the device PNG encoder (omr_png_encode_batch_device): random shapes, 1 / 3 / 4 channels, content classes, several
images of mixed sizes per call in one slot shape, source bases and pitches aligned and not, compression 0 and 1.  PNG has no
canonical stream, so the arbiters are decoders: Pillow, tests/png_ref.py and the project's own device decoder must return
the image, every chunk's CRC must be right, and the stream must equal the restatement's (tests/png_enc_ref.py).
Usage: python tests/fuzz/fuzz_png_encode.py [cases] [seed]"""
import io
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KINDS = ("noise", "white", "card", "sheet", "repeated row", "constant rows", "four-valued", "gradient", "checkerboard")
_sheet = []


def content(kind, rows, cols, cn, seed=1):
    """one image of a content class: gray [rows, cols] or [rows, cols, cn]"""
    from oics import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = (rows, cols) if cn == 1 else (rows, cols, cn)

    def spread(g):  # a gray plane -> cn channels that differ
        if cn == 1:
            return g
        planes = [g, 255 - g, np.roll(g, 5, 1), np.roll(g, 3, 0)][:cn]
        return np.ascontiguousarray(np.stack(planes, 2))

    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    if kind == "card":
        if cn == 1:
            return synth.make_card(rows, cols, seed)[0].copy()
        bgr = synth.make_color_card(rows, cols, seed)[0]
        return bgr.copy() if cn == 3 else np.ascontiguousarray(np.dstack([bgr, rng.integers(0, 256, (rows, cols), dtype=np.uint8)]))
    if kind == "sheet":
        if not _sheet:
            _sheet.append(np.load(os.path.join(ROOT, "tests", "golden", "dataset_image001.npz"))["gray_small"])
        g = _sheet[0]
        g = np.tile(g, ((rows + g.shape[0] - 1) // g.shape[0], (cols + g.shape[1] - 1) // g.shape[1]))[:rows, :cols]
        return np.ascontiguousarray(spread(g))
    if kind == "repeated row":
        return np.ascontiguousarray(np.broadcast_to(rng.integers(0, 256, (1,) + shape[1:], dtype=np.uint8), shape))
    if kind == "constant rows":
        v = rng.integers(0, 256, (rows,) + (1,) * (len(shape) - 1), dtype=np.uint8)
        return np.ascontiguousarray(np.broadcast_to(v, shape))
    if kind == "four-valued":
        return rng.integers(0, 4, shape, dtype=np.uint8)
    if kind == "gradient":
        return spread((np.add.outer(np.arange(rows) * 3, np.arange(cols) * 2) & 255).astype(np.uint8))
    if kind == "checkerboard":
        return spread(((np.add.outer(np.arange(rows), np.arange(cols)) & 1) * 255).astype(np.uint8))
    raise ValueError(kind)


def encode_on_device(imgs, rows, cols, cn, compression=1, base_offset=0, pitch_pad=0, explicit_sizes=True, fill=0xA5):
    """imgs: host images, each at most rows x cols (None: a 0 x 0 entry) -> (streams, out_len); asserts that nothing is
    written at or behind out_len[i] in slot i (the output is pre-filled with `fill`)."""
    import torch
    from oics import png
    n = len(imgs)
    step = cols * cn + pitch_pad
    stride = rows * step
    host = np.zeros(base_offset + n * stride + 8, np.uint8)
    sizes = np.zeros((n, 2), np.int32)
    for i, im in enumerate(imgs):
        if im is None:
            continue
        r, c = im.shape[:2]
        sizes[i] = (r, c)
        slot = host[base_offset + i * stride: base_offset + (i + 1) * stride].reshape(rows, step)
        slot[:r, :c * cn] = im.reshape(r, c * cn)
    d = torch.from_numpy(host).to("cuda:0")
    bound = png.bound(rows, cols, cn)
    out = torch.full((max(n, 1), bound), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lens = png.encode_batch_device(d.data_ptr() + base_offset, stride, step, rows, cols, cn, sizes if explicit_sizes else None,
                                   n, compression, out.data_ptr(), bound)
    got = out.cpu().numpy()
    streams = []
    for i in range(n):
        L = int(lens[i])
        assert 0 <= L <= bound, "slot %d: length %d above the bound %d" % (i, L, bound)
        assert (got[i, L:] == fill).all(), "slot %d written at or behind out_len" % i
        streams.append(got[i, :L].tobytes())
    return streams, lens


def chunks(stream):
    """[(type, data, crc is right)] of a stream"""
    out, p = [], 8
    while p < len(stream):
        n = struct.unpack(">I", stream[p:p + 4])[0]
        kind, data = stream[p + 4:p + 8], stream[p + 8:p + 8 + n]
        out.append((kind, data, zlib.crc32(kind + data) & 0xffffffff == struct.unpack(">I", stream[p + 8 + n:p + 12 + n])[0]))
        p += 12 + n
    return out


def host_arbiters(stream, img):
    """Pillow, png_ref and the chunk layout on one stream -> None or what is wrong"""
    import png_ref
    from PIL import Image
    cn = 1 if img.ndim == 2 else img.shape[2]
    ch = chunks(stream)
    if stream[:8] != png_ref.SIGNATURE or [c[0] for c in ch] != [b"IHDR", b"IDAT", b"IEND"] or not all(c[2] for c in ch):
        return "chunks %r" % [(c[0], c[2]) for c in ch]
    rows, cols = img.shape[:2]
    if ch[0][1] != struct.pack(">IIBBBBB", cols, rows, 8, {1: 0, 3: 2, 4: 6}[cn], 0, 0, 0):
        return "IHDR"
    z = ch[1][1]
    if z[0] != 0x78 or (z[0] << 8 | z[1]) % 31 or z[1] & 0x20:
        return "zlib header"
    raw = zlib.decompress(z)
    if len(raw) != rows * (1 + cols * cn) or max(raw[::1 + cols * cn]) > 4:
        return "raw data"
    pil = np.asarray(Image.open(io.BytesIO(stream)))
    want = img if cn == 1 else img[..., ::-1] if cn == 3 else img[..., [2, 1, 0, 3]]
    if pil.shape != want.shape or not (pil == want).all():
        return "Pillow's decode differs"
    code, dec = png_ref.decode(stream, 1 if cn == 1 else 3)
    if code != 0 or not (dec == (img if cn < 4 else img[..., :3])).all():
        return "png_ref's decode differs (code %d)" % code
    return None


def device_arbiters(stream, img):
    from oics import png
    cn = 1 if img.ndim == 2 else img.shape[2]
    if png.info(stream) != (img.shape[0], img.shape[1], {1: 0, 3: 2, 4: 6}[cn], 8):
        return "png.info %r" % (png.info(stream),)
    dec = png.decode(stream, 1 if cn == 1 else 3)
    if dec.shape != (img if cn < 4 else img[..., :3]).shape or not (dec == (img if cn < 4 else img[..., :3])).all():
        return "the device decoder's image differs"
    return None


def one_case(rng, restate_below=40000):
    import png_enc_ref
    cn = int(rng.choice([1, 3, 4]))
    rows, cols = int(rng.integers(1, 161)), int(rng.integers(1, 161))
    compression = int(rng.choice([0, 1, 1, 1, 6, 9]))
    n = int(rng.integers(1, 5))
    imgs = []
    for i in range(n):
        r, c = (rows, cols) if i == 0 else (int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1)))
        imgs.append(content(KINDS[int(rng.integers(0, len(KINDS)))], r, c, cn, int(rng.integers(1, 1 << 30))))
    if n > 2 and rng.integers(0, 2):
        imgs[1] = None
    streams, _ = encode_on_device(imgs, rows, cols, cn, compression, base_offset=int(rng.integers(0, 4)),
                                  pitch_pad=int(rng.integers(0, 6)))
    for i, im in enumerate(imgs):
        where = "rows %d cols %d cn %d level %d image %d (%s)" % (rows, cols, cn, compression, i, None if im is None else im.shape)
        if im is None:
            if streams[i] != b"":
                return where + ": a stream for a 0 x 0 entry"
            continue
        err = host_arbiters(streams[i], im) or device_arbiters(streams[i], im)
        if err:
            return where + ": " + err
        if im.size <= restate_below and streams[i] != png_enc_ref.encode(im, compression):
            return where + ": differs from the restatement"
    return None


def run(cases, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in range(cases):
        err = one_case(rng)
        if err:
            return "case %d: %s" % (k, err)
    return None


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    err = run(cases, seed)
    print(err or "fuzz_png_encode: %d cases decode to their images and equal the restatement" % cases)
    sys.exit(1 if err else 0)
