"""The device 8-bit TIFF encoder (omr_tiff8_encode_batch_device / omr_tiff8_encode) on the GPU.  Every file is checked three
ways: it equals the restatement tests/tiff8_enc_ref.py byte for byte (which test_tiff8_enc_ref.py proves readable), Pillow's
libtiff decodes it to the canvas, and omr_tiff_decode_batch_device decodes it to the canvas, gray and BGR.  Nothing is
written at or behind a file's end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tiff8_enc_ref as ref  # noqa: E402
import tiff8_ref  # noqa: E402
import oics  # noqa: E402
from oics import _lib, tiff, transfer  # noqa: E402
from test_gpu_tiff_decode import decode_on_device  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)
ROWS = (1, 2, 7)
RPS = (0, 1, 2, 6, 7, 12)  # 0, 1, rows and rows + 5 for every member of ROWS
MODES = ((1, 1), (5, 1), (5, 2))  # (compression, predictor)
_WANT = {}


def want(img, comp, pred, rps, dpi=0):
    """the restatement's file, computed once per picture and parameters"""
    key = (img.shape, img.tobytes(), comp, pred, rps, dpi)
    if key not in _WANT:
        _WANT[key] = ref.encode(img, comp, pred, rps, dpi)
    return _WANT[key]


def encode_on_device(imgs, rows, cols, cn, comp=5, pred=1, rps=0, dpi=0, base_offset=0, pitch_pad=0, explicit_sizes=True, fill=0xA5):
    """imgs: host images, each at most rows x cols (None: a 0 x 0 entry) -> (files, out_len); asserts that nothing is written
    at or behind out_len[i] in slot i (the output is pre-filled with `fill`)"""
    import torch
    n = len(imgs)
    step = cols * cn + pitch_pad
    stride = rows * step
    host = np.full(base_offset + n * stride + 8, 0x5A, np.uint8)
    sizes = np.zeros((n, 2), np.int32)
    bound = tiff.bound8(rows, cols, cn, comp, rps)
    for i, im in enumerate(imgs):
        if im is None:
            continue
        r, c = im.shape[:2]
        sizes[i] = (r, c)
        bound = max(bound, tiff.bound8(r, c, cn, comp, rps))
        slot = host[base_offset + i * stride: base_offset + (i + 1) * stride].reshape(rows, step)
        slot[:r, :c * cn] = im.reshape(r, c * cn)
    d = torch.from_numpy(host).to("cuda:0")
    out = torch.full((max(n, 1), bound), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lens = tiff.encode8_batch_device(d.data_ptr() + base_offset, stride, step, rows, cols, cn, sizes if explicit_sizes else None, n,
                                     out.data_ptr(), bound, comp, pred, rps, dpi)
    got = out.cpu().numpy()
    files = []
    for i in range(n):
        L = int(lens[i])
        assert 0 <= L <= bound, "slot %d: length %d above the bound %d" % (i, L, bound)
        assert (got[i, L:] == fill).all(), "slot %d written at or behind out_len" % i
        files.append(got[i, :L].tobytes())
    return files, lens


def read_back(files, imgs, rows, cols, cn):
    """Pillow and the device decoder return every canvas (the decoder: gray for gray files, BGR for RGB ones)"""
    for s, im in zip(files, imgs):
        assert (tiff8_ref.pillow_read(s) == (im if cn == 1 else im[..., ::-1])).all()
    got, size, rc = decode_on_device(files, rows, cols, cn)
    assert (rc == 0).all(), rc
    for g, im in zip(got, imgs):
        assert g.shape == im.shape and (g == im).all()


def three_ways(imgs, rows, cols, cn, comp, pred, rps, dpi=0, **kw):
    files, _ = encode_on_device(imgs, rows, cols, cn, comp, pred, rps, dpi, **kw)
    for im, s in zip(imgs, files):
        assert s == want(im, comp, pred, rps, dpi), (im.shape, comp, pred, rps)
    read_back(files, imgs, rows, cols, cn)
    return files


def noise(rows, cols, cn, seed):
    return tiff8_ref.content("noise", rows, cols, 1 if cn == 1 else 3, seed)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("cols", WIDTHS)
def test_every_width_row_count_strip_size_and_mode(cols, cn):
    kinds = ("noise", "text", "gradient")
    k = WIDTHS.index(cols)
    files, imgs = [], []
    for m, (comp, pred) in enumerate(MODES):
        for j, rps in enumerate(RPS):
            batch = [tiff8_ref.content(kinds[(k + j + i) % 3], r, cols, 1 if cn == 1 else 3, 100 * k + 10 * j + i) for i, r in enumerate(ROWS)]
            dpi = 300 if (j + m) & 1 else 0
            got, _ = encode_on_device(batch, max(ROWS), cols, cn, comp, pred, rps, dpi)
            for im, s in zip(batch, got):
                assert s == want(im, comp, pred, rps, dpi), (cols, cn, im.shape, comp, pred, rps)
            files += got
            imgs += batch
    read_back(files, imgs, max(ROWS), cols, cn)


def test_code_widths_switch_at_254_766_and_1790():
    """one-row gray strips of noise without a repeated pair: n bytes give exactly n codes and EOI at index n, so the strips
    stand just under, at and just over every switch"""
    raw = ref.pairless_noise(1800, 7)
    sizes = [n for lo in (250, 762, 1786) for n in range(lo, lo + 11)]
    for lo, edge in ((250, 254), (762, 766), (1786, 1790)):
        counts = [ref.code_counts(raw[:n].tobytes())[0] for n in range(lo, lo + 11)]
        assert counts == list(range(lo, lo + 11)) and {edge - 1, edge, edge + 1} <= set(counts)
    imgs = [raw[:n].reshape(1, n).copy() for n in sizes]
    three_ways(imgs, 1, max(sizes), 1, 5, 1, 1)


def test_the_full_table_and_strips_that_end_around_a_clear():
    page = noise(64, 256, 1, 3)
    raw = page.tobytes()
    codes = ref.lzw_codes(raw)
    assert sum(1 for c, i in codes[1:] if c == ref.CLEAR) >= 3 and all(i == ref.CLEAR_AT for c, i in codes[1:] if c == ref.CLEAR)
    three_ways([page], 64, 256, 1, 5, 1, 64)
    # the strip's last match has index 3835, so that Clear and a 9-bit EOI end it; one byte less and one more
    n = next(n for n in range(3000, len(raw)) if ref.lzw_codes(raw[:n])[-2:] == [(ref.CLEAR, ref.CLEAR_AT), (ref.EOI, 0)])
    imgs = [np.frombuffer(raw[:m], np.uint8).reshape(1, m).copy() for m in (n - 1, n, n + 1)]
    three_ways(imgs, 1, n + 1, 1, 5, 1, 1)
    # long entries: a constant strip (KwKwK chains), a period-2 and a period-3 page
    flat = np.arange(64 * 256)
    pages = [np.full((64, 256), 200, np.uint8), ((flat % 2) * 255).astype(np.uint8).reshape(64, 256), (flat % 3 + 1).astype(np.uint8).reshape(64, 256)]
    three_ways(pages, 64, 256, 1, 5, 1, 64)
    three_ways(pages, 64, 256, 1, 5, 2, 64)


@pytest.mark.parametrize("cn", [1, 3])
def test_predictor_pictures(cn):
    ramp = np.tile(np.arange(256, dtype=np.uint8), (3, 2))[:, 3:500]
    stripes = np.tile(np.array([0, 255], np.uint8), (3, 249))[:, :497]  # 0 - 255 wraps to 1
    if cn == 3:
        ramp = np.stack([ramp, 255 - ramp, ramp // 2], axis=2)
        stripes = np.stack([stripes, 255 - stripes, stripes], axis=2)
    imgs = [np.ascontiguousarray(ramp), np.ascontiguousarray(stripes)]
    if cn == 3:
        one_flat = noise(3, 497, 3, 5)
        one_flat[..., 1] = 77  # per sample, not per byte: G's differences are a run of zeros
        imgs.append(one_flat)
        d = np.frombuffer(ref.raw_strips(one_flat, 2, 3)[0][0], np.uint8).reshape(3, 497, 3)
        assert (d[:, 1:, 1] == 0).all()
    for rps in (0, 2):
        three_ways(imgs, 3, 497, cn, 5, 2, rps)


@pytest.mark.parametrize("cn", [1, 3])
def test_source_layouts_give_one_file(cn):
    imgs = [noise(37, 67, cn, cn), tiff8_ref.content("text", 5, 33, 1 if cn == 1 else 3, 2)]
    for comp, pred in MODES:
        expect = [want(im, comp, pred, 8) for im in imgs]
        for off, pad in ((0, 0), (1, 0), (2, 1), (3, 2), (0, 3), (1, 4 - (67 * cn) % 4), (0, 61)):
            got, _ = encode_on_device(imgs, 37, 67, cn, comp, pred, 8, base_offset=off, pitch_pad=pad)
            assert got == expect, (comp, pred, off, pad)
        read_back(expect, imgs, 37, 67, cn)
    full = [noise(37, 67, cn, 9), noise(37, 67, cn, 10)]
    a, _ = encode_on_device(full, 37, 67, cn, explicit_sizes=True)
    b, _ = encode_on_device(full, 37, 67, cn, explicit_sizes=False)
    assert a == b == [want(im, 5, 1, 0) for im in full]
    read_back(a, full, 37, 67, cn)


@pytest.mark.parametrize("mode", MODES)
def test_batches_of_mixed_sizes_and_determinism(mode):
    comp, pred = mode
    rows, cols = 40, 70
    kinds = ("noise", "text", "gradient", "constant", "period2")
    pool = [tiff8_ref.content(kinds[i % 5], 1 + (7 * i) % rows, 1 + (11 * i) % cols, 1, i + 1) for i in range(67)]
    for n in (1, 2, 67):
        imgs = list(pool[:n])
        if n >= 2:
            imgs[1] = None  # a 0 x 0 entry
        if n > 60:
            imgs[60] = None
        files, lens = encode_on_device(imgs, rows, cols, 1, comp, pred, 0)
        for i, (img, s) in enumerate(zip(imgs, files)):
            if img is None:
                assert s == b"" and lens[i] == 0
            else:
                assert s == want(img, comp, pred, 0), (n, i)
        kept = [(s, im) for s, im in zip(files, imgs) if im is not None]
        read_back([s for s, _ in kept], [im for _, im in kept], rows, cols, 1)
    # alone and at another place of another batch
    moved = [pool[5], None, pool[0], pool[5]]
    files, _ = encode_on_device(moved, rows, cols, 1, comp, pred, 0)
    assert files[0] == files[3] == want(pool[5], comp, pred, 0) and files[2] == want(pool[0], comp, pred, 0)
    kept = [(s, im) for s, im in zip(files, moved) if im is not None]
    read_back([s for s, _ in kept], [im for _, im in kept], rows, cols, 1)
    assert encode_on_device([], rows, cols, 1, comp, pred)[0] == []


def test_host_form_cap_rule_and_stats():
    img = tiff8_ref.content("text", 53, 37, 3, 5)
    s = tiff.encode8(img, 5, 2, 8, 300)
    assert s == want(img, 5, 2, 8, 300) == transfer.TransformableMatrix(img).encode_tiff8(5, 2, 8, 300)
    assert (tiff.decode(s, 3) == img).all()
    gray = noise(200, 300, 1, 1)  # noise: LZW passes the first buffer, the second call takes the length
    assert tiff.encode8(gray) == want(gray, 5, 1, 0) and tiff.encode8(gray, 1) == want(gray, 1, 1, 0)
    _, im = transfer.as_image(img)
    n = C.c_int64(-7)
    buf = np.full(len(s) + 8, 0xA5, np.uint8)
    L = oics.lib()
    assert L.omr_tiff8_encode(C.byref(im), 5, 2, 8, 300, buf.ctypes.data_as(_lib.u8p), len(s) - 1, C.byref(n)) == -4
    assert L.omr_last_error().decode() == "the file takes %d bytes, the buffer holds %d" % (len(s), len(s) - 1)
    assert n.value == len(s) and (buf == 0xA5).all()
    assert L.omr_tiff8_encode(C.byref(im), 5, 2, 8, 300, None, 0, C.byref(n)) == -4 and n.value == len(s)
    assert L.omr_tiff8_encode(C.byref(im), 5, 2, 8, 300, buf.ctypes.data_as(_lib.u8p), len(s), C.byref(n)) == 0
    assert buf[:len(s)].tobytes() == s and (buf[len(s):] == 0xA5).all()
    tiff.encode8_stats(True)
    tiff.encode8(img)
    groups, ms = tiff.encode8_stats(False)
    assert groups == 1 and len(ms) == len(tiff.STAGES_ENC8) and all(v > 0 for v in ms)
    tiff.encode8(img)
    assert tiff.encode8_stats(False) == (0, [0.0] * 4)
