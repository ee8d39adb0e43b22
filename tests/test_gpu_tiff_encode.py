"""The device Group 4 TIFF encoder (omr_tiff_encode_batch_device / omr_tiff_encode) on the GPU: its files equal the
restatement tests/tiff_enc_ref.py byte for byte (whose strips test_tiff_enc_ref.py proves to be libtiff's), Pillow and
omr_tiff_decode read every file back as the thresholded picture, nothing is written at or behind a file's end, and the
Group 4 files libtiff wrote come back strip for strip after a decode on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tiff_cases  # noqa: E402
import tiff_enc_ref as ref  # noqa: E402
import tiff_ref  # noqa: E402
import oics  # noqa: E402
from oics import _lib, tiff, transfer  # noqa: E402
from test_gpu_tiff_decode import decode_on_device  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 257, 2561, 2700)
ROWS = (1, 2, 37, 65, 129)
RPS = (0, 1, 8, 64, 65)
KINDS = tiff_cases.CONTENTS + ("noise",)


def encode_on_device(imgs, rows, cols, cn, threshold=127, rps=0, dpi=0, base_offset=0, pitch_pad=0, explicit_sizes=True, fill=0xA5):
    """imgs: host images, each at most rows x cols (None: a 0 x 0 entry) -> (files, out_len); asserts that nothing is written
    at or behind out_len[i] in slot i (the output is pre-filled with `fill`)."""
    import torch
    n = len(imgs)
    step = cols * cn + pitch_pad
    stride = rows * step
    host = np.full(base_offset + n * stride + 8, 0x5A, np.uint8)
    sizes = np.zeros((n, 2), np.int32)
    for i, im in enumerate(imgs):
        if im is None:
            continue
        r, c = im.shape[:2]
        sizes[i] = (r, c)
        slot = host[base_offset + i * stride: base_offset + (i + 1) * stride].reshape(rows, step)
        slot[:r, :c * cn] = im.reshape(r, c * cn)
    d = torch.from_numpy(host).to("cuda:0")
    bound = tiff.bound(rows, cols, rps)
    out = torch.full((max(n, 1), bound), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lens = tiff.encode_batch_device(d.data_ptr() + base_offset, stride, step, rows, cols, cn, sizes if explicit_sizes else None, n,
                                    out.data_ptr(), bound, threshold, rps, dpi)
    got = out.cpu().numpy()
    files = []
    for i in range(n):
        L = int(lens[i])
        assert 0 <= L <= bound, "slot %d: length %d above the bound %d" % (i, L, bound)
        assert (got[i, L:] == fill).all(), "slot %d written at or behind out_len" % i
        files.append(got[i, :L].tobytes())
    return files, lens


def picture(kind, rows, cols, seed):
    """-> a gray image whose thresholded picture at 127 is the content `kind`, in grays on both sides of the threshold"""
    if kind == "noise":
        bits = (np.random.RandomState(seed).rand(rows, cols) < 0.3).astype(np.uint8)
    else:
        bits = tiff_cases.content(kind, rows, cols, seed=seed)
    g = np.random.RandomState(seed + 1).randint(0, 128, (rows, cols))
    return np.where(bits != 0, g, 255 - g).astype(np.uint8), bits


def read_back(files, pictures, rows, cols):
    """Pillow, and the device decoder where it takes the width, return every thresholded picture"""
    for s, bits in zip(files, pictures):
        assert (tiff_ref.pillow_read(s) == np.where(bits != 0, 0, 255)).all()
    if cols <= tiff_ref.T6_MAX_COLS:
        imgs, size, rc = decode_on_device(files, rows, cols, 1)
        assert (rc == 0).all(), rc
        for im, bits in zip(imgs, pictures):
            assert im.shape == bits.shape and (im == np.where(bits != 0, 0, 255)).all()


@pytest.mark.parametrize("cols", WIDTHS)
def test_every_width_row_count_and_strip_size_equals_the_restatement(cols):
    """per width: one call per RowsPerStrip, its images the five row counts with the contents cycled through them (wide
    rows: contents without noise, to keep the restatement quick)"""
    wide = cols > 257
    rows_set = ROWS
    kinds = tiff_cases.CONTENTS if wide else KINDS
    k = WIDTHS.index(cols)
    for j, rps in enumerate(RPS):
        made = [picture(kinds[(k + j + i) % len(kinds)], r, cols, 100 * k + 10 * j + i) for i, r in enumerate(rows_set)]
        imgs = [m[0] for m in made]
        files, _ = encode_on_device(imgs, max(rows_set), cols, 1, rps=rps, dpi=300 if j & 1 else 0)
        for (img, bits), s in zip(made, files):
            assert s == ref.encode(img, 127, rps, 300 if j & 1 else 0), (cols, img.shape, rps)
        read_back(files, [m[1] for m in made], max(rows_set), cols)


def test_one_row_of_12300_columns():
    img, bits = picture("text", 1, 12300, 5)
    blank = np.full((1, 12300), 255, np.uint8)
    files, _ = encode_on_device([img, blank, 255 - blank], 1, 12300, 1)
    assert files == [ref.encode(img), ref.encode(blank), ref.encode(255 - blank)]
    read_back(files, [bits, np.zeros_like(bits), np.ones_like(bits)], 1, 12300)


@pytest.mark.parametrize("cn", [1, 3])
def test_thresholds_and_the_tie(cn):
    ramp = np.tile(np.arange(256, dtype=np.uint8), (3, 2))[:, 3:500]
    img = ramp if cn == 1 else np.repeat(ramp[..., None], 3, axis=2)  # B = G = R: the gray value is the byte
    for thr in (0, 127, 254):
        (s,), _ = encode_on_device([img], 3, ramp.shape[1], cn, threshold=thr, rps=2)
        assert s == ref.encode(img, thr, 2)
        got = tiff_ref.pillow_read(s)
        assert (got[ramp == thr] == 0).all() and (got[ramp == thr + 1] == 255).all()  # white iff greater than the threshold
        assert (got == np.where(ramp <= thr, 0, 255)).all()
    # a 0 / 255 image encodes to itself at any threshold
    bw = np.where(tiff_cases.content("text", 9, 70, 1) != 0, 0, 255).astype(np.uint8)
    bw = bw if cn == 1 else np.repeat(bw[..., None], 3, axis=2)
    a = [encode_on_device([bw], 9, 70, cn, threshold=t)[0][0] for t in (0, 127, 254)]
    assert a[0] == a[1] == a[2] == ref.encode(bw, 127)


def test_colour_goes_through_the_projects_gray():
    rng = np.random.RandomState(11)
    bgr = rng.randint(100, 156, (37, 65, 3)).astype(np.uint8)  # gray values around the threshold
    gray = transfer.transfer_rgb_image_to_gray_image(bgr).matrix  # the device's own conversion
    assert (gray == ref.gray_of(bgr)).all()
    (a,), _ = encode_on_device([bgr], 37, 65, 3, threshold=127, rps=8)
    (b,), _ = encode_on_device([gray], 37, 65, 1, threshold=127, rps=8)
    assert a == b == ref.encode(bgr, 127, 8)
    assert 0.2 < ref.threshold(bgr, 127).mean() < 0.8


@pytest.mark.parametrize("cn", [1, 3])
def test_source_layouts_give_one_file(cn):
    rng = np.random.RandomState(cn)
    imgs = [rng.randint(0, 256, (37, 67) if cn == 1 else (37, 67, 3)).astype(np.uint8),
            rng.randint(0, 256, (5, 33) if cn == 1 else (5, 33, 3)).astype(np.uint8)]
    want = [ref.encode(im, 127, 8) for im in imgs]
    for off, pad in ((0, 0), (1, 0), (2, 1), (3, 2), (0, 3), (1, 4 - (67 * cn) % 4), (0, 61)):
        got, _ = encode_on_device(imgs, 37, 67, cn, rps=8, base_offset=off, pitch_pad=pad)
        assert got == want, (off, pad)


def test_batches_sizes_and_determinism():
    rows, cols = 40, 70
    pool = [picture(KINDS[i % len(KINDS)], 1 + (7 * i) % rows, 1 + (11 * i) % cols, i + 1)[0] for i in range(70)]
    want = {}
    for n in (1, 3, 70):
        imgs = list(pool[:n])
        if n >= 3:
            imgs[1] = None  # a 0 x 0 entry
        files, lens = encode_on_device(imgs, rows, cols, 1, rps=8)
        for i, (img, s) in enumerate(zip(imgs, files)):
            if img is None:
                assert s == b"" and lens[i] == 0
                continue
            if i not in want:
                want[i] = ref.encode(img, 127, 8)
            assert s == want[i], (n, i)
    full = [picture("text", rows, cols, 3)[0], picture("blobs", rows, cols, 4)[0]]
    a, _ = encode_on_device(full, rows, cols, 1, explicit_sizes=True)
    b, _ = encode_on_device(full, rows, cols, 1, explicit_sizes=False)
    assert a == b == [ref.encode(im) for im in full]
    assert encode_on_device([], rows, cols, 1)[0] == []


def test_host_form_cap_rule_and_stats():
    img, bits = picture("text", 53, 37, 5)
    s = tiff.encode(img, 127, 8, 300)
    assert s == ref.encode(img, 127, 8, 300) == transfer.TransformableMatrix(img).encode_tiff(127, 8, 300)
    assert (tiff.decode(s, 1) == np.where(bits != 0, 0, 255)).all()
    _, im = transfer.as_image(img)
    n = C.c_int64(-7)
    buf = np.full(len(s) + 8, 0xA5, np.uint8)
    L = oics.lib()
    assert L.omr_tiff_encode(C.byref(im), 127, 8, 300, buf.ctypes.data_as(_lib.u8p), len(s) - 1, C.byref(n)) == -4
    assert L.omr_last_error().decode() == "the file takes %d bytes, the buffer holds %d" % (len(s), len(s) - 1)
    assert n.value == len(s) and (buf == 0xA5).all()
    assert L.omr_tiff_encode(C.byref(im), 127, 8, 300, None, 0, C.byref(n)) == -4 and n.value == len(s)
    assert L.omr_tiff_encode(C.byref(im), 127, 8, 300, buf.ctypes.data_as(_lib.u8p), len(s), C.byref(n)) == 0
    assert buf[:len(s)].tobytes() == s and (buf[len(s):] == 0xA5).all()
    tiff.encode_stats(True)
    tiff.encode(img)
    groups, ms = tiff.encode_stats(False)
    assert groups == 1 and len(ms) == len(tiff.STAGES_ENC) and all(v > 0 for v in ms)
    tiff.encode(img)
    assert tiff.encode_stats(False) == (0, [0.0] * 4)


def test_libtiffs_own_files_come_back_strip_for_strip():
    """the Group 4 members of the small cases with Photometric 0: decoded on the device, encoded with the file's
    RowsPerStrip, the strips equal the input's"""
    cases = [(name, s) for name, s in tiff_cases.small_cases() if name.startswith("group4")]
    cases = [(name, s, tiff_ref.parse(s)) for name, s in cases]
    cases = [c for c in cases if c[2]["photometric"] == 0]
    assert len(cases) > 100
    imgs, size, rc = decode_on_device([s for _, s, _ in cases], 40, 260, 1)
    assert (rc == 0).all()
    for rps in sorted({h["rps"] for _, _, h in cases}):
        # RowsPerStrip is per call, and taken as the rows where it is larger: 37 serves the one-strip files of 37 rows only
        sel = [i for i, (_, _, h) in enumerate(cases) if h["rps"] == rps]
        files, _ = encode_on_device([imgs[i] for i in sel], 40, 260, 1, rps=rps)
        for i, f in zip(sel, files):
            assert tiff_ref.strips_of(f) == tiff_ref.strips_of(cases[i][1]), cases[i][0]
