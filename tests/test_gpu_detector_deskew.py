"""The Hough and FFT deskew flows on the GPU, all parity bit for bit.

  gray    omr_rgb_to_gray_batch_device against the per-call omr_rgb_to_gray_device and against oracle.rgb2gray, 3 and 4
          channels, ragged row ends (cols 1, 3, 5, 61, 64, 67 and 300: two tiles across; 19 rows: two tiles down), packed
          buffers and buffers at odd addresses with pitches that are no multiple of 4 and strides larger than a scan; the
          destination block is compared whole, so every byte outside the gray images must keep its sentinel.
  device  omr_hough_deskew_batch_device / omr_fft_deskew_batch_device on five ruled cards of 150 x 199 at different angles
          and a blank one, 1 and 3 channels: angles as f64 bits against the per-call detector on the per-call gray, the whole
          block of slots against one omr_rotate_device_ex call per scan into an identical block (canvases, and every byte
          outside them), LINEAR + CONTAIN and NEAREST + DEFAULT.  The blank card: rc -215, 0 x 0 and an untouched slot for
          Hough; angle 0.0 and the rotate by 0 for FFT.  The detector parameters (Hough 40 / 5; FFT 30 / 90 / 40 / 5) were
          picked on the CPU oracle so that every ruled card has segments; the first test asserts that on the oracle.
  host    mixed shapes and channel counts in one call, every result at its own index, equal to the per-call triple.
  streams a 4:2:0 JPEG, a gray JPEG, an RGB PNG, a JPEG tagged orientation 6, a progressive JPEG (-213) and a truncated
          file: JPEG outputs byte for byte omr_jpeg_encode of the host form's canvas for omr_imread's decode, PNG outputs
          decode (Pillow) to that canvas, NULL outputs give the same angles."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg_decode as fz  # noqa: E402
import orient_ref as O  # noqa: E402
import png_ref as P  # noqa: E402
from oics import _lib, fft, hough, imread, jpeg, synth, transfer  # noqa: E402

pytestmark = pytest.mark.gpu

L = _lib.lib()
HOUGH = (40.0, 5.0)
FFT = (30.0, 90.0, 40.0, 5.0)
ROWS, COLS = 150, 199
CARDS = [(61, None), (62, 3.0), "blank", (63, -7.0), (64, 20.0), (65, 33.0)]  # (seed, skew); None: the card's own skew
BORDER = (255, 255, 255, 0)
LINEAR, NEAREST, CONTAIN, DEFAULT = 1, 0, 1, 0
_CACHE = {}


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def card(rows, cols, cn, what):
    if what == "blank":
        return np.full((rows, cols) if cn == 1 else (rows, cols, cn), 255, np.uint8)
    return synth.make_card(rows, cols, *what)[0] if cn == 1 else synth.make_color_card(rows, cols, *what)[0]


def to_gray(img):
    return img if img.ndim == 2 else transfer.transfer_rgb_image_to_gray_image(img).matrix


def per_call_angle(which, img):
    """the per-call detector on the per-call gray: the angle, or None where the Hough detector raises for want of a segment"""
    g = to_gray(img)
    if which == "fft":
        return fft.get_angle_with_fft(g, *FFT)
    try:
        return hough.get_angle_with_hough(g, *HOUGH)
    except _lib.OmrError as e:
        assert e.code == -215
        return None


def reference(which, cn):
    """the batch's scans and their per-call angles, once per (detector, channels)"""
    key = (which, cn)
    if key not in _CACHE:
        scans = [card(ROWS, COLS, cn, w) for w in CARDS]
        for a in scans:
            a.setflags(write=False)
        _CACHE[key] = (scans, [per_call_angle(which, s) for s in scans])
    return _CACHE[key]


# ---- the cards have segments (CPU oracle) ------------------------------------------------------------------------------
def test_every_ruled_card_has_segments_on_the_oracle(oracle):
    for cn in (1, 3):
        for w in CARDS:
            img = card(ROWS, COLS, cn, w)
            g = img if cn == 1 else oracle.rgb2gray(img)
            if w == "blank":
                with pytest.raises(RuntimeError):
                    oracle.get_angle_with_hough(g, *HOUGH)
                continue
            assert oracle.get_angle_with_hough(g, *HOUGH)[1] > 0, (cn, w)
    angles = [a for a in reference("hough", 3)[1] if a is not None]
    assert len(angles) == 5 and len(set(angles)) >= 3  # the batch rotates by different angles


# ---- the gray kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [3, 4])
@pytest.mark.parametrize("layout", ["packed", "odd"])
def test_gray_batch_is_the_per_call_conversion(oracle, cn, layout):
    rows, n = 19, 3
    rng = np.random.default_rng(7 + cn)
    for cols in (1, 3, 5, 61, 64, 67, 300):
        odd = layout == "odd"
        sstep = cols * cn + (3 if odd else 0)          # odd: 3 n + 3 and 4 n + 3 -- pitches that are no multiple of 4 for
        if odd and sstep % 4 == 0:                     # every width here but those where it lands on one: one more byte then
            sstep += 1
        sstride = rows * sstep + (13 if odd else 0)
        dstep = cols + (1 if odd else 0)
        if odd and dstep % 4 == 0:
            dstep += 1
        dstride = rows * dstep + (6 if odd else 0)
        sbase, dbase = (1, 3) if odd else (0, 0)
        imgs = rng.integers(0, 256, (n, rows, cols, cn), dtype=np.uint8)
        host = np.full(sbase + n * sstride + 8, 0x5A, np.uint8)
        for i in range(n):
            v = host[sbase + i * sstride: sbase + i * sstride + rows * sstep].reshape(rows, sstep)
            v[:, : cols * cn] = imgs[i].reshape(rows, cols * cn)
        d_src = torch.from_numpy(host).to("cuda:0")
        pattern = torch.full((dbase + n * dstride + 8,), 0xA5, dtype=torch.uint8, device="cuda:0")
        got, want = pattern.clone(), pattern.clone()
        torch.cuda.synchronize()
        transfer.rgb_to_gray_batch(d_src.data_ptr() + sbase, n, sstride, sstep, rows, cols, cn, got.data_ptr() + dbase, dstride, dstep)
        for i in range(n):
            assert L.omr_rgb_to_gray_device(C.c_void_p(d_src.data_ptr() + sbase + i * sstride), sstep, rows, cols, cn,
                                            C.c_void_p(want.data_ptr() + dbase + i * dstride), dstep, None) == 0
        torch.cuda.synchronize()
        got, want = got.cpu().numpy(), want.cpu().numpy()
        assert np.array_equal(got, want), (cols, "the batch differs from the per-call form, or wrote outside an image")
        assert np.array_equal(d_src.cpu().numpy(), host)
        for i in range(n):
            g = got[dbase + i * dstride: dbase + i * dstride + rows * dstep].reshape(rows, dstep)
            assert np.array_equal(g[:, :cols], oracle.rgb2gray(imgs[i])), (cols, i)
            assert (g[:, cols:] == 0xA5).all() and (got[dbase + i * dstride + rows * dstep: dbase + (i + 1) * dstride] == 0xA5).all()
        assert (got[:dbase] == 0xA5).all() and (got[dbase + n * dstride:] == 0xA5).all()


# ---- the device flows ----------------------------------------------------------------------------------------------------
def device_flow(which, scans, cn, flags, clip, odd):
    """-> (angles, rc, n_lines, sizes, the block of slots, the identical block filled by one omr_rotate_device_ex per scan)"""
    n = len(scans)
    row = COLS * cn
    step = row + (3 if odd else 0)
    stride = ROWS * step + (5 if odd else 0)
    base = 1 if odd else 0
    host = np.full(base + n * stride, 0x5A, np.uint8)
    for i, a in enumerate(scans):
        host[base + i * stride: base + i * stride + ROWS * step].reshape(ROWS, step)[:, :row] = a.reshape(ROWS, row)
    d = torch.from_numpy(host).to("cuda:0")
    mr, mc = transfer.detector_deskew_canvas(ROWS, COLS, clip)
    ostep = mc * cn + (5 if odd else 0)
    ostride = mr * ostep + (9 if odd else 0)
    obase = 3 if odd else 0
    pattern = torch.full((obase + n * ostride + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    got, want = pattern.clone(), pattern.clone()
    torch.cuda.synchronize()
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    ang, rc, nl, sizes = mod.deskew_device(d.data_ptr() + base, n, stride, ROWS, COLS, cn, step, *args, flags, 0, BORDER, clip,
                                           got.data_ptr() + obase, ostride, ostep)
    assert np.array_equal(d.cpu().numpy(), host)  # the scans are read-only
    b = (C.c_uint8 * 4)(*BORDER)
    for i in range(n):
        if rc[i] != 0:
            continue
        dr, dc = C.c_int32(), C.c_int32()
        assert L.omr_rotate_size(ROWS, COLS, float(ang[i]), clip, C.byref(dr), C.byref(dc)) == 0
        assert (dr.value, dc.value) == tuple(sizes[i]) and dr.value <= mr and dc.value <= mc
        assert L.omr_rotate_device_ex(C.c_void_p(d.data_ptr() + base + i * stride), step, ROWS, COLS, cn, float(ang[i]), 1.0, flags, 0,
                                      C.cast(b, _lib.u8p), clip, C.c_void_p(want.data_ptr() + obase + i * ostride), ostep, dr.value,
                                      dc.value, None) == 0, L.omr_last_error()
    torch.cuda.synchronize()
    return ang, rc, nl, sizes, got.cpu().numpy(), want.cpu().numpy(), (obase, ostride)


@pytest.mark.parametrize("which", ["hough", "fft"])
@pytest.mark.parametrize("cn,flags,clip,odd", [(3, LINEAR, CONTAIN, True), (1, LINEAR, CONTAIN, False), (3, NEAREST, DEFAULT, False),
                                               (1, NEAREST, DEFAULT, True)])
def test_device_flow_is_the_per_call_chain(which, cn, flags, clip, odd):
    scans, per = reference(which, cn)
    ang, rc, nl, sizes, got, want, (obase, ostride) = device_flow(which, scans, cn, flags, clip, odd)
    blank = CARDS.index("blank")
    for i, e in enumerate(per):
        if e is None:
            assert which == "hough" and i == blank
            assert rc[i] == -215 and bits(ang[i]) == 0 and nl[i] == 0 and tuple(sizes[i]) == (0, 0)
            assert (got[obase + i * ostride: obase + (i + 1) * ostride] == 0xA5).all(), "the slot of a scan without a segment was written"
        else:
            assert rc[i] == 0 and bits(ang[i]) == bits(e), (i, ang[i], e)
            assert i == blank or nl[i] > 0
    if which == "fft":  # no segment: angle 0.0, a success, and the rotate by 0
        assert bits(ang[blank]) == 0 and nl[blank] == 0 and rc[blank] == 0 and tuple(sizes[blank]) == (ROWS, COLS)
    # canvases byte for byte omr_rotate_device_ex's, and every byte of the block outside them as it was
    assert np.array_equal(got, want)
    assert (got != 0xA5).any()


# ---- host images ---------------------------------------------------------------------------------------------------------
MIXED = [(150, 199, 3, (61, None)), (120, 90, 1, (71, 5.0)), (150, 199, 1, (62, 3.0)), (120, 90, 3, (72, -4.0)), (150, 199, 3, "blank"),
         (150, 199, 3, (64, 20.0)), (120, 90, 1, (73, 12.0))]


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_host_form_mixed_shapes_equal_the_per_call_triple(which):
    imgs = [card(r, c, cn, w) for r, c, cn, w in MIXED]
    if which == "hough":
        ang, rc, out = hough.deskew(imgs, *HOUGH, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN)
    else:
        ang, out = fft.deskew(imgs, *FFT, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN)
        rc = np.zeros(len(imgs), np.int32)
    seen = 0
    for i, img in enumerate(imgs):
        e = per_call_angle(which, img)
        if e is None:
            assert MIXED[i][3] == "blank" and rc[i] == -215 and bits(ang[i]) == 0 and out[i] is None
            continue
        seen += 1
        assert rc[i] == 0 and bits(ang[i]) == bits(e), (i, ang[i], e)
        want = transfer.rotate_mat(img, e, 1.0, LINEAR, 0, BORDER, CONTAIN).matrix
        assert out[i].shape == want.shape and np.array_equal(out[i], want), i
    assert seen >= len(imgs) - 1


# ---- file contents -------------------------------------------------------------------------------------------------------
def _files():
    """[(stream, channels the decode has, scan_rc expected)]: one bucket of 120 x 90 after imread's turn, and two refusals"""
    if "files" not in _CACHE:
        tall = [synth.make_color_card(120, 90, 80 + i, s)[0] for i, s in enumerate((4.0, -6.0, 9.0))]
        wide = synth.make_color_card(90, 120, 84, 3.0)[0]
        good = fz.make_stream(tall[0], 95, subsampling=2)
        _CACHE["files"] = [(good, 0), (fz.make_stream(tall[1], 100, gray=True), 0),
                           (P.write(np.ascontiguousarray(tall[2][..., ::-1]), 2, 8), 0),
                           (O.tag_jpeg(fz.make_stream(wide, 95, subsampling=2), 6), 0),
                           (fz.make_stream(tall[0], 90, progressive=True), -213), (good[: len(good) // 2], None)]
    return _CACHE["files"]


@pytest.mark.parametrize("which", ["hough", "fft"])
def test_streams_form_equals_the_host_form_on_imreads_decode(which):
    from PIL import Image
    files = _files()
    streams = [s for s, _ in files]
    mod, args = (hough, HOUGH) if which == "hough" else (fft, FFT)
    ang, rc, out = mod.deskew_streams(streams, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN, level=95)
    assert rc[4] == -213 and out[4] is None and ang[4] == 0.0          # progressive: the decoder's refusal stays
    assert rc[5] == -215 and out[5] is None and ang[5] == 0.0          # cut in the middle of its entropy data
    imgs = [imread.decode(s, 3) for s in streams[:4]]
    assert [im.shape for im in imgs] == [(120, 90, 3)] * 4             # the tagged sheet counts by its turned shape
    h = mod.deskew(imgs, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN)
    h_ang, h_img = h[0], h[-1]
    made = 0
    for i in range(4):
        assert bits(ang[i]) == bits(h_ang[i]), (i, ang[i], h_ang[i])
        if h_img[i] is None:
            assert which == "hough" and rc[i] == -215 and out[i] is None
            continue
        made += 1
        assert rc[i] == 0 and out[i] == jpeg.encode(h_img[i], 95), (i, "the output streams differ")
    assert made >= 3
    a_png, rc_png, out_png = mod.deskew_streams(streams, *args, flags=LINEAR, border_value=BORDER, clip_strategy=CONTAIN, png=True, level=1)
    assert list(rc_png) == list(rc) and (bits(a_png) == bits(ang)).all()
    for i in range(4):
        if h_img[i] is not None:
            back = np.asarray(Image.open(io.BytesIO(out_png[i])).convert("RGB"))[..., ::-1]
            assert back.shape == h_img[i].shape and (back == h_img[i]).all(), i
    a2, rc2, none = mod.deskew_streams(streams, *args, want_out=False)   # NULL out: the angles alone
    assert none is None and list(rc2) == list(rc) and (bits(a2) == bits(ang)).all()
    # the gray form: the Y plane through the same doors
    g_streams = streams[:2] + streams[3:4]
    a1, rc1, out1 = mod.deskew_streams(g_streams, *args, flags=LINEAR, border_value=(255,) * 4, clip_strategy=CONTAIN, channels=1, level=95)
    g_imgs = [imread.decode(s, 1) for s in g_streams]
    g = mod.deskew(g_imgs, *args, flags=LINEAR, border_value=(255,) * 4, clip_strategy=CONTAIN)
    for i in range(3):
        assert bits(a1[i]) == bits(g[0][i]), i
        assert (out1[i] is None) == (g[-1][i] is None) and (out1[i] is None or out1[i] == jpeg.encode(g[-1][i], 95)), i
