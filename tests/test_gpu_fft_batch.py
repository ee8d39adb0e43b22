"""omr_fft_angles_batch_device / omr_get_angles_with_fft_batch / omr_fourier_transform_batch_device on the GPU.  All
parity is bit for bit, against two yardsticks: the per-call entry points (angle bits, segment counts, pictures byte for
byte), and the CPU oracle's Canny -> HoughLinesP(threshold 100) -> fft.rs vote and tests/lined_ref.py run on the GPU's
OWN log picture (the spectrum pictures agree with the CPU restatement only to one grey level, so the oracle's chain on
the oracle's picture finds other segments: tests/test_gpu_fft.py).

Shapes: 256 x 320 (a power of two and a mixed-radix axis), 300 x 420 (mixed radix both ways) and 75 x 100 (too small for
a line of 100 votes: no scan of it has a segment).  Batches of 11 scans run one full launch group of 8 and a short one of
3; the 256 x 320 batch holds one all-zero scan.  The tests assert the mix they need from the segment counts."""
import ctypes as C

import numpy as np
import pytest
import torch

import lined_ref as lr
from oics import _lib, fft, hough, omr, synth
from oracle import oracle_fft as offt

pytestmark = pytest.mark.gpu

PARAMS = {"p1": (50.0, 150.0, 100.0, 15.0), "p2": (30.0, 90.0, 40.0, 5.0)}  # as tests/test_gpu_fft.py
SHAPES = {"pow2": (256, 320), "mixed": (300, 420), "small": (75, 100)}
N = 11
SEED0 = {"pow2": 2, "mixed": 9, "small": 3}
ZERO_AT = 5  # the all-zero scan's place inside the 256 x 320 batch


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


_SCANS, _REF, _DEV = {}, {}, {}


def scans_of(shape):
    """the batch's scans with their per-call log pictures, computed once per shape"""
    if shape not in _SCANS:
        rows, cols = SHAPES[shape]
        scans = [synth.make_card(rows, cols, SEED0[shape] + i)[0] for i in range(N)]
        if shape == "pow2":
            scans[ZERO_AT] = np.zeros((rows, cols), np.uint8)
        logs = [fft.get_fft_image(a)[1] for a in scans]
        for a in scans + logs:
            a.setflags(write=False)
        _SCANS[shape] = (scans, logs)
    return _SCANS[shape]


def reference(shape, pset):
    """per scan the per-call answer (angle, picture, segment count), once per (shape, parameters)"""
    if (shape, pset) not in _REF:
        c1, c2, mll, mlg = PARAMS[pset]
        scans, logs = scans_of(shape)
        per = []
        for img, lg in zip(scans, logs):
            ang, pic = fft.get_angle_with_fft(img, c1, c2, mll, mlg, want_picture=True)
            assert bits(fft.get_angle_with_fft(img, c1, c2, mll, mlg)) == bits(ang)
            count = len(hough.hough_lines_p(hough.canny(lg, c1, c2), 1.0, np.pi / 180.0, 100, mll, mlg))
            pic.setflags(write=False)
            per.append((ang, pic, count))
        _REF[(shape, pset)] = per
    return _REF[(shape, pset)]


def assert_mix(shape, per):
    """a batch cannot pass with every scan empty, nor without a scan whose vote has something to choose from"""
    counts = [p[2] for p in per]
    if shape == "small":
        assert counts == [0] * len(per), counts
        return
    assert any(c >= 2 and a != 0.0 for a, _, c in per), [(a, c) for a, _, c in per]
    if shape == "pow2":
        assert counts[ZERO_AT] == 0, counts


def run_device(scans, pset, pictures, odd_layout=True):
    """the device form on `scans` (one shape); returns angles, n_lines and the whole picture buffer with its layout"""
    n = len(scans)
    rows, cols = scans[0].shape
    step = cols + (3 if odd_layout else 0)
    stride = rows * step + (5 if odd_layout else 0)
    base = 1 if odd_layout else 0
    host = np.full(base + n * stride, 0x5A, np.uint8)
    for i, a in enumerate(scans):
        host[base + i * stride: base + i * stride + rows * step].reshape(rows, step)[:, :cols] = a
    d = torch.from_numpy(host).to("cuda:0")
    lstep = 3 * cols + (4 if odd_layout else 0)
    lstride = rows * lstep + (7 if odd_layout else 0)
    lbase = 3 if odd_layout else 0
    out = torch.full((lbase + n * lstride + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ang, nl = fft.fft_angles_batch_device(d.data_ptr() + base, n, stride, rows, cols, step, *PARAMS[pset],
                                          d_lined=out.data_ptr() + lbase if pictures else None, lined_stride_bytes=lstride,
                                          lined_step=lstep)
    assert np.array_equal(d.cpu().numpy(), host)  # the scans are read-only
    return ang, nl, out.cpu().numpy(), (lbase, lstride, lstep)


def device_result(shape, pset):
    """the device form with pictures in the odd layout, once per (shape, parameters)"""
    if (shape, pset) not in _DEV:
        _DEV[(shape, pset)] = run_device(scans_of(shape)[0], pset, True)
    return _DEV[(shape, pset)]


def pictures_of(out, layout, n, rows, cols):
    """the n pictures of a buffer, after checking that every byte outside them kept its sentinel"""
    lbase, lstride, lstep = layout
    assert (out[:lbase] == 0xA5).all() and (out[lbase + n * lstride:] == 0xA5).all()
    pics = []
    for i in range(n):
        slot = out[lbase + i * lstride: lbase + (i + 1) * lstride]
        pic = slot[: rows * lstep].reshape(rows, lstep)
        assert (pic[:, 3 * cols:] == 0xA5).all() and (slot[rows * lstep:] == 0xA5).all(), i
        pics.append(pic[:, : 3 * cols].reshape(rows, cols, 3))
    return pics


CASES = [(s, p) for s in SHAPES for p in PARAMS]


@pytest.mark.parametrize("shape,pset", CASES)
def test_device_form_is_the_per_call_form(shape, pset):
    scans, _ = scans_of(shape)
    rows, cols = SHAPES[shape]
    per = reference(shape, pset)
    assert_mix(shape, per)
    ang, nl, out, layout = device_result(shape, pset)
    assert nl.tolist() == [p[2] for p in per]
    for i, (e_ang, e_pic, count) in enumerate(per):
        assert bits(ang[i]) == bits(e_ang), (i, ang[i], e_ang, count)
    for i, pic in enumerate(pictures_of(out, layout, N, rows, cols)):  # every slot is written, the bare edges included
        assert np.array_equal(pic, per[i][1]), (i, per[i][2])
    # without pictures the angles are the same, and nothing is written
    ang2, nl2, out2, _ = run_device(scans, pset, False)
    assert (bits(ang2) == bits(ang)).all() and nl2.tolist() == nl.tolist() and (out2 == 0xA5).all()


def test_the_mix_of_scans_is_what_the_tests_need():
    """both parameter sets on both larger shapes: a scan with two or more segments and an angle other than 0.0; the
    all-zero scan and every 75 x 100 scan without a segment, angle 0.0 and the bare GRAY2BGR picture"""
    for shape, pset in CASES:
        per = reference(shape, pset)
        assert_mix(shape, per)
        empty = [i for i, p in enumerate(per) if p[2] == 0]
        if shape != "mixed":
            assert empty
        for i in empty:
            ang, pic, _ = per[i]
            assert bits(ang) == 0
            assert (pic[:, :, 0] == pic[:, :, 1]).all() and (pic[:, :, 0] == pic[:, :, 2]).all()  # no segment drawn
            assert set(np.unique(pic).tolist()) <= {0, 255}
    assert (reference("pow2", "p1")[ZERO_AT][1] == 0).all()


@pytest.mark.parametrize("shape,pset", CASES)
def test_against_the_oracle_chain_on_the_gpus_log_picture(oracle, shape, pset):
    c1, c2, mll, mlg = PARAMS[pset]
    scans, _ = scans_of(shape)
    rows, cols = SHAPES[shape]
    d = torch.from_numpy(np.stack(scans)).to("cuda:0")
    logs = torch.zeros((N, rows, cols), dtype=torch.uint8, device="cuda:0")
    fft.fft_image_batch_device(d.data_ptr(), N, rows * cols, rows, cols, cols, logs.data_ptr())
    logs = logs.cpu().numpy()
    ang, nl, out, layout = device_result(shape, pset)
    pics = pictures_of(out, layout, N, rows, cols)
    for i in range(N):
        edges = oracle.canny(logs[i], c1, c2)
        lines = oracle.hough_lines_p(edges, mll, mlg, threshold=100)
        assert nl[i] == len(lines), i
        assert bits(ang[i]) == bits(offt.vote_fft_rs(lines)), (i, ang[i])
        assert np.array_equal(pics[i], lr.lined_picture(edges, np.asarray(lines, np.int32).reshape(-1, 4))), i


def test_host_form_lands_every_result_at_its_own_index():
    pset = "p2"
    c1, c2, mll, mlg = PARAMS[pset]
    picks = [("pow2", 0), ("mixed", 3), ("small", 1), ("pow2", ZERO_AT), ("mixed", 0), ("small", 7), ("mixed", 10), ("pow2", 9),
             ("small", 4)]
    imgs = [scans_of(s)[0][i] for s, i in picks]
    per = [reference(s, pset)[i] for s, i in picks]
    assert sum(1 for p in per if p[2] == 0) >= 4 and sum(1 for p in per if p[2] >= 2) >= 2, [p[2] for p in per]
    ang, pics = fft.get_angles_with_fft(imgs, c1, c2, mll, mlg, want_pictures=True)
    ang2 = fft.get_angles_with_fft(imgs, c1, c2, mll, mlg)
    for i, (e_ang, e_pic, count) in enumerate(per):
        assert bits(ang[i]) == bits(e_ang) and bits(ang2[i]) == bits(e_ang), (i, count)
        assert np.array_equal(pics[i], e_pic), (i, count)
    # a row pitch wider than the row (a view into a larger image), in a batch of one
    rows, cols = SHAPES["mixed"]
    wide = np.full((rows, cols + 9), 7, np.uint8)
    wide[:, :cols] = imgs[1]
    view = wide[:, :cols]
    im = _lib.OmrImage(view.ctypes.data, rows, cols, 1, view.strides[0])
    a1 = np.zeros(1)
    p1 = (_lib.OmrImageOwned * 1)()
    _lib.check(_lib.lib().omr_get_angles_with_fft_batch(C.byref(im), 1, c1, c2, mll, mlg, a1.ctypes.data_as(_lib.f64p), p1))
    assert bits(a1[0]) == bits(per[1][0]) and np.array_equal(hough._take(p1[0]), per[1][1])
    # an invalid image (3 channels) anywhere in the list fails the call with the per-call code; nothing is written
    bad = np.zeros((rows, cols, 3), np.uint8)
    with pytest.raises(_lib.OmrError) as e0:
        fft.get_angle_with_fft(bad, c1, c2, mll, mlg)
    for where in (0, 4, 9):
        lst = imgs[:where] + [bad] + imgs[where:]
        keep = [fft.as_image(a) for a in lst]
        arr = (_lib.OmrImage * len(lst))(*[im for _, im in keep])
        angles = np.full(len(lst), 7.0)
        owned = (_lib.OmrImageOwned * len(lst))()
        code = _lib.lib().omr_get_angles_with_fft_batch(arr, len(lst), c1, c2, mll, mlg, angles.ctypes.data_as(_lib.f64p), owned)
        assert code == e0.value.code == -215, where
        assert (angles == 7.0).all() and not any(o.data for o in owned)


def colour(gray, cn, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    img = np.stack([gray] * cn, axis=2).astype(np.int16)
    img[:, :, :3] += rng.integers(-12, 13, size=gray.shape + (3,), dtype=np.int16)  # the channels differ
    if cn == 4:
        img[:, :, 3] = rng.integers(0, 256, size=gray.shape)  # alpha is not read
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("cn", [3, 4])
def test_fourier_transform_batch_is_the_per_call_form(cn):
    rows, cols = SHAPES["mixed"]
    scans = [colour(g, cn, 200 + i) for i, g in enumerate(scans_of("mixed")[0][:5])]
    scans[2] = np.zeros((rows, cols, cn), np.uint8)  # the per-call form fails here for want of a segment
    n = len(scans)
    step = cols * cn + 3
    stride = rows * step + 5
    host = np.full(1 + n * stride, 0x5A, np.uint8)
    for i, a in enumerate(scans):
        host[1 + i * stride: 1 + i * stride + rows * step].reshape(rows, step)[:, : cols * cn] = a.reshape(rows, cols * cn)
    d = torch.from_numpy(host).to("cuda:0")
    seen = set()
    for pset in PARAMS:
        ang, st, nl = omr.fourier_transform_batch_device(d.data_ptr() + 1, n, stride, rows, cols, cn, step, *PARAMS[pset])
        for i, img in enumerate(scans):
            try:
                r = omr.get_result_from_fourier_transform(img, *PARAMS[pset])
            except _lib.OmrError as e:
                assert e.code == -215 and "no line segment" in e.message
                assert nl[i] == 0 and st[i] == int(omr.ResultStatus.NotAResult) and bits(ang[i]) == 0, (pset, i)
                seen.add("none")
                continue
            assert nl[i] > 0 and bits(ang[i]) == bits(r.angle) and st[i] == int(r.status), (pset, i, ang[i], r.angle)
            seen.add("some")
    assert np.array_equal(d.cpu().numpy(), host)
    assert seen == {"none", "some"}
