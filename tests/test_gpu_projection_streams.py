"""omr_deskew_with_projections_batch_streams / _streams_png on the device: the reference benchmark's flow from file
contents to file contents.

The reference side of every comparison is Pillow's decode of the stream (what imread returns) fed to the per-call
functions: get_angle_with_projections, rotate_mat (CONTAIN, scale 1, constant border) and encode_jpeg / encode_png.  Angles
are compared as f64 bits, streams byte for byte.  Content: the cards of tests/fuzz/fuzz_jpeg.py and the dataset's sheets,
skewed with rotate_mat; streams written by Pillow (tests/fuzz/fuzz_jpeg_decode.py) and by tests/png_ref.py."""
import io
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg  # noqa: E402
import fuzz_jpeg_decode as fj  # noqa: E402
import fuzz_png_decode as fp  # noqa: E402
import png_ref as P  # noqa: E402
from oics import projection, transfer  # noqa: E402
from oics.types import RotateClipStrategy  # noqa: E402

pytestmark = pytest.mark.gpu

NEAREST, LINEAR = 0, 1
SWEEP = (10, 0.5, 0.5)
WHITE = (255, 255, 255)
DATASET = os.path.join(HERE, "golden", "dataset")


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _decoded(stream, channels=3):
    """Pillow's decode: what imread(IMREAD_COLOR) (channels 3) or the gray convenience (1) is given"""
    return (fp if stream[:8] == P.SIGNATURE else fj).pillow_decode(stream, channels)


_CHAIN = {}


def _chain(stream, sweep, interp, channels=3, png=False, level=100, border=WHITE):
    """(angle, canvas, encoded canvas) of the per-call chain on Pillow's decode; computed once per argument set"""
    key = (stream, sweep, interp, channels, png, level, border)
    if key not in _CHAIN:
        dec = _decoded(stream, channels)
        ang = projection.get_angle_with_projections(dec, sweep[0], sweep[1], sweep[2], 1)
        canvas = transfer.rotate_mat(dec, ang, 1.0, interp, 0, tuple(border) + (0,), RotateClipStrategy.CONTAIN)
        _CHAIN[key] = (ang, canvas.get_mat(), canvas.encode_png(level) if png else canvas.encode_jpeg(level))
    return _CHAIN[key]


def _card(rows, cols, seed, skew):
    """a colour card of the JPEG fuzzer, turned by `skew` degrees inside its frame"""
    img = fuzz_jpeg.content(np.random.Generator(np.random.PCG64(seed)), rows, cols, 3, 1)
    return transfer.rotate_mat(img, skew, 1.0, LINEAR, 0, WHITE + (0,)).get_mat()


def _rgb_png(img, **kw):
    return P.write(img[..., ::-1], 2, 8, filters="rotate", **kw)


def _flip_idat_byte(png):
    s = bytearray(png)
    s[png.index(b"IDAT") + 10] ^= 0x20
    return bytes(s)


def _mixed(rows, cols, seed):
    """[(stream, scan_rc expected)] of one shape: the good kinds with a refused and a damaged sheet in the middle"""
    c = [_card(rows, cols, seed + i, skew) for i, skew in enumerate((-4.0, 2.5, 6.0, -1.5, 3.5, 0.5, -6.5))]
    bit = (c[4][..., 1] > 127).astype(np.uint8)
    return [(fj.make_stream(c[0], 90, gray=True), 0),
            (fj.make_stream(c[1], 95, subsampling=2), 0),
            (fj.make_stream(c[5], 90, progressive=True), -213),
            (fj.make_stream(c[2], 100, subsampling=0, restart_marker_blocks=3), 0),
            (_rgb_png(c[3]), 0),
            (_flip_idat_byte(_rgb_png(c[6])), -215),
            (P.write(bit, 0, 1, filters=0), 0)]


_BATCH = []


def _two_shapes():
    """37 x 53: the colour row is 159 bytes, no multiple of 4, neither side a multiple of 8 or 16; and 64 x 48.  The two
    shapes' sheets alternate in the batch."""
    if not _BATCH:
        a, b = _mixed(37, 53, 100), _mixed(64, 48, 200)
        _BATCH.extend(x for pair in zip(a, b) for x in pair)
    return _BATCH


def _check(streams, want_rc, got, sweep, interp, channels=3, png=False, level=100, border=WHITE):
    ang, idx, rc, out = got
    N, _ = projection.candidate_count(sweep[0], sweep[1])
    assert list(rc) == list(want_rc), list(rc)
    for i, (s, code) in enumerate(zip(streams, want_rc)):
        if code:
            assert ang[i] == 0.0 and idx[i] == -1 and out[i] is None, i
            continue
        ref_ang, canvas, ref_bytes = _chain(s, sweep, interp, channels, png, level, border)
        assert _bits(ang[i]) == _bits(ref_ang), (i, ang[i], ref_ang)
        assert _bits((int(idx[i]) - N) * sweep[1]) == _bits(ref_ang), (i, idx[i])
        assert out[i] == ref_bytes, (i, len(out[i]), len(ref_bytes), "the output streams differ")


@pytest.mark.parametrize("interp", [LINEAR, NEAREST])
def test_mixed_batch_of_two_shapes_equals_the_per_call_chain(interp):
    """gray JPEG, 4:2:0, 4:4:4 with a restart interval, RGB PNG, 1-bit gray PNG, with a progressive JPEG (-213) and a PNG
    with one IDAT byte flipped (-215) in the middle, per shape; one bucket holds both kinds of stream"""
    streams, want_rc = [s for s, _ in _two_shapes()], [c for _, c in _two_shapes()]
    got = projection.deskew_streams(streams, *SWEEP, interp=interp, quality=100, want_idx=True)
    _check(streams, want_rc, got, SWEEP, interp)
    outs = [o for o in got[3] if o is not None]
    assert len(outs) == 10 and len(set(outs)) == 10      # ten different sheets: the comparison says something


def test_png_outputs_equal_encode_png_and_decode_to_the_canvas():
    from PIL import Image
    streams, want_rc = [s for s, _ in _two_shapes()], [c for _, c in _two_shapes()]
    got = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, quality=1, png=True, want_idx=True)
    _check(streams, want_rc, got, SWEEP, LINEAR, png=True, level=1)
    for s, code, o in zip(streams, want_rc, got[3]):
        if code == 0:
            canvas = _chain(s, SWEEP, LINEAR, png=True, level=1)[1]
            back = np.asarray(Image.open(io.BytesIO(o)).convert("RGB"))[..., ::-1]
            assert back.shape == canvas.shape and (back == canvas).all()


def test_gray_channel_form_and_the_angles_alone():
    """channels = 1: the Y plane of a gray and of a colour JPEG, an 8-bit and a 1-bit gray PNG, an RGB PNG refused for its
    sheet; single-component JPEG and colour-type-0 PNG out; the angles-only form answers the same angles"""
    c = [_card(53, 37, 300 + i, skew) for i, skew in enumerate((3.0, -2.0, 5.5, -4.5, 1.0))]
    streams = [fj.make_stream(c[0], 92, gray=True), fj.make_stream(c[1], 97, subsampling=2), _rgb_png(c[4]),
               P.write(c[2][..., 1], 0, 8, filters=4), P.write((c[3][..., 0] > 100).astype(np.uint8), 0, 1, filters=0)]
    want_rc = [0, 0, -213, 0, 0]
    got = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, border=(255,), quality=95, channels=1, want_idx=True)
    _check(streams, want_rc, got, SWEEP, LINEAR, channels=1, level=95)
    from oics import jpeg
    assert [jpeg.info(o)[2] for o in got[3] if o] == [1, 1, 1, 1]
    as_png = projection.deskew_streams(streams, *SWEEP, interp=NEAREST, border=(255,), quality=1, channels=1, png=True, want_idx=True)
    _check(streams, want_rc, as_png, SWEEP, NEAREST, channels=1, png=True, level=1)
    from oics import png
    assert [png.info(o)[2] for o in as_png[3] if o] == [0, 0, 0, 0]
    ang, idx, rc = projection.get_angles_from_streams(streams, *SWEEP, channels=1, want_idx=True)
    assert list(rc) == want_rc and (_bits(ang) == _bits(got[0])).all() and (idx == got[1]).all()
    ang3, rc3 = projection.get_angles_from_streams(streams, *SWEEP)
    assert list(rc3) == [0] * 5
    for i, s in enumerate(streams):
        assert _bits(ang3[i]) == _bits(_chain(s, SWEEP, LINEAR)[0]), i


def _deskew_chunk():
    src = open(os.path.join(ROOT, "omr-img-corrector_amd", "csrc", "flow_frame.hpp")).read()
    return int(re.search(r"const int kDeskewChunk = (\d+);", src).group(1))


def test_chunk_boundary_every_sheet_as_if_sent_alone():
    """kDeskewChunk + 1 distinct sheets of 40 x 56, the last of the first chunk damaged: every result is the one the same
    sheet gets in a call of one, and the sheets on both sides of the boundary are the per-call chain's"""
    z = _deskew_chunk()
    streams = []
    for i in range(z + 1):
        card = _card(40, 56, 400 + i, -8.0 + 0.5 * i)
        kind = dict(gray=True) if i % 2 == 0 else dict(subsampling=i % 3)
        streams.append(_rgb_png(card) if i % 3 == 2 else fj.make_stream(card, 90 + i % 10, **kind))
    streams[z - 1] = _flip_idat_byte(_rgb_png(_card(40, 56, 499, 1.0)))
    want_rc = [0] * (z - 1) + [-215, 0]
    ang, idx, rc, out = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, want_idx=True)
    assert list(rc) == want_rc and out[z - 1] is None and ang[z - 1] == 0.0 and idx[z - 1] == -1
    assert len({o for o in out if o}) == z
    for i, s in enumerate(streams):
        a1, i1, r1, o1 = projection.deskew_streams([s], *SWEEP, interp=LINEAR, want_idx=True)
        assert r1[0] == rc[i] and _bits(a1[0]) == _bits(ang[i]) and i1[0] == idx[i] and o1[0] == out[i], i
    for i in (0, z - 2, z):
        ref_ang, _, ref_bytes = _chain(streams[i], SWEEP, LINEAR)
        assert _bits(ang[i]) == _bits(ref_ang) and out[i] == ref_bytes, i
    # the angles-only form takes the whole batch in one run
    a2, r2 = projection.get_angles_from_streams(streams, *SWEEP)
    assert list(r2) == want_rc and (_bits(a2) == _bits(ang)).all()


def test_steep_winner_beyond_the_warps_staging():
    """a 96 x 128 colour card skewed by 33 degrees, swept at +-45 @ 1.0: the winner lies where a colour tile's source box no
    longer fits LDS and the warp taps global memory"""
    card = _card(96, 128, 81, 33.0)   # the oracle's chain answers -34 for this card
    streams = [fj.make_stream(card, 95, subsampling=2), _rgb_png(card)]
    sweep = (45, 1.0, 0.5)
    for interp in (LINEAR, NEAREST):
        got = projection.deskew_streams(streams, *sweep, interp=interp, want_idx=True)
        _check(streams, [0, 0], got, sweep, interp)
        assert (np.abs(got[0]) >= 28.0).all(), got[0]


def test_a_bucket_no_context_is_made_for():
    """omr_projection_batch_create refuses, for 1 or 3 channels: a working size that truncates to 0 or reaches 32767
    (the per-call function fails on such a sheet too: its code, from the header alone), and nothing else a stream can ask
    for -- 4 channels, the case tests/test_gpu_projection_batch.py reaches bucket_per_call with, is no value of `channels`
    here, and a canvas beyond the warp's tables needs rows + cols above 46340.  So the reachable refusal is checked: a
    bucket of 1 x 96 sheets at scale 0.5 answers -215 per sheet, the per-call function's code, and its neighbours of
    another shape are the per-call chain's."""
    card = _card(40, 56, 600, 2.0)
    good = fj.make_stream(card, 95, subsampling=2)
    thin = P.write(np.ascontiguousarray(_card(8, 96, 601, 0.0)[:1, :, ::-1]), 2, 8)
    with pytest.raises(Exception) as e:
        projection.get_angle_with_projections(_decoded(thin), SWEEP[0], SWEEP[1], SWEEP[2], 1)
    assert e.value.code == -215
    streams = [thin, good, thin]
    got = projection.deskew_streams(streams, *SWEEP, interp=LINEAR, want_idx=True)
    _check(streams, [-215, 0, -215], got, SWEEP, LINEAR)


def _dataset_sheet(name, skew):
    """the reference's own test (lib.rs:44-82): the sheet turned by `skew`, gray, written as JPEG"""
    from PIL import Image
    img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(DATASET, name)).convert("RGB"))[..., ::-1])
    turned = transfer.rotate_mat(img, skew, 1.0, LINEAR, 0, WHITE + (0,)).get_mat()
    return fj.make_stream(turned, 95, gray=True)


def test_the_references_own_parameters_on_dataset_sheets():
    """(45, 0.2, 0.2), LINEAR, quality 100 on three dataset sheets with an injected skew, as gray JPEG; the detected angle
    is within 0.5 degrees of the injected one (lib.rs:103-113: the reference's own condition, checked beforehand on the
    CPU with the oracle for these sheets and skews)"""
    sweep = (45, 0.2, 0.2)
    chosen = (("image001.jpg", 2.0), ("image002.jpg", -3.4), ("image003.jpg", 4.2))
    streams = [_dataset_sheet(name, skew) for name, skew in chosen]
    got = projection.deskew_streams(streams, *sweep, interp=LINEAR, quality=100, want_idx=True)
    _check(streams, [0, 0, 0], got, sweep, LINEAR)
    # get_angle_with_projections answers the rotation that undoes the skew: rotate_mat by it restores the sheet.  The
    # oracle's chain gives -2.0, 3.4 and -4.2 for these three.
    for (name, skew), a in zip(chosen, got[0]):
        assert abs(-a - skew) < 0.5, (name, skew, a)
