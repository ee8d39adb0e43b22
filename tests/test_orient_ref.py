"""tests/orient_ref.py against Pillow: the restatement of the eight EXIF transforms equals ImageOps.exif_transpose, the
codes compose as they should, and the EXIF segment it builds is one Pillow reads (CPU only)."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orient_ref as O  # noqa: E402


def _img(cn):
    rng = np.random.Generator(np.random.PCG64(57 + cn))
    return rng.integers(0, 256, (5, 7) if cn == 1 else (5, 7, 3), dtype=np.uint8)


def _pillow(img, code):
    from PIL import Image, ImageOps
    im = Image.fromarray(img)
    exif = Image.Exif()
    exif[0x0112] = code
    im.info["exif"] = exif.tobytes()
    b = io.BytesIO()
    im.save(b, format="PNG", exif=exif)          # lossless, and Pillow reads the orientation back from the file
    return np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(b.getvalue()))))


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("code", O.CODES)
def test_restatement_equals_exif_transpose(code, cn):
    img = _img(cn)
    want = _pillow(img, code)
    got = O.apply(img, code)
    assert got.shape == want.shape == O.turned_shape(5, 7, code) + img.shape[2:]
    assert (got == want).all()
    if code != 1:
        assert got.shape != img.shape or (got != img).any()


@pytest.mark.parametrize("cn", [1, 3])
def test_codes_compose(cn):
    img = _img(cn)
    assert (O.apply(O.apply(img, 6), 8) == img).all() and (O.apply(O.apply(img, 8), 6) == img).all()
    for code in (2, 3, 4, 5, 7):
        assert (O.apply(O.apply(img, code), code) == img).all(), code
    assert (O.apply(O.apply(img, 6), 6) == O.apply(img, 3)).all()


@pytest.mark.parametrize("little_endian", [True, False])
@pytest.mark.parametrize("code", O.CODES)
def test_spliced_segment_is_read_by_pillow(code, little_endian):
    from PIL import Image, ImageOps
    img = _img(3)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=100, subsampling=0)
    plain = b.getvalue()
    tagged = O.tag_jpeg(plain, code, little_endian)
    im = Image.open(io.BytesIO(tagged))
    assert im.getexif().get(0x0112) == code
    stored = np.asarray(Image.open(io.BytesIO(plain)))
    assert (np.asarray(ImageOps.exif_transpose(im)) == O.apply(stored, code)).all()
