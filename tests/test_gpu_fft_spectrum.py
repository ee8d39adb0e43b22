"""The FFT kernels' float arrays against a float64 DFT, path by path (fft.hip, fft_mixed.hip, fft_big.hip through the
inspection hook omr_fft_spectrum_raw; references, layouts and measures: tests/fft_ref.py, proved in tests/test_fft_ref.py).

tests/test_gpu_fft.py sees the transforms through the two 8-bit pictures, to one grey level: a bin may be several per cent
wrong there.  This is the layer beneath it.  For every shape and input:

  a. row pass, complex: |G - F| over all bins but DC against np.fft.fft of the float64 rows, rms and maximum, normalised
     by the rms of the reference; the DC bin relative to itself.  An odd last row (which goes alone) is part of it.
  b. magnitudes: | |G| - |F| | against np.fft.fft2 / (R C) in float64 (for the impulses: the closed form), same measures.
  c. extrema: the returned min and max are mag.min() and mag.max() of the returned array, bit for bit.
  d. pictures: both 8-bit pictures of the same run equal launch_spec_pictures's expressions evaluated in float64 on the
     GPU's own |F| and extrema, byte for byte -- the shift, the mirror, an odd last row and column, the conversion --
     except where the float64 value before rounding lies within 0.01 grey level of a rounding boundary (float32
     evaluation of some ten operations on values <= 255 errs by about 3e-4 level); at most 5 % of a picture may lie
     there, asserted before the comparison.

The limit of (a) and (b) is not a constant: the same input goes through a float32 stand-in (scipy.fft on complex64, one
pocketfft transform) and through the same measures, and the kernel's error must stay within a factor of the stand-in's on
that case -- 8 for the direct transforms (power of two, mixed radix: float32 twiddle tables, radix-8 / radix-16
butterflies, no FMA contraction), 16 for the chirp transforms (three transforms of M >= 2 n points and two pointwise
products where the stand-in runs one), the larger of the two axes' factors for the magnitudes.  A stand-in error below
2e-7 counts as 2e-7 (fft_ref.bounds): where pocketfft happens to be exact -- every bin of a constant image but DC -- the
limit must not become rounding noise.  The constant image's bins are all leakage and are measured against DC.

Shapes: the smallest that reach each factorisation (fft_ref.LENGTHS, once as columns = row pass on real row pairs, once as
rows = column pass, the other axis 5 or 8), the pairing edges of the row pass, three shapes with both passes non-trivial,
and every axis length from 1 to 33 on noise.  Batches need nothing here: tests/test_gpu_fft_batch.py holds them
bit-identical to the per-call pictures.  Each case prints its figures (FFTSPEC ...) before it asserts;
profiles/r29_fft_spectrum.md is made from those lines."""
import json

import numpy as np
import pytest

import fft_ref as R
from oics import fft

pytestmark = pytest.mark.gpu

CASES = [(r, c, k) for (r, c) in R.shapes_all_inputs() for k in R.INPUTS] + [(r, c, "noise") for (r, c) in R.shapes_noise_only()]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("rows,cols,kind", CASES, ids=["%dx%d-%s" % c for c in CASES])
def test_spectrum_against_float64_dft(rows, cols, kind):
    g, closed, (s_row, s_mag, _) = R.choose_input(kind, rows, cols)
    row, mag, (mn, mx), m8, l8 = fft.spectrum_raw(g)
    half = cols // 2 + 1
    assert row.shape == s_row.shape == (half, rows) and mag.shape == s_mag.shape == (half, rows)
    assert m8.shape == l8.shape == (rows, cols)
    (path_c, f_c), (path_r, f_r) = R.axis_path(cols), R.axis_path(rows)
    s_er, s_ef = R.measure(g, closed, s_row, s_mag)
    er, ef = R.measure(g, closed, row, mag)
    lim_r, lim_f = R.bounds(s_er, f_c), R.bounds(s_ef, max(f_c, f_r))
    pic = R.hook_to_picture(mag, cols)
    e_m8, e_l8, pre_m, pre_l = R.pictures64(pic, mn, mx)
    zone_m, bad_m = R.picture_check(m8, e_m8, pre_m)
    zone_l, bad_l = R.picture_check(l8, e_l8, pre_l)
    ext_ok = bool(_bits(mn) == _bits(mag.min()) and _bits(mx) == _bits(mag.max()))
    print("FFTSPEC " + json.dumps({"rows": rows, "cols": cols, "kind": kind, "row_path": path_c, "col_path": path_r,
                                   "row_factor": f_c, "mag_factor": max(f_c, f_r), "standin_row": s_er, "kernel_row": er,
                                   "standin_mag": s_ef, "kernel_mag": ef, "extrema": ext_ok, "zone": [zone_m, zone_l],
                                   "mismatch": [bad_m, bad_l]}))
    for name, e, s, lim in (("row pass", er, s_er, lim_r), ("magnitudes", ef, s_ef, lim_f)):
        for what, a, b, c in zip(("rel_rms", "rel_max", "dc"), e, s, lim):
            assert np.isfinite(a) and a <= c, "%s %s: kernel %.3g, stand-in %.3g, limit %.3g" % (name, what, a, b, c)
    assert ext_ok, ("extrema", float(mn), float(mag.min()), float(mx), float(mag.max()))
    assert zone_m <= R.ZONE_MAX_SHARE and zone_l <= R.ZONE_MAX_SHARE, ("boundary zone", zone_m, zone_l)
    assert bad_m == 0, "magnitude picture: %d bytes differ outside the boundary zone" % bad_m
    assert bad_l == 0, "log picture: %d bytes differ outside the boundary zone" % bad_l


def test_outputs_are_optional_and_one_run():
    """any subset of the outputs, and the pictures are omr_get_fft_image's"""
    import ctypes as C
    from oics import _lib
    from oics.transfer import as_image
    g, _ = R.make_input("noise", 37, 50)
    row, mag, (mn, mx), m8, l8 = fft.spectrum_raw(g)
    a, b = fft.get_fft_image(g)
    assert (a == m8).all() and (b == l8).all()
    keep, im = as_image(g)
    only = np.zeros_like(mag)
    assert _lib.lib().omr_fft_spectrum_raw(C.byref(im), None, only.ctypes.data_as(_lib.f32p), None, None, None) == 0
    assert (_bits(only) == _bits(mag)).all()
    ext = np.zeros(2, np.float32)
    assert _lib.lib().omr_fft_spectrum_raw(C.byref(im), None, None, ext.ctypes.data_as(_lib.f32p), None, None) == 0
    assert (_bits(ext) == _bits([mn, mx])).all()
    assert _lib.lib().omr_fft_spectrum_raw(C.byref(im), None, None, None, None, None) == -5
