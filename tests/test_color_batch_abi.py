"""CPU-side checks of the colour batch entry points (omr_batch_run_device_cn / omr_batch_deskew_device_cn): declared in
include/omrdeskew.h with the agreed parameter lists, exported by the library, bound by the ctypes table, and argument
errors reported without a GPU.  Plus the property the GPU tests rely on: make_color_card's inks are classified the
opposite way by the reference's gray formula (quirk B8) and by true BGR weights."""
import ctypes as C
import os
import sys

import numpy as np

import oics
from oics import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_shim_ffi  # noqa: E402

RUN_ARGS = [("omr_batch_ctx *", "ctx"), ("const uint8_t *", "d_scans"), ("int64_t", "scan_stride_bytes"),
            ("int64_t", "step_bytes"), ("int32_t", "channels"), ("int32_t", "n"), ("int32_t", "black_max"),
            ("int32_t *", "d_best_idx"), ("double *", "d_v_sd"), ("double *", "d_h_sd")]
DESKEW_ARGS = [("omr_batch_ctx *", "ctx"), ("const uint8_t *", "d_scans"), ("int64_t", "scan_stride_bytes"),
               ("int64_t", "step_bytes"), ("int32_t", "channels"), ("int32_t", "n"), ("int32_t", "black_max"),
               ("int32_t", "interp"), ("const uint8_t *", "border_value"), ("uint8_t *", "d_out"),
               ("int64_t", "out_stride_bytes"), ("int64_t", "out_step_bytes"), ("int32_t *", "d_out_size"),
               ("int32_t *", "d_best_idx")]


def _decls():
    return {name: (ret, params) for name, ret, params in gen_shim_ffi.parse_header()}


def _norm(params):
    return [(" ".join(t.replace("*", " * ").split()), n) for t, n in params]


def test_header_declares_colour_batch_entry_points():
    d = _decls()
    for name, args in (("omr_batch_run_device_cn", RUN_ARGS), ("omr_batch_deskew_device_cn", DESKEW_ARGS)):
        assert name in d, name
        ret, params = d[name]
        assert ret == "int", (name, ret)
        assert _norm(params) == _norm(args), (name, params)


def test_library_exports_and_ctypes_binds_them():
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("omr_batch_run_device_cn", "omr_batch_deskew_device_cn"):
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS["omr_batch_run_device_cn"][1]) == len(RUN_ARGS)
    assert len(_lib.SYMBOLS["omr_batch_deskew_device_cn"][1]) == len(DESKEW_ARGS)


def test_null_context_is_badarg_without_a_gpu():
    L = oics.lib()
    best = (C.c_int32 * 4)()
    rc = L.omr_batch_run_device_cn(None, C.c_void_p(16), 3 * 64 * 64, 3 * 64, 3, 1, 127, C.cast(best, C.c_void_p), None, None)
    assert rc == -5
    assert b"ctx" in L.omr_last_error() or b"argument" in L.omr_last_error()
    border = (C.c_uint8 * 4)(255, 255, 255, 0)
    rc = L.omr_batch_deskew_device_cn(None, C.c_void_p(16), 3 * 64 * 64, 3 * 64, 3, 1, 127, 0, border, C.c_void_p(16),
                                      1 << 20, 1024, None, None)
    assert rc == -5
    assert len(L.omr_last_error()) > 0


def test_color_card_inks_split_the_two_gray_formulas(oracle):
    img, theta = synth.make_color_card(320, 226, 7, skew=3.0)
    assert img.shape == (320, 226, 3) and img.dtype == np.uint8 and theta == 3.0
    quirk = oracle.rgb2gray(img).astype(np.int32)  # cvtColor(COLOR_RGB2GRAY) on BGR bytes (quirk B8)
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    true_bgr = ((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15).astype(np.int32)
    ink = (quirk <= 200) | (true_bgr <= 200)  # not paper
    differ = (quirk <= 127) != (true_bgr <= 127)
    assert ink.sum() > 1000
    assert differ[ink].mean() > 0.25, differ[ink].mean()
    # both directions occur: black only to the quirk formula, and black only to true weights
    assert ((quirk <= 127) & (true_bgr > 127)).sum() > 200
    assert ((quirk > 127) & (true_bgr <= 127)).sum() > 200
    # the paper is tinted and noisy per channel
    paper = (quirk > 200) & (true_bgr > 200)
    assert abs(float(np.median(b[paper])) - 250) <= 2 and abs(float(np.median(r[paper])) - 222) <= 2
    assert b[paper].std() > 1.0 and r[paper].std() > 1.0
