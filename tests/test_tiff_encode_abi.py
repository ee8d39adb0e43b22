"""CPU-side checks of the Group 4 TIFF encoder's boundary (omr_tiff_bound, omr_tiff_encode*, the three _tiff flows):
declared in the header, the ctypes table and ffi.rs alike and exported; the bound against its formula and the run
lengths' code sizes the formula rests on; every argument error before any device work, outputs untouched; the Python and
Rust front doors."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tiff_enc_ref as ref  # noqa: E402
import oics  # noqa: E402
from oics import _lib, tiff  # noqa: E402

STREAMS = ["const uint8_t * const *", "const int64_t *", "int32_t", "int32_t"]
TAIL = ["int32_t", "int32_t", "int32_t", "double *", "int32_t *", "uint8_t * *", "int64_t *"]
NEW = {
    "omr_tiff_bound": ("int", ["int32_t", "int32_t", "int32_t", "int64_t *"]),
    "omr_tiff_encode_batch_device": ("int", ["const uint8_t *", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "const int32_t *",
                                             "int32_t", "int32_t", "int32_t", "int32_t", "uint8_t *", "int64_t", "int64_t *"]),
    "omr_tiff_encode": ("int", ["const omr_image *", "int32_t", "int32_t", "int32_t", "uint8_t *", "int64_t", "int64_t *"]),
    "omr_tiff_encode_stats": ("int", ["int32_t", "int32_t *", "double *"]),
    "omr_deskew_with_projections_batch_streams_tiff": ("int", STREAMS + ["uint16_t", "double", "double", "int32_t", "const uint8_t *",
                                                                         "int32_t", "int32_t", "int32_t", "double *", "int32_t *",
                                                                         "int32_t *", "uint8_t * *", "int64_t *"]),
    "omr_deskew_with_hough_batch_streams_tiff": ("int", STREAMS + ["double", "double", "int32_t", "int32_t", "const uint8_t *",
                                                                   "int32_t"] + TAIL),
    "omr_deskew_with_fft_batch_streams_tiff": ("int", STREAMS + ["double", "double", "double", "double", "int32_t", "int32_t",
                                                                 "const uint8_t *", "int32_t"] + TAIL),
}
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint16_t": C.c_uint16, "double": C.c_double}
NO_GPU = oics.lib().omr_device_count() < 1


def _err():
    return oics.lib().omr_last_error().decode()


def test_symbols_agree_everywhere():
    import gen_shim_ffi as g
    decls = {name: (ret, [t for t, _ in params]) for name, ret, params in g.parse_header()}
    L = C.CDLL(_lib.LIB_PATH)
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    for name, (ret, args) in NEW.items():
        assert decls[name] == (ret, args), (name, decls.get(name))
        assert hasattr(L, name)
        res, at = _lib.SYMBOLS[name]
        assert res is C.c_int and len(at) == len(args), name
        for c, t in zip(args, at):
            if "*" in c:
                assert t is C.c_void_p or hasattr(t, "contents") or hasattr(t, "_type_"), (name, c, t)
            else:
                assert t is CTYPES[c], (name, c, t)
        assert re.search(r"pub fn %s\(" % name, ffi), name
    # the stats call is its PNG twin
    assert decls["omr_tiff_encode_stats"] == decls["omr_png_encode_stats"]


def test_run_code_sizes_the_bound_rests_on():
    """a white run of r >= 1 takes at most 6 r bits and a black one at most 6 r - 3; a run of 0 at most 10"""
    white, black = ref.codes()

    def bits(tab, k):
        out = []
        ref._span(out, k, 0 if tab is white else 1)
        return sum(b for _, b in out)
    for r in list(range(1, 6000)) + [12288, 65536, (1 << 20) - 1, 1 << 20]:
        assert bits(white, r) <= 6 * r and bits(black, r) <= 6 * r - 3, r
    assert bits(white, 0) == 8 and bits(black, 0) == 10
    assert bits(white, 1) == 6 and bits(black, 1) == 3  # alternating pixels: 3 + 6 + 3 bits a pair


def test_bound_against_its_formula_and_the_limits():
    for rows, cols in [(1, 1), (1, 300), (300, 1), (15, 17), (150, 270), (3508, 2480), (1 << 20, 1), (1, 1 << 20), (1 << 10, 1 << 20)]:
        for rps in (0, 1, 8, 64, rows, rows + 5):
            if min(rps or rows, rows) * ref.row_bound(cols) + 31 > 2 ** 31 - 1:
                continue
            assert tiff.bound(rows, cols, rps) == ref.bound(rows, cols, rps), (rows, cols, rps)
    assert tiff.bound(1, 1, 0) == 186 + 8 + 8  # one row of 39 bits and the EOFB: 63 bits, 8 bytes
    out = C.c_int64(-1)
    L = oics.lib()
    assert L.omr_tiff_bound(8, 8, 0, None) == -5
    assert L.omr_tiff_bound(8, 8, -1, C.byref(out)) == -5 and "rows_per_strip" in _err()
    for rows, cols, rps, text in [(0, 8, 0, "empty"), (8, 0, 0, "empty"), ((1 << 20) + 1, 1, 0, "imread"), (1, (1 << 20) + 1, 0, "imread"),
                                  ((1 << 15) + 1, 1 << 15, 1, "imread"), (1 << 15, 1 << 15, 0, "2^31 bits"),
                                  (1 << 15, 1 << 15, 9363, "2^31 bits")]:
        assert L.omr_tiff_bound(rows, cols, rps, C.byref(out)) == -215 and text in _err(), (rows, cols, rps, _err())
    assert out.value == -1
    # the decision from the formula: rows of a strip x (7 cols + 32) + 31 must stay below 2^31
    cols = 1 << 15
    rps = max(r for r in range(9300, 9400) if r * ref.row_bound(cols) + 31 <= 2 ** 31 - 1)
    assert tiff.bound(1 << 15, cols, rps) == ref.bound(1 << 15, cols, rps)
    assert L.omr_tiff_bound(1 << 15, cols, rps + 1, C.byref(out)) == -215 and "2^31 bits" in _err()


def _batch(d_imgs=0x1000, stride=None, step=None, rows=16, cols=24, cn=3, sizes=None, n=2, thr=127, rps=0, dpi=0, d_out=0x2000,
           out_stride=None, out_len=True):
    step = cols * cn if step is None else step
    stride = rows * step if stride is None else stride
    out_stride = 1 << 40 if out_stride is None else out_stride
    lens = np.full(max(n, 1), -7, np.int64)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int32)
    rc = oics.lib().omr_tiff_encode_batch_device(d_imgs, stride, step, rows, cols, cn, None if sz is None else sz.ctypes.data_as(_lib.i32p),
                                                 n, thr, rps, dpi, d_out, out_stride,
                                                 lens.ctypes.data_as(C.POINTER(C.c_int64)) if out_len else None)
    return rc, lens


def test_batch_argument_errors_come_before_any_device_work():
    """the pointers are not device memory: a call that touched them would crash, with or without a GPU"""
    cases = [
        (dict(d_imgs=None), -5, "null"), (dict(d_out=None), -5, "null"), (dict(out_len=False), -5, "null"),
        (dict(n=-1), -5, "negative n"),
        (dict(cn=2), -5, "1 or 3 channels"), (dict(cn=4), -5, "1 or 3 channels"),
        (dict(thr=-1), -5, "threshold"), (dict(thr=255), -5, "threshold"), (dict(rps=-1), -5, "rows_per_strip"), (dict(dpi=-1), -5, "dpi"),
        (dict(rows=0), -215, "empty"), (dict(cols=(1 << 20) + 1), -215, "imread"),
        (dict(rows=1 << 15, cols=1 << 15, cn=1), -215, "2^31 bits"),
        (dict(step=24 * 3 - 1), -5, "step_bytes"), (dict(stride=16 * 72 - 1), -5, "img_stride_bytes"),
        (dict(sizes=[[16, 24], [17, 24]]), -5, "sizes[1]"), (dict(sizes=[[16, 25], [1, 1]]), -5, "sizes[0]"),
        (dict(sizes=[[16, 24], [-1, 3]]), -5, "sizes[1]"), (dict(sizes=[[0, 5], [1, 1]]), -5, "sizes[0]"),
        (dict(out_stride=tiff.bound(16, 24, 0) - 1), -5, "omr_tiff_bound"),
        (dict(rps=1, out_stride=tiff.bound(16, 24, 1) - 1), -5, "omr_tiff_bound"),
    ]
    for kw, code, text in cases:
        rc, lens = _batch(**kw)
        assert rc == code and text in _err(), (kw, rc, _err())
        assert (lens == -7).all(), kw
    rc, lens = _batch(n=0)
    assert rc == 0 and (lens == -7).all()
    if NO_GPU:
        rc, lens = _batch()
        assert rc == -217 and (lens == -7).all()


def test_bad_sizes_have_the_wording_all_four_encoders_share():
    """the same four bad `sizes` stand in test_jpeg_abi, test_png_encode_abi, test_tiff_encode_abi and test_tiff8_encode_abi:
    every encoder's batch entry point answers them with these words, to the letter"""
    for sizes, text in [([[16, 24], [17, 24]], "sizes[1] = 17 x 24 does not fit the 16 x 24 slot"),
                        ([[16, 25], [1, 1]], "sizes[0] = 16 x 25 does not fit the 16 x 24 slot"),
                        ([[16, 24], [-1, 3]], "sizes[1] = -1 x 3 does not fit the 16 x 24 slot"),
                        ([[0, 5], [1, 1]], "sizes[0] = 0 x 5 does not fit the 16 x 24 slot")]:
        rc, lens = _batch(sizes=sizes)
        assert rc == -5 and _err() == text and (lens == -7).all(), (sizes, rc, _err())


def test_host_form_argument_errors_and_the_cap_rule():
    L = oics.lib()
    img = np.zeros((8, 12), np.uint8)
    _, im = oics.transfer.as_image(img)
    n = C.c_int64(-7)
    buf = np.full(64, 0xA5, np.uint8)
    p = buf.ctypes.data_as(_lib.u8p)
    assert L.omr_tiff_encode(None, 127, 0, 0, p, 64, C.byref(n)) == -5
    assert L.omr_tiff_encode(C.byref(im), 127, 0, 0, p, 64, None) == -5
    assert L.omr_tiff_encode(C.byref(im), 127, 0, 0, None, 64, C.byref(n)) == -5
    assert L.omr_tiff_encode(C.byref(im), 127, 0, 0, p, -1, C.byref(n)) == -5
    for thr, rps, dpi, text in ((255, 0, 0, "threshold"), (-1, 0, 0, "threshold"), (127, -1, 0, "rows_per_strip"), (127, 0, -1, "dpi")):
        assert L.omr_tiff_encode(C.byref(im), thr, rps, dpi, p, 64, C.byref(n)) == -5 and text in _err()
    bad = _lib.OmrImage(im.data, 8, 12, 1, 11)
    assert L.omr_tiff_encode(C.byref(bad), 127, 0, 0, p, 64, C.byref(n)) == -5 and "step_bytes" in _err()
    bad = _lib.OmrImage(im.data, 8, 12, 4, 48)
    assert L.omr_tiff_encode(C.byref(bad), 127, 0, 0, p, 64, C.byref(n)) == -5 and "channels" in _err()
    big = _lib.OmrImage(im.data, 1 << 15, 1 << 15, 1, 1 << 15)
    assert L.omr_tiff_encode(C.byref(big), 127, 0, 0, None, 0, C.byref(n)) == -215 and "2^31 bits" in _err()
    assert n.value == -7 and (buf == 0xA5).all()
    if NO_GPU:  # (with a GPU: -4 and the length, tests/test_gpu_tiff_encode.py)
        assert L.omr_tiff_encode(C.byref(im), 127, 0, 0, p, 64, C.byref(n)) == -217 and n.value == -7
    assert L.omr_tiff_encode_stats(0, None, None) == 0
    g = C.c_int32(-1)
    ms = np.full(4, -1.0)
    assert L.omr_tiff_encode_stats(0, C.byref(g), ms.ctypes.data_as(C.POINTER(C.c_double))) == 0 and g.value == 0 and (ms == 0).all()


def _flow(which, streams=True, lens=True, n=2, channels=3, thr=127, rps=0, dpi=0, angles=True, scan_rc=True, out=True, out_len=True,
          border=True, interp=1, clip=1):
    L = oics.lib()
    data = np.zeros(16, np.uint8)
    sp = (C.c_void_p * 2)(data.ctypes.data, data.ctypes.data)
    sl = np.array([16, 16], np.int64)
    ang = np.full(2, -7.0)
    rc = np.full(2, -7, np.int32)
    ptrs = (_lib.u8p * 2)()
    ol = np.full(2, -7, np.int64)
    b = np.array([255, 255, 255, 0], np.uint8)
    common = (sp if streams else None, sl.ctypes.data_as(C.POINTER(C.c_int64)) if lens else None, n, channels)
    tail = (ang.ctypes.data_as(_lib.f64p) if angles else None,)
    outs = (rc.ctypes.data_as(_lib.i32p) if scan_rc else None, ptrs if out else None, ol.ctypes.data_as(C.POINTER(C.c_int64)) if out_len else None)
    bp = b.ctypes.data_as(_lib.u8p) if border else None
    if which == "projection":
        r = L.omr_deskew_with_projections_batch_streams_tiff(*common, 45, 0.2, 0.2, interp, bp, thr, rps, dpi, *tail, None, *outs)
    elif which == "hough":
        r = L.omr_deskew_with_hough_batch_streams_tiff(*common, 40.0, 5.0, interp, 0, bp, clip, thr, rps, dpi, *tail, *outs)
    else:
        r = L.omr_deskew_with_fft_batch_streams_tiff(*common, 30.0, 90.0, 40.0, 5.0, interp, 0, bp, clip, thr, rps, dpi, *tail, *outs)
    untouched = (ang == -7.0).all() and (rc == -7).all() and (ol == -7).all() and not any(bool(p) for p in ptrs)
    return r, untouched


def test_flow_argument_errors_come_before_any_device_work():
    for which in ("projection", "hough", "fft"):
        cases = [dict(streams=False), dict(lens=False), dict(n=0), dict(angles=False), dict(scan_rc=False), dict(out=False),
                 dict(out_len=False), dict(border=False), dict(channels=2), dict(channels=4), dict(thr=-1), dict(thr=255),
                 dict(rps=-1), dict(dpi=-1)]
        for kw in cases:
            r, untouched = _flow(which, **kw)
            assert r == -5 and untouched, (which, kw, r, _err())
        r, untouched = _flow(which, interp=5)
        assert r == -213 and untouched, (which, r)
        if which != "projection":
            r, untouched = _flow(which, clip=7)
            assert r == -5 and untouched, (which, r)
    # the detector flows' public format argument keeps refusing everything but 0 and 1, the private value included
    data = np.zeros(16, np.uint8)
    sp = (C.c_void_p * 1)(data.ctypes.data)
    sl = np.array([16], np.int64)
    ang, rc = np.zeros(1), np.zeros(1, np.int32)
    b = np.array([255, 255, 255, 0], np.uint8)
    for fmt in (2, -26, -1):
        r = oics.lib().omr_deskew_with_hough_batch_streams(sp, sl.ctypes.data_as(C.POINTER(C.c_int64)), 1, 3, 40.0, 5.0, 1, 0,
                                                           b.ctypes.data_as(_lib.u8p), 1, fmt, 100, ang.ctypes.data_as(_lib.f64p),
                                                           rc.ctypes.data_as(_lib.i32p), None, None)
        assert r == -5 and "format" in _err(), fmt


def test_refused_files_need_no_device():
    """a call whose every stream is refused does no device work: the codes come back with or without a GPU"""
    for which in ("projection", "hough", "fft"):
        fn = {"projection": oics.projection.deskew_streams_tiff, "hough": oics.hough.deskew_streams_tiff, "fft": oics.fft.deskew_streams_tiff}[which]
        args = {"projection": (45, 0.2, 0.2), "hough": (40.0, 5.0), "fft": (30.0, 90.0, 40.0, 5.0)}[which]
        ang, rc, out = fn([b"II*\0" + bytes(12), b"not a picture at all"], *args)
        assert list(ang) == [0.0, 0.0] and all(int(c) != 0 for c in rc) and out == [None, None]


def test_front_doors_are_there():
    assert callable(tiff.encode) and callable(tiff.encode_batch_device) and callable(tiff.bound) and callable(tiff.encode_stats)
    assert callable(oics.transfer.TransformableMatrix.encode_tiff)
    src = {f: open(os.path.join(ROOT, "shim", "oics", "src", f + ".rs")).read() for f in ("transfer", "projection", "hough", "fft")}
    assert "pub fn encode_tiff(" in src["transfer"] and "ffi::omr_tiff_encode(" in src["transfer"]
    assert "pub fn deskew_files_with_projections_tiff(" in src["projection"]
    assert "pub fn deskew_files_with_hough_tiff(" in src["hough"] and "pub fn deskew_files_with_fft_tiff(" in src["fft"]
