"""CPU-side checks of the JPEG decoder's boundary (omr_jpeg_info, omr_jpeg_decode_batch_device, omr_jpeg_decode,
omr_jpeg_decode_stats, omr_correct_default_batch_streams): declared
in the header, the ctypes table and ffi.rs alike and exported; omr_jpeg_info against the restatement's parser; every
argument error and every header refusal before any device work; the Python and Rust front doors."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_jpeg_decode as fz  # noqa: E402
import jpeg_dec_ref as R  # noqa: E402
import jpeg_ref  # noqa: E402
import oics  # noqa: E402
import test_jpeg_dec_ref as cases  # noqa: E402
from oics import _lib, jpeg  # noqa: E402

NEW = {
    "omr_jpeg_info": ("int", ["const uint8_t *", "int64_t", "int32_t *", "int32_t *", "int32_t *", "int32_t *"]),
    "omr_jpeg_decode_batch_device": ("int", ["const uint8_t * const *", "const int64_t *", "int32_t", "int32_t", "uint8_t *",
                                             "int64_t", "int64_t", "int32_t", "int32_t", "int32_t *", "int32_t *"]),
    "omr_jpeg_decode": ("int", ["const uint8_t *", "int64_t", "int32_t", "omr_image_owned *"]),
    "omr_jpeg_decode_stats": ("int", ["int32_t", "int32_t *", "int32_t *", "int32_t *", "double *"]),
    "omr_correct_default_batch_streams": ("int", ["const uint8_t * const *", "const int64_t *", "int32_t", "uint16_t", "double",
                                                  "int32_t", "int32_t", "double", "double", "int32_t", "double *", "int32_t *",
                                                  "int32_t *", "uint8_t * *", "int64_t *"]),
}
# what ffi.rs must say, argument for argument (written out here, not derived with the generator's own mapping)
RUST = {
    "omr_jpeg_info": (["*const u8", "i64", "*mut i32", "*mut i32", "*mut i32", "*mut i32"], "c_int"),
    "omr_jpeg_decode_batch_device": (["*mut *const u8", "*const i64", "i32", "i32", "*mut u8", "i64", "i64", "i32", "i32",
                                      "*mut i32", "*mut i32"], "c_int"),
    "omr_jpeg_decode": (["*const u8", "i64", "i32", "*mut OmrImageOwned"], "c_int"),
    "omr_jpeg_decode_stats": (["i32", "*mut i32", "*mut i32", "*mut i32", "*mut f64"], "c_int"),
    "omr_correct_default_batch_streams": (["*mut *const u8", "*const i64", "i32", "u16", "f64", "i32", "i32", "f64", "f64", "i32",
                                           "*mut f64", "*mut i32", "*mut i32", "*mut *mut u8", "*mut i64"], "c_int"),
}
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint16_t": C.c_uint16, "double": C.c_double}
PARAMS = (45, 0.2, 248, 230, 150.0, 50.0)  # correct_default's, lib.rs:192-205
NO_GPU = oics.lib().omr_device_count() < 1


def _err():
    return oics.lib().omr_last_error().decode()


def test_symbols_agree_everywhere():
    import gen_shim_ffi as g
    decls = {name: (ret, [t for t, _ in params]) for name, ret, params in g.parse_header()}
    L = C.CDLL(_lib.LIB_PATH)
    ffi = open(os.path.join(ROOT, "shim", "oics", "src", "ffi.rs")).read()
    assert g.render(g.parse_header()) == ffi, "ffi.rs is stale: run python tools/gen_shim_ffi.py"
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
        m = re.search(r"pub fn %s\(([^)]*)\)( -> (\w+))?;" % name, ffi)
        assert m, name
        rust_args = [a.split(":", 1)[1].strip() for a in m.group(1).split(",") if a.strip()]
        assert (rust_args, m.group(3)) == RUST[name], (name, rust_args, m.group(3))
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    assert "Decoding is not part of the library" not in header


def _info(s):
    b = np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8)
    out = [C.c_int32(-7) for _ in range(4)]
    rc = oics.lib().omr_jpeg_info(b.ctypes.data, len(s), *[C.byref(v) for v in out])
    return rc, tuple(v.value for v in out)


def _streams():
    """good streams of every variant and shape, the encoder's restatement's, a dataset sheet; the refusals"""
    out = []
    k = 0
    for rows, cols in cases.SHAPES:
        for v in cases.VARIANTS:
            out.append(fz.make_stream(cases.content(rows, cols, ("noise", "flat", "ruled")[k % 3]), (100, 90, 25)[k % 3], **v))
            k += 1
    img = cases.content(15, 17, "noise")
    out += [jpeg_ref.encode(img, 75), jpeg_ref.encode(img[..., 0].copy(), 75)]
    out.append(open(os.path.join(cases.DATASET, "image001.jpg"), "rb").read())
    return out


def _refused():
    good = fz.make_stream(cases.content(37, 53, "noise"), 90, subsampling=2)
    sof, sos = good.index(b"\xff\xc0"), good.index(b"\xff\xda")

    def patched(at, value):
        b = bytearray(good)
        b[at] = value
        return bytes(b)

    exif6 = b"Exif\x00\x00II*\x00\x08\x00\x00\x00\x01\x00\x12\x01\x03\x00\x01\x00\x00\x00\x06\x00\x00\x00\x00\x00\x00\x00"
    app1 = b"\xff\xe1" + (len(exif6) + 2).to_bytes(2, "big") + exif6
    return [fz.make_stream(cases.content(37, 53, "noise"), 90, progressive=True), patched(sof + 1, 0xC1), patched(sof + 4, 12),
            patched(sof + 11, 0x41), patched(sof + 14, 0x12), good[:sof] + app1 + good[sof:],
            good[:sof] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + good[sof:],
            good[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00", b"\x00" + good[1:], b"", good[:sof + 6], good[:sos],
            patched(sos + 6, 0x13), patched(sof + 12, 3), good[:sof + 5] + b"\x00\x00" + good[sof + 7:]]


def test_info_equals_the_restatements_parser():
    for s in _streams() + _refused():
        code, h = R.parse(s)
        rc, (rows, cols, comps, sampling) = _info(s)
        assert rc == code, (rc, code, _err())
        if rc:
            assert _err()
        assert (rows, cols) == ((h.rows, h.cols) if h else (0, 0))
        if code == 0:
            assert (comps, sampling) == (h.ncomp, h.hs << 4 | h.vs)
            assert jpeg.info(s) == (rows, cols, comps, sampling)
    codes = [R.parse(s)[0] for s in _refused()]
    assert codes.count(R.NOTIMPL) == 8 and codes.count(R.BADARG) == 7
    assert oics.lib().omr_jpeg_info(None, 10, None, None, None, None) == -5
    good = _streams()[0]
    b = np.frombuffer(good, np.uint8)
    assert oics.lib().omr_jpeg_info(b.ctypes.data, b.size, None, None, None, None) == 0


def _batch(streams, channels=3, d_out=0x1000, stride=None, step=None, rows=64, cols=64, n=None, size=True, rc=True,
           null_stream=None, lens=True):
    bufs = [np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8) for s in streams]
    n = len(bufs) if n is None else n
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data for b in bufs])
    if null_stream is not None:
        ptrs[null_stream] = None
    ln = np.array([len(s) for s in streams] + [0], np.int64)
    step = cols * channels if step is None else step
    stride = rows * step if stride is None else stride
    out_size, codes = np.full((max(n, 1), 2), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    r = oics.lib().omr_jpeg_decode_batch_device(ptrs if streams is not None else None,
                                                ln.ctypes.data_as(C.POINTER(C.c_int64)) if lens else None, n, channels, d_out,
                                                stride, step, rows, cols, out_size.ctypes.data_as(_lib.i32p) if size else None,
                                                codes.ctypes.data_as(_lib.i32p) if rc else None)
    return r, out_size, codes


def test_argument_errors_and_header_refusals_come_before_any_device_work():
    """d_out is not device memory: a call that touched it would crash, with or without a GPU"""
    good = fz.make_stream(cases.content(37, 53, "noise"), 90, subsampling=2)
    for kw, text in [(dict(n=-1), "negative n"), (dict(d_out=None), "null"), (dict(size=False), "null"), (dict(rc=False), "null"),
                     (dict(lens=False), "null"), (dict(null_stream=0), "streams[0]"), (dict(channels=2), "1 or 3"),
                     (dict(channels=4), "1 or 3"), (dict(rows=0), "empty"), (dict(cols=-1), "empty"),
                     (dict(step=64 * 3 - 1), "step_bytes"), (dict(stride=64 * 192 - 1), "out_stride_bytes")]:
        r, size, codes = _batch([good], **kw)
        assert r == -5 and text in _err(), (kw, r, _err())
        assert (size == -7).all() and (codes == -7).all(), kw
    r, size, codes = _batch([], n=0)
    assert r == 0 and (codes == -7).all()
    # every stream refused: the codes per image, no device asked for
    bad = _refused()
    r, size, codes = _batch(bad)
    assert r == 0 and list(codes) == [R.parse(s)[0] for s in bad] and (size == 0).all()
    # an image larger than its slot
    r, size, codes = _batch([good, bad[0]], rows=36, cols=53)
    assert r == 0 and list(codes) == [-5, -213]
    r, size, codes = _batch([good], rows=37, cols=52)
    assert r == 0 and codes[0] == -5
    if NO_GPU:
        r, size, codes = _batch([bad[0], good])
        assert r == -217 and list(codes) == [-213, 0] and list(size[1]) == [37, 53]


def test_host_form_argument_errors():
    L = oics.lib()
    good = np.frombuffer(fz.make_stream(cases.content(16, 16, "flat"), 90), np.uint8)
    out = _lib.OmrImageOwned()
    assert L.omr_jpeg_decode(None, 10, 3, C.byref(out)) == -5
    assert L.omr_jpeg_decode(good.ctypes.data, good.size, 3, None) == -5
    assert L.omr_jpeg_decode(good.ctypes.data, good.size, 2, C.byref(out)) == -5
    prog = np.frombuffer(fz.make_stream(cases.content(16, 16, "flat"), 90, progressive=True), np.uint8)
    assert L.omr_jpeg_decode(prog.ctypes.data, prog.size, 3, C.byref(out)) == -213
    assert L.omr_jpeg_decode(good.ctypes.data, 1, 3, C.byref(out)) == -5 and not out.data
    if NO_GPU:
        assert L.omr_jpeg_decode(good.ctypes.data, good.size, 3, C.byref(out)) == -217 and not out.data
        with pytest.raises(oics.OmrError) as e:
            jpeg.decode(good.tobytes())
        assert e.value.code == -217
        with pytest.raises(oics.OmrError) as e:
            oics.transfer.TransformableMatrix.from_jpeg_bytes(good.tobytes())
        assert e.value.code == -217


def test_entropy_data_of_2_to_the_32_bits_is_refused_on_the_host():
    """a header in front of 2^29 bytes that nobody touches: the parser alone decides, before any device work"""
    good = fz.make_stream(cases.content(16, 16, "flat"), 90)
    sos = good.index(b"\xff\xda")
    hdr = good[:sos + 2 + ((good[sos + 2] << 8) | good[sos + 3])]
    big = np.zeros(len(hdr) + (1 << 29), np.uint8)       # calloc'ed: the pages behind the header are never read
    big[:len(hdr)] = np.frombuffer(hdr, np.uint8)
    L = oics.lib()
    assert L.omr_jpeg_info(big.ctypes.data, big.size, None, None, None, None) == -215 and "2^32 bits" in _err()
    assert L.omr_jpeg_info(big.ctypes.data, len(hdr) + (1 << 28), None, None, None, None) == 0
    ptrs = (C.c_void_p * 1)(big.ctypes.data)
    ln = np.array([big.size], np.int64)
    size, codes = np.full((1, 2), -7, np.int32), np.full(1, -7, np.int32)
    r = L.omr_jpeg_decode_batch_device(ptrs, ln.ctypes.data_as(C.POINTER(C.c_int64)), 1, 3, 0x1000, 16 * 48, 48, 16, 16,
                                       size.ctypes.data_as(_lib.i32p), codes.ctypes.data_as(_lib.i32p))
    assert r == 0 and codes[0] == -215 and (size == 0).all()
    out = _lib.OmrImageOwned()
    assert L.omr_jpeg_decode(big.ctypes.data, big.size, 3, C.byref(out)) == -215 and not out.data


def _composite(streams, n=None, null_stream=None, lens=True, outs=(True,) * 5, neg_len=False):
    bufs = [np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8) for s in streams]
    n = len(bufs) if n is None else n
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data for b in bufs])
    if null_stream is not None:
        ptrs[null_stream] = None
    ln = np.array([len(s) for s in streams] + [0], np.int64)
    if neg_len:
        ln[0] = -1
    m = max(n, 1)
    ang, chk, rc = np.full(m, -7.0), np.full(m, -7, np.int32), np.full(m, -7, np.int32)
    jp, jl = (_lib.u8p * m)(), np.full(m, -7, np.int64)
    args = [ang.ctypes.data_as(_lib.f64p), chk.ctypes.data_as(_lib.i32p), rc.ctypes.data_as(_lib.i32p), jp,
            jl.ctypes.data_as(C.POINTER(C.c_int64))]
    args = [a if keep else None for a, keep in zip(args, outs)]
    r = oics.lib().omr_correct_default_batch_streams(ptrs if streams is not None else None,
                                                     ln.ctypes.data_as(C.POINTER(C.c_int64)) if lens else None, n, *PARAMS, 100,
                                                     *args)
    return r, ang, chk, rc, jp, jl


def test_streams_composite_argument_errors_and_refusals_come_before_any_device_work():
    good = fz.make_stream(cases.content(37, 53, "noise"), 90, subsampling=2)
    cases_ = [dict(n=0), dict(n=-1), dict(lens=False), dict(null_stream=0), dict(neg_len=True)]
    cases_ += [dict(outs=tuple(k != j for k in range(5))) for j in range(5)]
    for kw in cases_:
        r, ang, chk, rc, jp, jl = _composite([good], **kw)
        assert r == -5 and _err(), kw
        assert (rc == -7).all() and (jl == -7).all(), kw
    # every sheet refused: the decoder's code per sheet, no output, no device asked for
    bad = _refused()
    r, ang, chk, rc, jp, jl = _composite(bad)
    assert r == 0 and list(rc) == [R.parse(s)[0] for s in bad]
    assert (ang == 0).all() and (chk == 0).all() and (jl == 0).all() and not any(jp[i] for i in range(len(bad)))
    if NO_GPU:
        r, ang, chk, rc, jp, jl = _composite([bad[0], good])
        assert r == -217 and not jp[0] and not jp[1]
        with pytest.raises(oics.OmrError) as e:
            oics.omr.correct_default_batch_streams([good], *PARAMS)
        assert e.value.code == -217
    assert [t[3] for t in oics.omr.correct_default_batch_streams(bad[:3], *PARAMS)] == [R.parse(s)[0] for s in bad[:3]]


def test_stats_are_zero_until_a_decode_ran_with_the_collection_on():
    bits, groups, rounds, ms = jpeg.decode_stats(False)
    assert bits > 0 and bits % 32 == 0 and len(ms) == len(jpeg.STAGES) == 6
    if NO_GPU:
        assert groups == 0 and rounds == 0 and ms == [0.0] * 6
    assert oics.lib().omr_jpeg_decode_stats(0, None, None, None, None) == 0


def test_front_doors():
    assert callable(jpeg.info) and callable(jpeg.decode) and callable(jpeg.decode_batch)
    assert callable(oics.omr.correct_default_batch_streams) and callable(jpeg.decode_stats)
    omr_rs = open(os.path.join(ROOT, "shim", "oics", "src", "omr.rs")).read()
    files = omr_rs.split("pub fn correct_default_files(")[1].split("\n}\n")[0]
    assert "std::fs::read(" in files and "ffi::omr_correct_default_batch_streams(" in files and "std::fs::write(" in files
    assert "ffi::omr_bytes_free(" in files and "imgcodecs" not in files and "scan_rc[i] != 0" in files
    many = omr_rs.split("pub fn correct_defaults(")[1].split("\n}\n")[0]
    assert "imgcodecs::imread" in many and "omr_correct_default_batch_streams" not in many     # stays as it is
    assert callable(oics.transfer.TransformableMatrix.from_jpeg_bytes)
    transfer = open(os.path.join(ROOT, "shim", "oics", "src", "transfer.rs")).read()
    dec = transfer.split("pub fn decode_jpeg(")[1].split("\n}\n")[0]
    assert "ffi::omr_jpeg_decode(" in dec and "imgcodecs" not in dec
    assert re.search(r"pub fn decode_jpeg\(\s*stream: &\[u8\],\s*channels: i32\s*\)\s*->\s*Result<TransformableMatrix", transfer)
