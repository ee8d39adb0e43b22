"""CPU-side checks of the PNG decoder's boundary (omr_png_info, omr_png_decode_batch_device, omr_png_decode,
omr_png_decode_stats, PNG sheets in omr_correct_default_batch_streams): declared in the header, the ctypes table and ffi.rs
alike and exported; omr_png_info against the restatement's parser with a stream per rule; every argument error and every
refusal before any device work; the Python and Rust front doors."""
import ctypes as C
import os
import re
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import png_ref as P  # noqa: E402
import oics  # noqa: E402
import test_png_ref as cases  # noqa: E402
from oics import _lib, png  # noqa: E402

NEW = {
    "omr_png_info": ("int", ["const uint8_t *", "int64_t", "int32_t *", "int32_t *", "int32_t *", "int32_t *"]),
    "omr_png_decode_batch_device": ("int", ["const uint8_t * const *", "const int64_t *", "int32_t", "int32_t", "uint8_t *",
                                            "int64_t", "int64_t", "int32_t", "int32_t", "int32_t *", "int32_t *"]),
    "omr_png_decode": ("int", ["const uint8_t *", "int64_t", "int32_t", "omr_image_owned *"]),
    "omr_png_decode_stats": ("int", ["int32_t", "int32_t *", "double *"]),
}
# what ffi.rs must say, argument for argument (written out here, not derived with the generator's own mapping)
RUST = {
    "omr_png_info": (["*const u8", "i64", "*mut i32", "*mut i32", "*mut i32", "*mut i32"], "c_int"),
    "omr_png_decode_batch_device": (["*mut *const u8", "*const i64", "i32", "i32", "*mut u8", "i64", "i64", "i32", "i32",
                                     "*mut i32", "*mut i32"], "c_int"),
    "omr_png_decode": (["*const u8", "i64", "i32", "*mut OmrImageOwned"], "c_int"),
    "omr_png_decode_stats": (["i32", "*mut i32", "*mut f64"], "c_int"),
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


def _info(s):
    b = np.frombuffer(bytes(s), np.uint8) if len(s) else np.zeros(1, np.uint8)
    out = [C.c_int32(-7) for _ in range(4)]
    rc = oics.lib().omr_png_info(b.ctypes.data, len(s), *[C.byref(v) for v in out])
    return rc, tuple(v.value for v in out)


def _good():
    out = []
    for k, (ct, depth) in enumerate(P.TAKEN):
        rows, cols = cases.SHAPES[k % len(cases.SHAPES)]
        arr = cases.content(rows, cols, ct, depth, cases.CONTENTS[k % 3], seed=k)
        out.append(P.write(arr, ct, depth, cases.palette_of(depth) if ct == 3 else None, filters="rotate",
                           cuts=(None, 1, [0, 2, 0])[k % 3], before_idat=[(b"gAMA", b"\x00\x00\xb1\x8f"), (b"tRNS", b"\x00\x01")]))
    tiff = b"II*\x00\x08\x00\x00\x00\x01\x00\x12\x01\x03\x00\x01\x00\x00\x00\x01\x00\x00\x00\x00\x00\x00\x00"
    out.append(P.write(cases.content(7, 9, 2, 8, "noise"), 2, 8, before_idat=[(b"eXIf", tiff)], after_idat=[(b"acTL", bytes(8))]))
    return out


ARR = cases.content(7, 9, 2, 8, "noise")
ZS = P.deflate(P.filter_rows(P.pack_rows(ARR, 2, 8), 3, 1))


def _rules():
    """(rule, stream, code): one stream per rule of the header's PNG section"""
    tiff6 = b"MM\x00*\x00\x00\x00\x08\x00\x01\x01\x12\x00\x03\x00\x00\x00\x01\x00\x06\x00\x00\x00\x00\x00\x00"
    good = P.assemble(7, 9, 2, 8, ZS)
    idat = good.index(b"IDAT") - 4
    iend = good.index(b"IEND") - 4
    head = P.SIGNATURE + P.ihdr(7, 9, 2, 8)
    pal_zs = P.deflate(bytes(7 * 10))

    def zhdr(b0, b1):
        return P.assemble(7, 9, 2, 8, bytes([b0, b1]) + ZS[2:])

    return [
        ("Adam7", P.assemble(7, 9, 2, 8, ZS, interlace=1), P.NOTIMPL),
        ("16-bit gray", P.assemble(7, 9, 0, 16, ZS), P.NOTIMPL),
        ("16-bit RGBA", P.assemble(7, 9, 6, 16, ZS), P.NOTIMPL),
        ("eXIf orientation 6", P.assemble(7, 9, 2, 8, ZS, before_idat=[(b"eXIf", tiff6)]), P.NOTIMPL),
        ("eXIf orientation 6 behind IDAT", P.assemble(7, 9, 2, 8, ZS, after_idat=[(b"eXIf", tiff6)]), P.NOTIMPL),
        ("acTL before IDAT", P.assemble(7, 9, 2, 8, ZS, before_idat=[(b"acTL", bytes(8))]), P.NOTIMPL),
        ("no signature", b"\x88" + good[1:], P.BADARG),
        ("a JPEG", b"\xff\xd8\xff\xe0" + bytes(20), P.BADARG),
        ("empty", b"", P.BADARG),
        ("a chunk running past the end", good[:idat + 20], P.BADARG),
        ("half a chunk header", good[:idat + 5], P.BADARG),
        ("IHDR missing", P.SIGNATURE + good[idat:], P.BADARG),
        ("IHDR not first", P.SIGNATURE + P.chunk(b"gAMA", bytes(4)) + good[8:], P.BADARG),
        ("IHDR twice", head + good[8:], P.BADARG),
        ("IHDR of 12 bytes", P.SIGNATURE + P.chunk(b"IHDR", bytes(12)) + good[idat:], P.BADARG),
        ("0 rows", P.assemble(0, 9, 2, 8, ZS), P.BADARG),
        ("0 cols", P.assemble(7, 0, 2, 8, ZS), P.BADARG),
        ("depth 4 with RGB", P.assemble(7, 9, 2, 4, ZS), P.BADARG),
        ("depth 16 with a palette", P.assemble(7, 9, 3, 16, ZS, palette=bytes(6)), P.BADARG),
        ("depth 3", P.assemble(7, 9, 0, 3, ZS), P.BADARG),
        ("colour type 5", P.assemble(7, 9, 5, 8, ZS), P.BADARG),
        ("interlace 2", P.assemble(7, 9, 2, 8, ZS, interlace=2), P.BADARG),
        ("no IDAT", head + P.chunk(b"IEND"), P.BADARG),
        ("IDAT not consecutive", head + P.chunk(b"IDAT", ZS[:5]) + P.chunk(b"tEXt", b"k\x00v") + P.chunk(b"IDAT", ZS[5:]) + P.chunk(b"IEND"), P.BADARG),
        ("a palette image without PLTE", P.assemble(7, 9, 3, 8, pal_zs), P.BADARG),
        ("PLTE of 7 bytes", P.assemble(7, 9, 3, 8, pal_zs, palette=bytes(7)), P.BADARG),
        ("PLTE of 771 bytes", P.assemble(7, 9, 3, 8, pal_zs, palette=bytes(771)), P.BADARG),
        ("PLTE behind IDAT", P.assemble(7, 9, 2, 8, ZS, after_idat=[(b"PLTE", bytes(6))]), P.BADARG),
        ("an unknown critical chunk", P.assemble(7, 9, 2, 8, ZS, before_idat=[(b"IDOT", bytes(4))]), P.BADARG),
        ("zlib: CM 7", zhdr(0x77, 0x00 + (31 - (0x7700 % 31)) % 31), P.BADARG),
        ("zlib: a 64 K window", zhdr(0x88, (31 - (0x8800 % 31)) % 31), P.BADARG),
        ("zlib: FDICT", zhdr(0x78, 0x20 + (31 - (0x7820 % 31)) % 31), P.BADARG),
        ("zlib: FCHECK", zhdr(0x78, 0x9d), P.BADARG),
        ("zlib: one byte of IDAT", P.assemble(7, 9, 2, 8, ZS[:1]), P.BADARG),
        ("no IEND", good[:iend], P.ASSERT),
        ("2^20 + 1 columns", P.assemble(1, (1 << 20) + 1, 0, 1, ZS), P.ASSERT),
        ("2^20 + 1 rows", P.assemble((1 << 20) + 1, 1, 0, 1, ZS), P.ASSERT),
        ("more than 2^30 pixels", P.assemble(1025, 1 << 20, 0, 1, ZS), P.ASSERT),
        ("a row of 2^30 RGB pixels", P.assemble(1, 1 << 30, 2, 8, ZS), P.ASSERT),
        ("2^32 bytes of raw data", P.assemble(1 << 18, 1 << 12, 6, 8, ZS), P.ASSERT),
    ]


def test_info_equals_the_restatements_parser():
    for s in _good():
        code, h = P.parse(s)
        assert code == 0
        rc, got = _info(s)
        assert rc == 0 and got == (h.rows, h.cols, h.color_type, h.depth), (rc, _err())
        assert png.info(s) == got
    for rule, s, want in _rules():
        code, h = P.parse(s)
        assert code == want, (rule, code)
        rc, got = _info(s)
        assert rc == code and _err(), (rule, rc, _err())
        assert got == ((h.rows, h.cols, h.color_type, h.depth) if h else (0, 0, 0, 0)), rule
        with pytest.raises(oics.OmrError) as e:
            png.info(s)
        assert e.value.code == want
    # the largest sizes the parser takes: imread's own limits
    for rows, cols, ct, depth in ((1, 1 << 20, 0, 1), (1 << 20, 1, 3, 1), (1 << 10, 1 << 20, 0, 1), (1 << 15, 1 << 15, 2, 8)):
        s = P.assemble(rows, cols, ct, depth, ZS, palette=bytes(6) if ct == 3 else None)
        assert _info(s) == (0, (rows, cols, ct, depth)) and P.parse(s)[0] == 0, (rows, cols)
    # a critical chunk's CRC is the decoder's business, not the parser's; an ancillary chunk's nobody's
    s = bytearray(_good()[3])
    s[s.index(b"IDAT") + 6] ^= 1
    assert _info(bytes(s))[0] == 0 and P.parse(bytes(s))[0] == 0 and P.decode(bytes(s))[0] == P.ASSERT
    assert oics.lib().omr_png_info(None, 10, None, None, None, None) == -5
    b = np.frombuffer(_good()[0], np.uint8)
    assert oics.lib().omr_png_info(b.ctypes.data, b.size, None, None, None, None) == 0


def test_info_equals_the_restatements_parser_on_mutated_streams():
    """byte flips, truncations and insertions anywhere in small files: the same code and the same IHDR fields"""
    rng = np.random.default_rng(23)
    seeds = _good()[:6] + [s for _, s, _ in _rules()[:6]]
    for k in range(1500):
        s = bytearray(seeds[k % len(seeds)])
        at = int(rng.integers(0, len(s)))
        if k % 3 == 0:
            s[at] ^= 1 << int(rng.integers(0, 8))
        elif k % 3 == 1:
            s = s[:at]
        else:
            s[at:at] = bytes(rng.integers(0, 256, int(rng.integers(1, 14)), dtype=np.uint8))
        code, h = P.parse(bytes(s))
        rc, got = _info(bytes(s))
        assert rc == code, (k, rc, code, _err())
        assert got == ((h.rows, h.cols, h.color_type, h.depth) if h else (0, 0, 0, 0)), k


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
    r = oics.lib().omr_png_decode_batch_device(ptrs, ln.ctypes.data_as(C.POINTER(C.c_int64)) if lens else None, n, channels,
                                               d_out, stride, step, rows, cols, out_size.ctypes.data_as(_lib.i32p) if size else None,
                                               codes.ctypes.data_as(_lib.i32p) if rc else None)
    return r, out_size, codes


def test_argument_errors_and_refusals_come_before_any_device_work():
    """d_out is not device memory: a call that touched it would crash, with or without a GPU"""
    good = P.assemble(7, 9, 2, 8, ZS)
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
    bad = [s for _, s, _ in _rules()]
    r, size, codes = _batch(bad)
    assert r == 0 and list(codes) == [c for _, _, c in _rules()] and (size == 0).all()
    # gray from a colour or a paletted stream; an image larger than its slot
    pal = P.write(cases.content(7, 9, 3, 4, "noise"), 3, 4, cases.palette_of(4))
    r, size, codes = _batch([good, pal], channels=1)
    assert r == 0 and list(codes) == [-213, -213] and "rgb_to_gray" in _err()
    r, size, codes = _batch([good, bad[0]], rows=6, cols=9)
    assert r == 0 and list(codes) == [-5, -213]
    r, size, codes = _batch([good], rows=7, cols=8)
    assert r == 0 and codes[0] == -5
    if NO_GPU:
        r, size, codes = _batch([bad[0], good])
        assert r == -217 and list(codes) == [-213, 0] and list(size[1]) == [7, 9]


def test_host_form_argument_errors():
    L = oics.lib()
    good = np.frombuffer(P.assemble(7, 9, 2, 8, ZS), np.uint8)
    out = _lib.OmrImageOwned()
    assert L.omr_png_decode(None, 10, 3, C.byref(out)) == -5
    assert L.omr_png_decode(good.ctypes.data, good.size, 3, None) == -5
    assert L.omr_png_decode(good.ctypes.data, good.size, 2, C.byref(out)) == -5
    assert L.omr_png_decode(good.ctypes.data, good.size, 1, C.byref(out)) == -213
    il = np.frombuffer(P.assemble(7, 9, 2, 8, ZS, interlace=1), np.uint8)
    assert L.omr_png_decode(il.ctypes.data, il.size, 3, C.byref(out)) == -213
    assert L.omr_png_decode(good.ctypes.data, 7, 3, C.byref(out)) == -5 and not out.data
    if NO_GPU:
        assert L.omr_png_decode(good.ctypes.data, good.size, 3, C.byref(out)) == -217 and not out.data
        with pytest.raises(oics.OmrError) as e:
            png.decode(good.tobytes())
        assert e.value.code == -217
        with pytest.raises(oics.OmrError) as e:
            oics.transfer.TransformableMatrix.from_png_bytes(good.tobytes())
        assert e.value.code == -217


def test_correct_default_batch_streams_takes_png_and_refuses_before_any_device_work():
    """only refused PNGs (and a refused JPEG among them): 0 with the codes in scan_rc, no output, no device asked for"""
    rules = _rules()
    jpeg_progressive_like = b"\xff\xd8\xff\xd9"
    streams = [s for _, s, _ in rules if s[:8] == P.SIGNATURE] + [jpeg_progressive_like]
    want = [c for _, s, c in rules if s[:8] == P.SIGNATURE] + [-5]
    got = oics.omr.correct_default_batch_streams(streams, *PARAMS)
    assert [t[3] for t in got] == want
    assert all(t[0] == 0.0 and t[1] is False and t[2] is None for t in got)
    assert want.count(-213) == 6 and want.count(-215) == 6
    if NO_GPU:
        with pytest.raises(oics.OmrError) as e:
            oics.omr.correct_default_batch_streams([streams[0], P.assemble(7, 9, 2, 8, ZS)], *PARAMS)
        assert e.value.code == -217


def test_stats_are_zero_until_a_decode_ran_with_the_collection_on():
    groups, ms = png.stats(False)
    assert len(ms) == len(png.STAGES) == 4
    if NO_GPU:
        assert groups == 0 and ms == [0.0] * 4
    assert oics.lib().omr_png_decode_stats(0, None, None) == 0


def test_front_doors():
    assert callable(png.info) and callable(png.decode) and callable(png.decode_batch_device) and callable(png.stats)
    assert callable(oics.transfer.TransformableMatrix.from_png_bytes)
    transfer = open(os.path.join(ROOT, "shim", "oics", "src", "transfer.rs")).read()
    dec = transfer.split("pub fn decode_png(")[1].split("\n}\n")[0]
    assert "ffi::omr_png_decode(" in dec and "imgcodecs" not in dec
    assert re.search(r"pub fn decode_png\(\s*stream: &\[u8\],\s*channels: i32\s*\)\s*->\s*Result<TransformableMatrix", transfer)
    omr_rs = open(os.path.join(ROOT, "shim", "oics", "src", "omr.rs")).read()
    doc = omr_rs.split("pub fn correct_default_files(")[0].rsplit("\n\n", 1)[1]
    assert "PNG" in doc and "JPEG" in doc
    files = omr_rs.split("pub fn correct_default_files(")[1].split("\n}\n")[0]
    assert "PNG" in files      # the error text no longer speaks of JPEG only
    header = open(os.path.join(ROOT, "include", "omrdeskew.h")).read()
    assert "PNG decoding on the device" in header
    mk = open(os.path.join(ROOT, "omr-img-corrector_amd", "csrc", "Makefile")).read()
    assert "png_dec.hip" in mk and "oics_png_dec.cpp" in mk
