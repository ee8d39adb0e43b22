"""tests/jpeg_rewrap.py (the coefficient-level stream rewriter) against Pillow / libjpeg-turbo: every stream the device
test (tests/test_gpu_jpeg_foreign.py) feeds the kernels is one Pillow decodes to exactly the bytes it decodes from the
original, at 1 and 3 channels, so the original's decode is what the kernels are held to.  The restatement of the decoder
(tests/jpeg_dec_ref.py) is held to the same bytes, sequentially and with the self-synchronising scheme; the deep tables
send at least 90 % of a stream's symbols down codes of more than 9 bits, the flat ones none."""
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg_decode as fz  # noqa: E402
import jpeg_dec_ref as R  # noqa: E402
import jpeg_rewrap as W  # noqa: E402


def _pillow(stream, channels):
    """Pillow's decode; a warning (libjpeg's, surfaced by Pillow) is an error here"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return fz.pillow_decode(stream, channels)


def _check(what, original, stream, stats, restatement=True, sub_bits=(1024,)):
    for channels in (1, 3):
        want = _pillow(original, channels)
        got = _pillow(stream, channels)
        assert got.shape == want.shape and (got == want).all(), (what, channels, "Pillow reads another picture")
        if restatement:
            for sub in (None,) + tuple(sub_bits):
                code, mine = R.decode(stream, channels, sub)
                assert code == 0, (what, channels, sub, code)
                assert mine.shape == want.shape and (mine == want).all(), (what, channels, sub)
    name = what[0]
    kinds = W.CASES[name].get("tables", "annexk")
    if kinds == "deep":
        assert stats["long"] >= 0.9 * stats["symbols"], (what, stats)
        assert stats["sixteen"] > 0, (what, stats)
    if kinds == "flat":
        assert stats["long"] == 0, (what, stats)


@pytest.mark.parametrize("name", list(W.CASES))
def test_rewritten_streams_decode_to_the_originals_bytes(name):
    for what, original, stream, stats in W.case_streams(name):
        _check(what, original, stream, stats, sub_bits=(32, 1024))


def test_large_picture():
    """the streams that span more than one workgroup of the synchronisation kernel; the restatement runs on two of them"""
    for k, (what, original, stream, stats) in enumerate(W.big_streams()):
        assert stats["entropy"] * 8 > W.BIG_BITS, (what, stats)
        _check(what, original, stream, stats, restatement=what[0] in ("deep_pad_zeros", "flat_pad_alt"))


def test_gray_frames_that_declare_sampling_factors():
    for what, original, stream, stats in W.gray_sampling_streams():
        _check(what, original, stream, stats)


def test_the_default_rewrite_is_the_original():
    """with Annex K's tables, 1-bit padding and libjpeg's layout the rewriter returns Pillow's own bytes: what it reads and
    what it emits are the stream's, not an approximation"""
    for sampling in W.SAMPLINGS:
        o = W.original(33, 47, sampling)
        assert W.rewrap(o)[0] == o, sampling


def test_table_shapes():
    freq = {s: 100 - k for k, s in enumerate((0x00, 0x01, 0x02, 0x11, 0x21, 0x03, 0xF0, 0x12, 0x31))}
    bits, vals = W.make_table("deep", freq, False, 0)
    lengths = {}
    k = 0
    for ln, n in enumerate(bits, 1):
        for _ in range(n):
            lengths[vals[k]] = ln
            k += 1
    assert [lengths[s] for s in (0x00, 0x01, 0x02, 0x11, 0x21, 0x03, 0xF0)] == [16, 15, 14, 13, 12, 11, 10]
    assert sorted(ln for s, ln in lengths.items() if s not in freq) == list(range(2, 10))
    assert W.make_table("flat", freq, False, 0)[0] == [0] * 7 + [128, 128] + [0] * 7
    assert W.make_table("flat", {0: 1}, True, 0) == ([0, 0, 0, 12] + [0] * 12, list(range(12)))
    assert W.make_table("lean", freq, False, 0)[0][3] == 9 and len(W.make_table("unused", freq, False, 0)[1]) == 14
