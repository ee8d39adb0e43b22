"""The restatement of the PNG encoder's rules (tests/png_enc_ref.py) against decoders that know nothing of it: Pillow,
zlib and tests/png_ref.py (whose inflate applies zlib's rules for code sets), and the size caps of the encoder's tests."""
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_png_encode as fz  # noqa: E402
import png_enc_ref as ref  # noqa: E402
import png_ref  # noqa: E402

SHAPES = [(1, 1), (1, 300), (300, 1), (2, 2), (15, 17), (53, 37)]


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_streams_decode_with_pillow_zlib_and_png_ref(cn):
    k = 0
    for rows, cols in SHAPES:
        for kind in fz.KINDS:
            k += 1
            if (rows, cols) == (53, 37) or k % 3 == cn % 3:  # every content at the largest shape, a third at the others
                img = fz.content(kind, rows, cols, cn, seed=k)
                err = fz.host_arbiters(ref.encode(img, 1), img)
                assert err is None, (rows, cols, cn, kind, err)
    img = fz.content("card", 15, 17, cn)
    s0 = ref.encode(img, 0)
    assert fz.host_arbiters(s0, img) is None
    assert set(ref.block_types(s0)) == {0}
    assert ref.encode(img, 1) == ref.encode(img, 9) == ref.encode(img, 100) and ref.encode(img, -3) == s0


def test_three_blocks_and_a_row_longer_than_a_piece():
    rows, cols = 129, 255   # raw = 129 x 256 = 2 x 16384 + 256: a third block of less than one piece
    assert 2 * ref.BLOCK < ref.raw_bytes(rows, cols, 1) < 2 * ref.BLOCK + ref.PIECE
    img = fz.content("sheet", rows, cols, 1)
    s = ref.encode(img, 1)
    assert fz.host_arbiters(s, img) is None
    blocks = ref.deflate_blocks(ref.filtered(img), 1, cols, 1)
    assert len(blocks) == 3 and any(t == 2 for t, _ in blocks)
    img = fz.content("repeated row", 4, 700, 1)   # 1 + row bytes = 701 > PIECE: the row above lies two pieces back
    assert fz.host_arbiters(ref.encode(img, 1), img) is None


def test_code_sets_are_complete_with_two_codes_and_within_their_limits():
    rng = np.random.Generator(np.random.PCG64(5))
    cases = [[0] * 30, [0] * 5 + [7] + [0] * 24, [3] + [0] * 29, [0, 9] + [0] * 28, [1] * 286,
             [1 << k for k in range(15)] + [0] * 4,                 # a Fibonacci-like skew over the code-length alphabet
             [16384] + [1] * 285, list(rng.integers(0, 400, 286)), [int(1.6 ** k) for k in range(30)]]
    for freq in cases:
        for limit, longest in ((ref.LIMIT15, 15), (ref.LIMIT7, 7)):
            if longest == 7 and len(freq) > 19:
                continue
            lens = ref.code_lengths([int(v) for v in freq], limit)
            assert sum(1 for n in lens if n) >= 2 and max(lens) <= longest
            assert sum(2 ** (longest - n) for n in lens if n) == 2 ** longest, "complete"
            assert all(lens[i] for i, v in enumerate(freq) if v)
            png_ref._Huff(lens, codes=True)  # zlib's rules: raises Damaged for an over-subscribed or incomplete set


def test_size_caps():
    rows, cols = 150, 270
    for cn in (1, 3):
        raw = ref.raw_bytes(rows, cols, cn)
        size = {kind: len(ref.encode(fz.content(kind, rows, cols, cn), 1)) for kind in fz.KINDS if kind != "sheet"}
        assert all(v <= ref.bound(rows, cols, cn) for v in size.values())
        assert ref.bound(rows, cols, cn) == 43 + raw + 5 * ((raw + 16383) // 16384) + 20
        assert size["noise"] <= raw + 43 + 5 * ((raw + 16383) // 16384) + 20   # raw + the bound's documented overhead
        assert size["white"] <= raw / 30, size
        assert size["repeated row"] <= raw / 20, size
        assert size["constant rows"] <= raw / 20, size
        assert size["four-valued"] <= 0.45 * raw, size


def test_filter_bytes_and_raw_length():
    img = fz.content("gradient", 37, 53, 3)
    s = ref.encode(img, 1)
    raw = zlib.decompress(fz.chunks(s)[1][1])
    assert len(raw) == 37 * (1 + 53 * 3) and max(raw[::1 + 53 * 3]) <= 4
    assert raw == ref.filtered(img).tobytes()
