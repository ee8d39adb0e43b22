"""The 8-bit TIFF restatement (tiff8_ref.py) against Pillow's libtiff, on the CPU: it decodes Pillow's files to Pillow's
pixels, Pillow decodes its writer's files under every policy to the source, and the damage cases raise in both."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tiff8_ref as R  # noqa: E402
import tiff_ref  # noqa: E402

KINDS = ("noise", "constant", "period2", "text", "gradient")
FORMS = ((5, "tiff_lzw", 1), (5, "tiff_lzw", 2), (32773, "packbits", 1), (1, "raw", 1))


@pytest.mark.parametrize("spp", [1, 3])
def test_restatement_reads_pillows_files_and_pillow_reads_the_writers(spp):
    for kind in KINDS:
        a = R.content(kind, 33, 65, spp, seed=2)
        for comp, name, pred in FORMS:
            for rps in (7, None):
                s = R.pillow_tiff(a, name, rps, pred)
                h = R.parse(s)
                assert (h["compression"], h["predictor"], h["bps"], h["spp"]) == (comp, pred, 8, spp)
                assert (R.decode(s) == a).all() and (R.pillow_read(s) == a).all(), (kind, name, pred)
                w = R.write(a, comp, rps, pred, order=">" if rps else "<")
                assert (R.pillow_read(w) == a).all() and (R.decode(w) == a).all(), (kind, name, pred)


@pytest.mark.parametrize("policy", R.POLICIES)
def test_pillow_reads_every_writer_policy(policy):
    a = R.content("noise", 70, 53, 3, seed=1)  # about 11 k codes in one strip: every width, the table filled more than once
    codes = R.lzw_codes(a.tobytes(), policy, 3)
    assert len(codes) > 2 * 3836 and codes.count(R.CLEAR) >= 3
    s = R.write(a, 5, policy=policy, seed=3)
    assert (R.pillow_read(s) == a).all() and (R.decode(s) == a).all()
    c = R.content("constant", 40, 257, 1)
    s = R.write(c, 5, policy=policy, seed=4, predictor=2)
    assert (R.pillow_read(s) == c).all() and (R.decode(s) == c).all()


def test_photometric_0_is_inverted_and_predictor_2_counts_with_lzw_alone():
    a = np.full((2, 5), 10, np.uint8)
    s = tiff_ref.assemble(2, 5, [a.tobytes()], 1, photometric=0, extra=[(258, 3, [8])])  # stored 10
    assert R.pillow_read(s)[0, 0] == 245 and R.decode(s)[0, 0] == 245
    g = R.content("gradient", 3, 9, 1)
    for comp in (1, 32773):  # libtiff knows the tag with LZW and Deflate alone
        strips = [g.tobytes()] if comp == 1 else [b"".join(R.packbits_encode(r) for r in g)]
        s = tiff_ref.assemble(3, 9, strips, comp, photometric=1, extra=[(258, 3, [8]), (317, 3, [2])])
        assert (R.pillow_read(s) == g).all() and (R.decode(s) == g).all() and R.parse(s)["predictor"] == 1


def damaged_strips(raw):
    """{name: a strip that neither libtiff nor the decoder reads to `raw`'s length}"""
    codes = R.lzw_codes(raw)
    full = R.lzw_codes(R.content("noise", 100, 100, 1, 9).tobytes(), "late")
    k = full.index(R.CLEAR, 1)
    return {"no leading Clear": R.pack_codes(codes[1:]), "a code beyond the table": R.pack_codes(codes[:5] + [300] + codes[6:]),
            "truncated": R.pack_codes(codes)[:len(R.pack_codes(codes)) // 2], "no literal after Clear": R.pack_codes([256, 258] + codes[2:]),
            "EOI before the rows are full": R.pack_codes(codes[:len(codes) // 2] + [R.EOI]),
            "the table pushed past 4095": R.pack_codes(full[:k] + full[k + 1:])}


def test_damage_raises_in_both():
    good = R.content("text", 8, 20, 1, seed=5)
    for name, strip in damaged_strips(good.tobytes()).items():
        rows, cols = (100, 100) if "4095" in name else (8, 20)
        s = tiff_ref.assemble(rows, cols, [strip], 5, photometric=1, extra=[(258, 3, [8])])
        with pytest.raises(Exception):
            R.pillow_read(s)
        with pytest.raises(R.Damaged):
            R.decode(s)


def test_what_libtiff_reads_is_read():
    a = R.content("text", 8, 20, 1, seed=5)
    codes = R.lzw_codes(a.tobytes())
    more = R.lzw_codes(a.tobytes() + bytes(range(40)))   # output left over after the rows
    for name, cs in (("Clears in a row", [256, 256] + codes[1:]), ("output left over", more), ("codes behind the rows", codes[:-1] + [511, 400, 257])):
        s = tiff_ref.assemble(8, 20, [R.pack_codes(cs)], 5, photometric=1, extra=[(258, 3, [8])])
        assert (R.pillow_read(s) == a).all() and (R.decode(s) == a).all(), name
