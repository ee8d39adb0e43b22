"""The crafted canvases of tests/jpeg_cases.py, on the restatement alone: what they make libjpeg's entropy coder write.
tests/test_gpu_jpeg_symbols.py compares the device encoder and decoder with Pillow on these canvases; the conditions here
are what makes that comparison worth its name -- every Huffman symbol libjpeg can be made to write is in some stream, and
the restatement that says so writes Pillow's bytes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_jpeg as fz  # noqa: E402
import jpeg_cases as jc  # noqa: E402
import jpeg_ref  # noqa: E402

# What chroma_canvas reaches of the chroma AC table, measured with symbols() over CHROMA_QUALITIES: the union of the sets
# written with table 1 by the five chroma-q* canvases.  All 162: the sizes 9 and 10, which Cb and Cr cannot reach at
# constant Y, come from the cells of two extreme colours (blue / yellow, red / cyan).
CHROMA_AC_REACHED = 162
CHROMA_AC_UNREACHED = ()

# The longest block among the crafted canvases, in bits: max over cases() of symbols().max_block_bits.  It is a block of
# the binary canvases (every pixel 0 or 255), its DC code included.  The suite's 150 x 270 noise at quality 100
# (tests/test_gpu_jpeg.py): 875 bits in gray, 801 in colour, by the same function.  The margin is the difference of the two measurements.
LONGEST_BLOCK_BITS = 987
NOISE_LONGEST_BLOCK_BITS = 875
LONGEST_BLOCK_MARGIN = LONGEST_BLOCK_BITS - NOISE_LONGEST_BLOCK_BITS

ALL_CASES = jc.names()


def _sym(name):
    return jc.symbols_of(jc.case_blocks(name))


def _stream(name):
    _, img, q = jc.case(name)
    cn = 1 if img.ndim == 2 else 3
    return jpeg_ref.header(img.shape[0], img.shape[1], cn, q) + jpeg_ref.entropy(jc.case_blocks(name), cn) + b"\xff\xd9"


@pytest.mark.parametrize("name", ALL_CASES)
def test_restatement_equals_pillow(name):
    """the restatement and libjpeg agree on every crafted canvas at its quality before either judges the kernel; and the
    walk the histogram is taken from has block_bits' lengths"""
    _, img, q = jc.case(name)
    assert max(img.shape[:2]) <= 528
    got = _stream(name)
    assert got == jpeg_ref.encode(img, q)
    want = fz.pillow_bytes(img, q)
    assert got == want, jc.explain(img, q, got, want)
    dc = [jpeg_ref.huff_codes(jpeg_ref.DC_LUMA), jpeg_ref.huff_codes(jpeg_ref.DC_CHROMA)]
    ac = [jpeg_ref.huff_codes(jpeg_ref.AC_LUMA), jpeg_ref.huff_codes(jpeg_ref.AC_CHROMA)]
    blocks = jc.case_blocks(name)
    for (comp, blk), (_, t, diff, walk) in list(zip(blocks, jc.scan_walk(blocks)))[::7]:
        assert sum(w[3] for w in walk) == len(jpeg_ref.block_bits(blk, diff, dc[t], ac[t]))


@pytest.mark.parametrize("name,img,q", jc.crops(), ids=[c[0] for c in jc.crops()])
def test_restatement_equals_pillow_on_the_crops(name, img, q):
    got, want = jpeg_ref.encode(img, q), fz.pillow_bytes(img, q)
    assert got == want, jc.explain(img, q, got, want)
    assert all(n % 8 == 1 for n in img.shape[:2])


def test_gray_canvases_write_every_luma_ac_symbol():
    reached, zrls = set(), set()
    for name in jc.names(colour=False):
        s = _sym(name)
        assert not s.ac[1] and not s.dc[1]
        reached |= s.ac[0]
        zrls |= s.zrl_counts
    assert reached == jc.ALL_AC, sorted(hex(v) for v in jc.ALL_AC - reached)
    assert {0, 1, 2, 3} <= zrls


def test_basis_canvases_alone_write_every_luma_ac_symbol():
    """the construction as measured over BASIS_QUALITIES: the saturated form reaches 162 of 162; the unsaturated form 155,
    all but (0, 10), (3, 10), (7, 10), (10, 10), (11, 10), (14, 10), (15, 10) -- a size-10 coefficient at those positions
    leaves 0..255 at every quality"""
    reached = {"basis-q%d": set(), "basis-sat-q%d": set()}
    for form in reached:
        for q in jc.BASIS_QUALITIES:
            reached[form] |= _sym(form % q).ac[0]
            img = jc.case(form % q)[1]
            assert img.shape[1] == 256 and img.shape[0] <= 320
        print(form, len(reached[form]), sorted(hex(v) for v in jc.ALL_AC - reached[form]))
    assert reached["basis-sat-q%d"] == jc.ALL_AC
    assert jc.ALL_AC - reached["basis-q%d"] <= {0x0A, 0x3A, 0x7A, 0xAA, 0xBA, 0xEA, 0xFA}


def test_dc_categories_0_to_11_in_both_tables_with_both_signs():
    signed = [set(), set()]
    for name in ALL_CASES:
        s = _sym(name)
        for t in (0, 1):
            signed[t] |= s.dc_signed[t]
    for t in (0, 1):
        assert signed[t] == set(range(-11, 12)), (t, sorted(set(range(-11, 12)) - signed[t]))
    # the staircases alone, per table; the chroma canvas's flat cells swing -1024 .. +1016 in Y, Cb and Cr
    stairs = [set(), set()]
    for q in jc.STAIR_QUALITIES:
        stairs[0] |= _sym("stair-q%d" % q).dc_signed[0]
        stairs[1] |= _sym("stair-colour-q%d" % q).dc_signed[1]
    assert stairs[0] == stairs[1] == set(range(-11, 12))
    s = _sym("chroma-q100")
    assert {-11, 11} <= s.dc_signed[0] and {-11, 11} <= s.dc_signed[1]
    dcs = [[int(b[0]) for c, b in jc.case_blocks("chroma-q100") if c == comp] for comp in range(3)]
    for comp in range(3):
        assert min(dcs[comp]) == -1024 and max(dcs[comp]) == 1016, comp


def test_staircase_predicts_across_row_ends_and_the_256_block_segment():
    """gray, 20 blocks a row: a difference of category 10 or 11 at the first block of some row, and at block 256 -- the first
    of the device's second scan segment, predicted from the last block of the first"""
    blocks = jc.case_blocks("stair-q100")
    assert len(blocks) == 320
    cats = [jc._nbits(d) for _, _, d, _ in jc.scan_walk(blocks)]
    assert max(cats[b] for b in range(20, 320, 20)) >= 10
    assert cats[256] >= 10
    # colour: block 256 is the Cb block of MCU 42; the MCUs around the boundary hold differences of category 10 or 11 too
    walk = jc.scan_walk(jc.case_blocks("stair-colour-q100"))
    assert max(jc._nbits(d) for _, _, d, _ in walk[250:262]) >= 10
    assert max(jc._nbits(walk[6 * m][2]) for m in range(20, 320, 20)) >= 10


def test_chroma_canvases_reach_the_chroma_ac_table():
    reached = set()
    for q in jc.CHROMA_QUALITIES:
        reached |= _sym("chroma-q%d" % q).ac[1]
    small = {(r << 4) | s for r in range(16) for s in range(1, 9)} | {0x00, 0xF0}
    assert small - set(CHROMA_AC_UNREACHED) <= reached, sorted(hex(v) for v in small - reached)
    assert not set(CHROMA_AC_UNREACHED) & small          # none of size <= 8 had to be given up
    assert len(reached) >= CHROMA_AC_REACHED and len(reached) + len(CHROMA_AC_UNREACHED) == 162
    assert reached == jc.ALL_AC - set(CHROMA_AC_UNREACHED)


def test_zrl_canvas():
    for q in jc.ZRL_QUALITIES:
        blocks = jc.case_blocks("zrl-q%d" % q)
        s = jc.symbols_of(blocks)
        assert {1, 2, 3} <= s.zrl_counts and s.max_zrl == 3
        no_eob = 0
        for _, blk in blocks:
            assert set(np.flatnonzero(blk[1:]) + 1) <= set(jc.ZRL_POSITIONS)
            no_eob += blk[63] != 0
        assert no_eob >= 8
        kinds = [[w[0] for w in walk] for _, _, _, walk in jc.scan_walk(blocks)]
        assert ["dc", "zrl", "zrl", "zrl", "ac"] in kinds                # 63 alone: three ZRLs, (14, s), no EOB
        assert ["dc", "zrl", "ac", "ac", "ac", "ac"] in kinds            # all four: ZRL (0, s), then (15, s) twice, (13, s)
        assert ["dc", "zrl", "ac", "zrl", "zrl", "ac"] in kinds          # 17 and 63: a ZRL, then two more inside the block
        assert ["dc", "zrl", "ac", "eob"] in kinds and ["dc", "zrl", "zrl", "ac", "eob"] in kinds
        assert ["dc", "zrl", "zrl", "zrl", "ac", "eob"] in kinds         # 49 alone


def test_crafted_blocks_are_longer_than_the_noise():
    longest = max(_sym(name).max_block_bits for name in ALL_CASES)
    noise = max(jc.symbols(jc.noise(cn), 100).max_block_bits for cn in (1, 3))
    print("longest crafted block", longest, "noise", noise)
    assert noise == NOISE_LONGEST_BLOCK_BITS
    assert longest == LONGEST_BLOCK_BITS == max(_sym(n).max_block_bits for n in ("binary-q100", "binary-colour-q100"))
    assert longest - noise >= LONGEST_BLOCK_MARGIN > 0
    assert longest <= 11 + 11 + 63 * (16 + 10)      # kMaxBlockBits of csrc/oics_jpeg.cpp


def test_stuffed_bytes_at_every_position_of_a_16_byte_span():
    """jpeg_ff_kernel and jpeg_stream_kernel give a thread 16 bytes of the unstuffed scan"""
    everywhere, across, last = [], [], []
    for name in ALL_CASES:
        _, raw = jc.scan_of(_stream(name))
        at = np.flatnonzero(np.frombuffer(raw, np.uint8) == 255)
        if len(set(at % 16)) == 16:
            everywhere.append(name)
        both = set(at) & set(at + 1)                  # i: bytes i - 1 and i are 0xFF
        if any(i % 16 == 0 for i in both):
            across.append(name)
        if raw[-1] == 255:
            last.append(name)
    print("every position:", everywhere, "\nacross a boundary:", across, "\nlast byte:", last)
    assert set(everywhere) & set(across), "no single stream has both"
    assert "stair-q100" in last
    assert len(everywhere) >= 10
    # dense: in the saturated basis canvas at quality 100 more than one unstuffed byte in 16 is 0xFF
    _, raw = jc.scan_of(_stream("basis-sat-q100"))
    assert raw.count(b"\xff") * 16 > len(raw)


def test_crops_put_dummy_blocks_beside_category_11():
    """in a BGR crop of 16 k + 1 columns (rows) the right (lower) Y blocks of the last MCUs are dummies; some MCU with
    dummies holds a real Y block whose DC difference is of category 11"""
    right = below = 0
    for name, img, q in jc.crops():
        if img.ndim != 3:
            continue
        rows, cols = img.shape[:2]
        mw, mh = -(-cols // 16), -(-rows // 16)
        walk = jc.scan_walk(jpeg_ref.scan_blocks(img, q))
        assert len(walk) == 6 * mw * mh
        for m in range(mw * mh):
            my, mx = divmod(m, mw)
            cat = max(jc._nbits(walk[6 * m + k][2]) for k in range(4))
            if cat == 11 and mx == mw - 1 and cols % 16 == 1:
                right += 1
            if cat == 11 and my == mh - 1 and rows % 16 == 1:
                below += 1
    print("MCUs with a category-11 Y block and dummies to the right:", right, "below:", below)
    assert right >= 2 and below >= 2


def test_explain_names_the_block_and_the_symbol():
    _, img, q = jc.case("zrl-q50")
    want = _stream("zrl-q50")
    start, _ = jc.scan_of(want)
    got = bytearray(want)
    got[start + 40] ^= 0x10
    msg = jc.explain(img, q, bytes(got), want)
    assert "byte %d " % (start + 40) in msg and "block " in msg and "symbol 0x" in msg, msg
    assert "header" in jc.explain(img, q, want[:100] + b"\x00" + want[101:], want)
    assert "first difference at byte %d" % (len(want) - 5) in jc.explain(img, q, want[:-5], want)
