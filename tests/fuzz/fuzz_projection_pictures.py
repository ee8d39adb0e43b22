"""Randomised parity run of omr_projection_pictures_device / _batch_device against the restatement of the reference's
two picture functions (tests/projpic_ref.py): random shapes (1..300 per side, now and then past a column tile), the
three value classes (0 / 255, the predicates' edge values, any byte), odd buffer offsets, pitches and batch strides
over a sentinel canvas, each picture alone or both, batches of 1..5.  Every byte is compared; the pitch padding and a
guard band behind the last row must stay untouched.  Stops at the first mismatch, prints the case and exits 1.
Usage: python tests/fuzz/fuzz_projection_pictures.py [cases] [seed]"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "omr-img-corrector_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

import projpic_ref as pr
from oics import _lib

SENTINEL = 0xA5
GUARD = 64  # sentinel bytes behind the last row of a picture (and behind the last picture of a batch)


def _canvas(off, n, stride):
    return torch.full((off + n * stride + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def _picture(buf, off, i, stride, rows, cols, pitch):
    """picture i of a downloaded canvas, or an error text when a byte outside its rows' first `cols` was written"""
    blk = buf[off + i * stride:off + (i + 1) * stride]
    grid = blk[:rows * pitch].reshape(rows, pitch)
    if (grid[:, cols:] != SENTINEL).any() or (blk[rows * pitch:] != SENTINEL).any():
        return None, "wrote outside picture %d's rows" % i
    return grid[:, :cols].copy(), None


def device_pictures(imgs, so=0, sp=None, sgap=0, ho=0, hp=None, hgap=0, vo=0, vp=None, vgap=0, want_h=True, want_v=True,
                    batch=None):
    """imgs: list of (rows, cols) u8 arrays of one shape -> (list of horizontal pictures or None, list of vertical
    pictures or None, error text or None).  One image goes through omr_projection_pictures_device unless batch=True;
    buffers start so / ho / vo bytes into their allocations, rows sp / hp / vp apart, images rows * pitch + gap apart."""
    n = len(imgs)
    rows, cols = imgs[0].shape
    sp, hp, vp = (cols if v is None else v for v in (sp, hp, vp))
    sstride, hstride, vstride = rows * sp + sgap, rows * hp + hgap, rows * vp + vgap
    sbuf = np.zeros(so + n * sstride + 4, np.uint8)
    for i, a in enumerate(imgs):
        sbuf[so + i * sstride:so + i * sstride + rows * sp].reshape(rows, sp)[:, :cols] = a
    d_s = torch.from_numpy(sbuf).cuda()
    d_h = _canvas(ho, n, hstride) if want_h else None
    d_v = _canvas(vo, n, vstride) if want_v else None
    torch.cuda.synchronize()
    ph = C.c_void_p(d_h.data_ptr() + ho) if want_h else None
    pv = C.c_void_p(d_v.data_ptr() + vo) if want_v else None
    if batch or (batch is None and n > 1):
        rc = _lib.lib().omr_projection_pictures_batch_device(C.c_void_p(d_s.data_ptr() + so), n, sstride, sp, rows, cols, ph,
                                                             hstride, hp, pv, vstride, vp, None)
    else:
        rc = _lib.lib().omr_projection_pictures_device(C.c_void_p(d_s.data_ptr() + so), sp, rows, cols, ph, hp, pv, vp, None)
    torch.cuda.synchronize()
    if rc != 0:
        return None, None, "rc %d: %s" % (rc, _lib.lib().omr_last_error().decode())
    if (d_s.cpu().numpy() != sbuf).any():
        return None, None, "wrote to the source"
    out = []
    for d, off, stride, pitch in ((d_h, ho, hstride, hp), (d_v, vo, vstride, vp)):
        if d is None:
            out.append(None)
            continue
        buf = d.cpu().numpy()
        if (buf[:off] != SENTINEL).any() or (buf[off + n * stride:] != SENTINEL).any():
            return None, None, "wrote outside the canvas"
        pics = []
        for i in range(n):
            pic, err = _picture(buf, off, i, stride, rows, cols, pitch)
            if err:
                return None, None, err
            pics.append(pic)
        out.append(pics)
    return out[0], out[1], None


def run_case(rng):
    big = rng.random() < 0.1
    rows, cols = (int(v) for v in rng.integers(1, 700 if big else 120, 2))
    n = int(rng.integers(1, 6))
    cls = ("binary", "six", "any")[int(rng.integers(0, 3))]
    imgs = [pr.random_image(rng, rows, cols, cls) for _ in range(n)]
    so, ho, vo = (int(v) for v in rng.integers(0, 4, 3))
    sp, hp, vp = (cols + int(v) for v in rng.integers(0, 6, 3))
    sgap, hgap, vgap = (int(v) for v in rng.integers(0, 9, 3))
    which = int(rng.integers(0, 3))  # both, horizontal alone, vertical alone
    batch = n > 1 or rng.random() < 0.3
    case = (rows, cols, n, cls, so, sp, sgap, ho, hp, hgap, vo, vp, vgap, which, batch)
    h, v, err = device_pictures(imgs, so, sp, sgap, ho, hp, hgap, vo, vp, vgap, which != 2, which != 1, batch)
    if err:
        return case, err
    for i, a in enumerate(imgs):
        if h is not None and not np.array_equal(h[i], pr.horizontal(a)):
            return case, "horizontal picture %d: %d bytes differ" % (i, int((h[i] != pr.horizontal(a)).sum()))
        if v is not None and not np.array_equal(v[i], pr.vertical(a)):
            return case, "vertical picture %d: %d bytes differ" % (i, int((v[i] != pr.vertical(a)).sum()))
    return case, None


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
    for i in range(cases):
        case, err = run_case(rng)
        if err:
            print("case", i, case, "(rows, cols, n, class, so, sp, sgap, ho, hp, hgap, vo, vp, vgap, which, batch):", err)
            sys.exit(1)
    print("cases", cases, "mismatches 0")
    sys.exit(0)


if __name__ == "__main__":
    main()
