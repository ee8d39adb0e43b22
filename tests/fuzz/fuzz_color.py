"""Randomised parity run of the colour batch entry points (development aid, not part of the test suite): random shapes
with widths = 0..3 (mod 4) (staged and unstaged warp paths), candidate ranges up to 45 degrees, launch groups, the
scan-lane sweep on and off (on only where every candidate fits it), both interpolations and random per-channel borders.
Every case checks omr_batch_deskew_device_cn against the 1-channel path on the oracle's gray of the same scans (winners
equal) and against the CPU oracle's colour rotate_mat -- NEAREST exact, LINEAR within one level per channel -- and
that nothing outside a scan's canvas is written.
Usage: python tests/fuzz/fuzz_color.py [cases] [seed]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "omr-img-corrector_amd"))
import numpy as np
import torch

import oics
from oics import projection, synth
from oracle import oracle as orc

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 1))
orc.build()
dev = torch.device("cuda:0")
bad = []
lanes_cases = 0
for c in range(cases):
    rows, cols = int(rng.integers(40, 700)), int(rng.integers(40, 700))
    cols = (cols & ~3) + c % 4  # widths = 0, 1, 2, 3 (mod 4) in turn
    lanes = c % 3 == 1
    max_angle = 10 if lanes else int(rng.choice([3, 10, 20, 45]))
    step = float(rng.choice([1.0, 0.5, 0.25]))
    n = int(rng.integers(1, 7))
    group = int(rng.choice([1, 2, 4, 8]))
    interp = int(rng.integers(0, 2))
    border = tuple(int(v) for v in rng.integers(0, 256, 3)) if c % 2 else (255, 255, 255)
    skews = rng.uniform(-max_angle, max_angle, n)
    cards = np.stack([synth.make_color_card(rows, cols, 1000 * c + i, skew=float(s))[0] for i, s in enumerate(skews)])
    gray = np.stack([orc.rgb2gray(x) for x in cards])
    b = projection.Batch(rows, cols, max_angle, step, device=0, n_streams=1)
    b.set_group(group)
    if lanes:
        try:
            b.set_lanes(64)
            lanes_cases += 1
        except oics.OmrError:
            lanes = False
    dr, dc = b.deskew_canvas()
    scans = torch.from_numpy(cards).to(dev)
    g = torch.from_numpy(gray).to(dev)
    out = torch.full((n, dr, dc * 3), 7, dtype=torch.uint8, device=dev)
    size = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    best = torch.full((n,), -1, dtype=torch.int32, device=dev)
    gbest = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the batch's streams do not wait for torch's)
    b.deskew_device_cn(scans.data_ptr(), rows * cols * 3, cols * 3, 3, n, 127, interp, border, out.data_ptr(), dr * dc * 3,
                       dc * 3, size.data_ptr(), best.data_ptr())
    b.run_device(g.data_ptr(), rows * cols, cols, n, 127, gbest.data_ptr())
    b.sync()
    N = b.N
    b.close()
    o, sz, bs, gb = out.cpu().numpy(), size.cpu().numpy(), best.cpu().numpy(), gbest.cpu().numpy()
    ok = (bs == gb).all()
    for i in range(n):
        angle = (int(bs[i]) - N) * step
        exp = orc.rotate_mat(cards[i], angle, 1.0, interp, border + (0,), 1)
        er, ec = exp.shape[:2]
        got = o[i, :er, :ec * 3].reshape(er, ec, 3)
        d = np.abs(got.astype(np.int16) - exp.astype(np.int16)).max()
        ok = ok and tuple(sz[i]) == (er, ec) and d <= (0 if interp == 0 else 1)
        ok = ok and (o[i, er:, :] == 7).all() and (o[i, :, ec * 3:] == 7).all()
    if not ok:
        bad.append((c, rows, cols, max_angle, step, n, group, lanes, interp, border))
    print("case %d: %dx%d +-%d @ %.2f, %d scans, group %d, lanes %s, %s, border %s: %s" %
          (c, cols, rows, max_angle, step, n, group, lanes, "LINEAR" if interp else "NEAREST", border, "ok" if ok else "MISMATCH"))
print("fuzz_color: %d cases (%d through the scan-lane sweep), %d mismatches %s" % (cases, lanes_cases, len(bad), bad))
sys.exit(1 if bad else 0)
