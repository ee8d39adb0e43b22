"""The scan-lane sweep decides every four rows how many segment slots per word it executes (slane.hpp:
slane_turn_header; tools/gen_slane_asm.py: the quarter entries of the loop bodies and their dispatch stubs).  At +-10 degrees
a word's segment count changes within a turn of 16 rows, so the waves do walk from one body into the same quarter of another
(tests/test_slane_quarter_headers.py shows on the CPU that the first two shapes hold such turns).  Bar: every candidate's f64
std-dev bit patterns and the arg-max of EVERY scan equal the CPU oracle's, in a workgroup of 16 strips x 1 scan group (64
scans) and of 4 x 4 with a scan group that holds no scans (130 scans in a context of 256 lanes), with all-black, all-white and
noise scans in the lanes; and the programs built on the device are dword-identical to the host generator's.  The third shape
has 140 rows: 11 turns, and the workgroup meets after a whole block of 64 rows."""
import numpy as np
import pytest
import torch

from oics import projection

pytestmark = pytest.mark.gpu

MAX_ANGLE, STEP = 10, 0.5
SHAPES = [(70, 100), (200, 94), (140, 131)]  # rows, cols; 94 = 30 modulo 32: the moved grid
DISTINCT = 12  # different scans of a shape (the oracle sweeps each once); the lanes hold them in a shuffled order


def make_scans(rows, cols):
    rng = np.random.Generator(np.random.PCG64(rows * 1000 + cols))
    out = [np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8)]
    for i in range(DISTINCT - 2):
        out.append(np.where(rng.random((rows, cols)) < rng.uniform(0.02, 0.7), 0, 255).astype(np.uint8))
    return out


_pool = {}


def pool(oracle, rows, cols):
    """the shape's scans and their oracle scores: computed once, never changed"""
    if (rows, cols) not in _pool:
        scans = make_scans(rows, cols)
        want = []
        for img in scans:
            evs, ehs = oracle.sweep(img, MAX_ANGLE, STEP, want_proj=False)[2:]
            want.append((evs, ehs, oracle.argmax_path1(evs, ehs)[0]))
        _pool[(rows, cols)] = (scans, want)
    return _pool[(rows, cols)]


def same_bits(x, y):
    return bool((np.ascontiguousarray(x).view(np.uint64) == np.ascontiguousarray(y).view(np.uint64)).all())


@pytest.mark.parametrize("n,lanes", [(64, 64), (130, 256)])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_quarter_dispatch_matches_the_oracle(oracle, rows, cols, n, lanes):
    scans, want = pool(oracle, rows, cols)
    pick = np.random.Generator(np.random.PCG64(n)).permutation(n) % DISTINCT
    dev = torch.device("cuda:0")
    A = projection.candidate_count(MAX_ANGLE, STEP)[1]
    buf = torch.from_numpy(np.stack([scans[k] for k in pick])).to(dev)
    best = torch.zeros(n, dtype=torch.int32, device=dev)
    vs = torch.zeros((n, A), dtype=torch.float64, device=dev)
    hs = torch.zeros((n, A), dtype=torch.float64, device=dev)
    b = projection.Batch(rows, cols, MAX_ANGLE, STEP, n_streams=1)
    b.set_lanes(lanes)
    b.run_device(buf.data_ptr(), rows * cols, cols, n, 127, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
    b.sync()
    dwords, differing = b.lanes_check_programs()
    b.close()
    assert dwords > 0 and differing == 0, "%d of %d program dwords differ from the host generator's" % (differing, dwords)
    best, vs, hs = best.cpu().numpy(), vs.cpu().numpy(), hs.cpu().numpy()
    for i, k in enumerate(pick):
        evs, ehs, ebest = want[k]
        assert same_bits(vs[i], evs), "v_sd bits, scan %d (pool scan %d)" % (i, k)
        assert same_bits(hs[i], ehs), "h_sd bits, scan %d (pool scan %d)" % (i, k)
        assert best[i] == ebest, "arg-max, scan %d (pool scan %d)" % (i, k)
