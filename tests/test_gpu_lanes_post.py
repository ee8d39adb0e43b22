"""What runs behind the scan-lane sweep (slane.hip: slane_stddev_kernel): the std-dev kernel reads
the column counts straight from the waves' counter dumps and the row counts from their accumulators, which it leaves zero
for the next launch on that scratch set.  Bar: bit-exact against the CPU oracle -- integer projections of EVERY candidate,
f64 std-dev bit patterns and the arg-max of every scan -- at shapes that hit one strip, a moved grid with short first and
last words, a last strip of one word and off = 0, and across launches of different sizes on one context."""
import numpy as np
import pytest
import torch

import oics
from oics import projection

pytestmark = pytest.mark.gpu


def make_scans(rows, cols, n, seed):
    """n different binary scans: random dots of every density, some with rules, a white and a black one"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        img = np.where(rng.random((rows, cols)) < rng.uniform(0.02, 0.7), 0, 255).astype(np.uint8)
        if i % 3 == 1:
            img[rng.integers(0, rows, 5), :] = 0
            img[:, rng.integers(0, cols, 4)] = 0
        if i % 29 == 7:
            img[:] = 255 if i % 2 else 0
        out.append(img)
    return out


class Lanes:
    """One scan-lane context and its device buffers"""

    def __init__(self, rows, cols, max_angle, step, lanes):
        self.rows, self.cols, self.lanes = rows, cols, lanes
        self.A = projection.candidate_count(max_angle, step)[1]
        self.dev = torch.device("cuda:0")
        self.b = projection.Batch(rows, cols, max_angle, step, n_streams=1)
        self.b.set_lanes(lanes)

    def run(self, scans):
        n = len(scans)
        buf = torch.from_numpy(np.stack(scans)).to(self.dev)
        best = torch.zeros(n, dtype=torch.int32, device=self.dev)
        vs = torch.zeros((n, self.A), dtype=torch.float64, device=self.dev)
        hs = torch.zeros((n, self.A), dtype=torch.float64, device=self.dev)
        self.b.run_device(buf.data_ptr(), self.rows * self.cols, self.cols, n, 127, best.data_ptr(), vs.data_ptr(), hs.data_ptr())
        self.b.sync()
        return best.cpu().numpy(), vs.cpu().numpy(), hs.cpu().numpy()

    def close(self):
        self.b.close()


def same_bits(x, y):
    return bool((np.ascontiguousarray(x).view(np.uint64) == np.ascontiguousarray(y).view(np.uint64)).all())


@pytest.mark.parametrize("rows,cols,max_angle,step,n", [
    (70, 45, 10, 2.5, 3),    # one strip
    (97, 95, 9, 1.5, 65),    # width = 31 modulo 32: the grid is moved, the first and the last word are short
    (80, 150, 6, 1.0, 70),   # five destination words: the last strip has one real word
    (64, 64, 10, 5.0, 64),   # off = 0, rows a multiple of 64
])
def test_every_column_and_row_of_every_candidate(oracle, rows, cols, max_angle, step, n):
    scans = make_scans(rows, cols, n, 7 * rows + cols)
    L = Lanes(rows, cols, max_angle, step, 64 * ((n + 63) // 64))
    L.b.lanes_keep(True)
    best, vs, hs = L.run(scans)
    probes = sorted({0, n - 1, 64 * ((n - 1) // 64) + ((n - 1) % 64) // 2, n // 2})  # first lane, last lane, one in the last (partial) group, one in the middle
    proj = {(i, a): L.b.lanes_projections(i, a, rows, cols) for i in probes for a in range(L.A)}
    L.close()
    for i, img in enumerate(scans):
        evp, ehp, evs, ehs = oracle.sweep(img, max_angle, step)
        if i in probes:
            for a in range(L.A):
                assert (proj[(i, a)][0] == evp[a]).all(), "column counts, scan %d candidate %d" % (i, a)
                assert (proj[(i, a)][1] == ehp[a]).all(), "row counts, scan %d candidate %d" % (i, a)
        assert same_bits(vs[i], evs), "v_sd bits, scan %d" % i
        assert same_bits(hs[i], ehs), "h_sd bits, scan %d" % i
        assert best[i] == oracle.argmax_path1(evs, ehs)[0]


def test_row_counts_are_cleared_by_their_reader(oracle):
    """Launches of different sizes on one context of 512 lanes: the two scratch sets alternate, so each is used again
    after a smaller launch.  A launch of 320 scans sweeps whole quads of scan groups -- groups 5-7 hold the bit images of
    the 512 scans before it, and their row counts must be gone before the next 512 -- and a launch of 1 or 70 scans
    leaves most of the set untouched.  Every scan of every launch against the oracle."""
    rows, cols, max_angle, step = 60, 90, 6, 1.0
    pool = make_scans(rows, cols, 1024, 99)
    ref = [oracle.sweep(img, max_angle, step, want_proj=False)[2:] for img in pool]
    refbest = [oracle.argmax_path1(v, h)[0] for v, h in ref]
    rng = np.random.Generator(np.random.PCG64(3))
    L = Lanes(rows, cols, max_angle, step, 512)
    # sets 0 1 0 1 0 1 | 0 1 0 1: the last four put 320 scans behind 512 on set 1, and 512 behind those
    for call, n in enumerate((512, 320, 512, 70, 1, 512, 512, 320, 1, 512)):
        pick = rng.permutation(len(pool))[:n]
        best, vs, hs = L.run([pool[k] for k in pick])
        for i, k in enumerate(pick):
            assert same_bits(vs[i], ref[k][0]) and same_bits(hs[i], ref[k][1]), "call %d (%d scans), scan %d" % (call, n, i)
            assert best[i] == refbest[k]
    L.close()


def test_keep_on_off_on(oracle):
    """The same 130 scans again and again on one context while omr_batch_lanes_keep is switched: the scores never change,
    the row counts are the oracle's whenever keep is on (also on a set whose launch before cleared by itself, and on one
    that was left dirty), and are refused when it is off."""
    rows, cols, max_angle, step, n = 75, 110, 6, 1.0, 130
    scans = make_scans(rows, cols, n, 11)
    probes = (0, 63, 64, 129)
    want = {i: oracle.sweep(scans[i], max_angle, step) for i in probes}
    L = Lanes(rows, cols, max_angle, step, 192)
    first = None
    for call, keep in enumerate((True, False, True, True, False, False, True)):
        L.b.lanes_keep(keep)
        best, vs, hs = L.run(scans)
        if first is None:
            first = (best, vs, hs)
            for i in probes:
                assert same_bits(vs[i], want[i][2]) and same_bits(hs[i], want[i][3])
        assert (best == first[0]).all() and same_bits(vs, first[1]) and same_bits(hs, first[2]), "call %d" % call
        for i in probes:
            for a in (0, L.A // 2, L.A - 1):
                if keep:
                    vp, hp = L.b.lanes_projections(i, a, rows, cols, scratch_set=call % 2)
                    assert (vp == want[i][0][a]).all() and (hp == want[i][1][a]).all(), "call %d scan %d candidate %d" % (call, i, a)
                else:
                    with pytest.raises(oics.OmrError):
                        L.b.lanes_projections(i, a, rows, cols, scratch_set=call % 2)
    L.close()


def test_column_counts_without_keep(oracle):
    rows, cols, max_angle, step, n = 80, 150, 6, 1.0, 70
    scans = make_scans(rows, cols, n, 5)
    L = Lanes(rows, cols, max_angle, step, 128)
    L.run(scans)
    for i in (0, 64, 69):
        evp = oracle.sweep(scans[i], max_angle, step)[0]
        for a in range(L.A):
            vp, hp = L.b.lanes_projections(i, a, rows, cols, want_rows=False)
            assert hp is None and (vp == evp[a]).all(), "column counts, scan %d candidate %d" % (i, a)
    L.close()
