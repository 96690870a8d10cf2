"""The bin sums of the three-barrier ihgp_adf8_kernel on their own copy of the lists (csrc/nagp_msr_desc.hpp: the chunks placed for few LDS bank
conflicts in the member reads) and the weights' Q | 2Q | v behind one address register.  A chunk keeps its members, their lanes and their
slots, so no sum changes a bit and what the schedule computed before it computes now: the shapes, seeds and tolerances are those of
tests/test_ihgp_adf_lean_tail.py.

  D, N      form of Q / 2Q / v     cubature
  16, 3     K4                     ut9
  32, 6     K8 (bench.py's cfg3)   ut7
  40, 4     K16-pad                ut9
  12, 2     run-time               ut9

T = 400, two sweeps.  Against the NumPy oracle (asserting first that the oracle's own sites stay below SITE_MAX, as that file does), and the
same bits between the stamped and the plain instantiation, the ring depths 4 / 8 / 16, and a batch of two against its segments."""
import numpy as np
import pytest

from test_gpu_parity import TOL_MEAN, TOL_LOGZ, rel, relz
from test_ihgp_adf_streamed_ring import _segments
import test_ihgp_adf_lean_tail as lt

pytestmark = pytest.mark.gpu

T = lt.T
_ids = dict(ids=lambda s: 'D%d-N%d' % s[:2])


@pytest.mark.parametrize('shape', lt.SHAPES, **_ids)
def test_bin_sums_against_the_oracle(shape, nagp_lib, monkeypatch, capfd):
    D, N, name = shape
    seed, link, itts = lt.SEEDS[(D, N)], lt.LINKS[0], 2
    ref = lt._oracle(D, N, seed, link, itts)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1])) and np.all(np.isfinite(ref[5]['nlZ']))
    for f in ('ttau', 'tnu'):      # the reference is determined on this problem
        s = np.asarray(ref[5][f], float)
        assert np.max(np.abs(s[np.isfinite(s)])) < lt.SITE_MAX, (f, float(np.max(np.abs(s[np.isfinite(s)]))))
    new, form = lt._public(D, N, seed, link, itts, monkeypatch, capfd)
    assert form == name, (form, name)
    fe, fv, fz = rel(new[0], ref[0]), rel(new[1], ref[1]), relz(new[5]['nlZ'], ref[5]['nlZ'])
    print('D=%d N=%d against the oracle: Eft %.2e Varft %.2e nlZ %.2e' % (D, N, fe, fv, fz))
    assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (fe, fv, fz)


@pytest.mark.parametrize('shape', lt.SHAPES, **_ids)
def test_stamped_and_plain_instantiation_give_the_same_bits(shape, nagp_lib, monkeypatch, capfd):
    D, N, name = shape
    probs, ys = _segments(D, N, T, 12600 + D, 1)
    stamped, form, _ = lt._plan(probs, ys, N, monkeypatch, capfd)
    assert form == name
    plain, _, _ = lt._plan(probs, ys, N, monkeypatch, capfd, stamps=False)
    assert np.all(np.isfinite(plain[0].Eft)) and np.all(np.isfinite(plain[0].nlZ))
    lt._same_bits(stamped[0], plain[0], shape)


@pytest.mark.parametrize('shape', lt.SHAPES[:2], **_ids)
def test_same_bits_at_every_ring_depth(shape, nagp_lib, monkeypatch, capfd):
    D, N, name = shape
    probs, ys = _segments(D, N, T, 12500 + D, 1)
    outs = {}
    for kb in (4, 8, 16):
        out, form, depth = lt._plan(probs, ys, N, monkeypatch, capfd, kb=kb)
        assert depth == kb and form == name, (kb, depth, form)
        outs[kb] = out[0]
    assert np.all(np.isfinite(outs[16].Eft)) and np.all(np.isfinite(outs[16].nlZ))
    for kb in (4, 8):
        lt._same_bits(outs[kb], outs[16], kb)


def test_a_batch_of_two_equals_the_segments_one_at_a_time(nagp_lib, monkeypatch, capfd):
    D, N = 32, 6
    probs, ys = _segments(D, N, T, 12700, 2)
    batch, form, _ = lt._plan(probs, ys, N, monkeypatch, capfd)
    assert form == 'K8'
    for q in range(2):
        one = lt._plan(probs[q:q + 1], ys[q:q + 1], N, monkeypatch, capfd)[0][0]
        lt._same_bits(batch[q], one, q)
        assert np.all(np.isfinite(one.Eft)) and np.all(np.isfinite(one.nlZ))
    assert not np.array_equal(batch[0].Eft, batch[1].Eft)      # the segments are different problems
