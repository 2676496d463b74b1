"""The matte refinement without a GPU: the statement of DESIGN.md section 36 (tests/refine_restatement.py) held against SciPy's uniform filter,
its cofactor solve against `np.linalg.solve`, its identities (an all-0 and an all-255 plane come back as they are, a constant guide gives no
NaN), the thing a guided upsampling must do (come closer to the true alpha at hair-like edges than the bilinear resize does), the cases with large
coefficients and with neighbouring bytes, and the host half of `maggie_amd.utils.refine` and of its wiring (argument checks before any device is
touched)."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import refine_restatement as R                              # noqa: E402
from maggie_amd import hip                                  # noqa: E402
from maggie_amd.utils import cutout, matteout, refine       # noqa: E402


def test_constants_are_the_header_s():
    text = open(os.path.join(ROOT, 'include', 'maggie_hip.h')).read()
    assert '#define MG_REFINE_MAX_RADIUS %d' % refine.MAX_RADIUS in text
    assert '#define MG_REFINE_MIN_EPS 1e-6' in text and refine.MIN_EPS == 1e-6
    assert '#define MG_CUTOUT_MAX_SIDE %d' % refine.MAX_SIDE in text
    assert (refine.RADIUS, refine.EPS) == (R.RADIUS, R.EPS) == (5, 1e-4)


@pytest.mark.parametrize('shape', [(13, 17), (1, 1)])
def test_window_sums_are_scipy_s_mirror_filter(shape):
    rng = np.random.RandomState(3)
    p = rng.randint(-(2 ** 20), 2 ** 20, shape)                 # the second window adds signed fixed-point coefficients
    for r in (1, 2, 3, 5, 64):
        got = R.window_sums(p, r)
        want = ndimage.uniform_filter(p.astype(np.float64), size=r, mode='mirror') * (r * r)
        assert got.dtype == np.int64 and got.shape == shape
        assert np.allclose(got, want, rtol=0, atol=0.5), (shape, r)                     # integers: equal


def test_cofactor_solve_is_numpy_s():
    rng = np.random.RandomState(7)
    for _ in range(1000):
        M = rng.uniform(-1, 1, (3, 3))
        S = M @ M.T + 1e-3 * np.eye(3)
        k = rng.uniform(-1, 1, 3)
        s = {q: np.float64(S[q]) for q in R.PAIRS}
        got = np.array(R.solve3(s, [np.float64(v) for v in k]))
        assert np.allclose(got, np.linalg.solve(S, k), rtol=1e-9, atol=0)


def test_constant_planes_come_back_and_a_constant_guide_gives_no_nan():
    rng = np.random.RandomState(5)
    I = rng.randint(0, 256, (23, 31, 3)).astype(np.uint8)
    G = rng.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    for v in (0, 255):
        for r, eps in ((5, 1e-4), (1, 1e-6), (64, 1.0)):
            assert (R.refine(I, G, np.full((9, 11), v, np.uint8), r, eps) == v).all(), (v, r, eps)
    p = rng.randint(0, 256, (9, 11)).astype(np.uint8)
    flat = np.full((9, 11, 3), 77, np.uint8)
    for r, eps in ((5, 1e-4), (3, 1e-6)):
        A, B, amax = R.coefficients(flat, p, r, eps)
        m = R.means(A, B, r)
        assert np.isfinite(m).all() and np.isfinite(amax)
        assert not A.any()                                      # no variance in the guide: a = 0 and b is the window mean of p
        out = R.refine(np.full((23, 31, 3), 77, np.uint8), flat, p, r, eps)
        assert out.dtype == np.uint8 and out.shape == (23, 31)


def test_the_filter_halves_the_error_of_the_bilinear_resize():
    I, G, p, a = R.scene()
    assert I.shape == (480, 640, 3) and G.shape == (120, 160, 3) and p.shape == (120, 160)
    mixed = (a > 12) & (a < 243)
    assert mixed.sum() == 5150
    true = a.astype(np.float64)
    got = R.refine(I, G, p, 5, 1e-4)
    plain = np.floor(np.clip(R.bilinear_up(p.astype(np.float64) / 255.0, 480, 640), 0.0, 1.0) * 255.0 + 0.5)
    err, err_plain = np.abs(got[mixed] - true[mixed]).mean(), np.abs(plain[mixed] - true[mixed]).mean()
    print('mean absolute error against the true alpha over %d mixed pixels: filter %.2f, bilinear %.2f grey levels' % (mixed.sum(), err, err_plain))
    assert err <= 0.5 * err_plain


def step_case():
    """An 8 x 8 guide of 100 whose channel 0 is 101 from column 4 on, under a 0 / 255 alpha step there: one grey level explains the whole step."""
    G = np.full((8, 8, 3), 100, np.uint8)
    G[:, 4:, 0] = 101
    p = np.zeros((8, 8), np.uint8)
    p[:, 4:] = 255
    return G, p


def test_large_coefficients_stay_inside_the_guards():
    G, p = step_case()
    out, amax = R.refine(G, G, p, 3, 1e-6, with_max=True)
    print('largest unclipped |a|: %.1f' % amax)
    assert 128 < amax < 250                                     # the bound 0.25 / sqrt(eps) = 250 holds: the clip at 256 does not act
    A, B, _ = R.coefficients(G, p, 3, 1e-6)
    assert np.abs(A).max() < 256 * 65536 and np.abs(B).max() < 1024 * 65536
    assert out.dtype == np.uint8 and out.min() == 0 and out.max() == 255


def test_neighbouring_bytes_under_snap():
    """Output bytes 0, 1, 254 and 255: at radius 1 and the largest eps the filter is almost the identity on a flat guide."""
    G = np.full((1, 8, 3), 50, np.uint8)
    p = np.array([[0, 1, 2, 128, 253, 254, 255, 1]], np.uint8)
    plain = R.refine(G, G, p, 1, 1.0)
    assert plain.tolist() == p.tolist()
    assert {0, 1, 254, 255} <= set(plain.ravel().tolist())
    assert R.refine(G, G, p, 1, 1.0, snap=True).tolist() == [[0, 0, 2, 128, 253, 255, 255, 0]]


def test_axis_tables_are_the_statement_s():
    for src, dst in ((1, 1), (1, 3), (5, 11), (7, 4), (9, 9), (64, 131), (576, 2160)):
        i0, i1, f = R.axis(src, dst)
        gi, gf = refine._axis(src, dst)
        assert gi.dtype == np.int32 and gf.dtype == np.float64
        assert np.array_equal(gi, i0) and np.array_equal(gf, f)
        assert i0.min() >= 0 and i1.max() <= src - 1 and f.min() >= 0.0 and f.max() < 1.0


def test_argument_checks_come_before_the_device():
    fr = np.zeros((4, 6, 3), np.uint8)
    a8 = torch.zeros((2, 2, 3), dtype=torch.uint8)
    af = torch.zeros((2, 4, 6), dtype=torch.float32)
    with pytest.raises(TypeError):
        refine.refine(fr.astype(np.float32), a8)
    with pytest.raises(TypeError):
        refine.refine(fr, np.zeros((2, 2, 3), np.uint8))                                 # the alpha is a tensor
    with pytest.raises(TypeError):
        refine.refine(fr, a8.double())
    with pytest.raises(TypeError):
        refine.refine(fr, a8, radius=5.0)
    with pytest.raises(TypeError):
        refine.refine(fr, a8, eps='small')
    with pytest.raises(TypeError):
        refine.refine(fr, a8, guide=np.zeros((2, 3, 3), np.float32))
    for radius in (0, 65, -1):
        with pytest.raises(ValueError):
            refine.refine(fr, a8, radius=radius)
    for eps in (0.0, 9e-7, 1.5, float('nan')):
        with pytest.raises(ValueError):
            refine.refine(fr, a8, eps=eps)
    with pytest.raises(ValueError):
        refine.refine(fr, a8[0, 0])
    with pytest.raises(ValueError):
        refine.refine(np.zeros((3, 4, 6, 3), np.uint8), a8)                              # two planes do not make three frames
    with pytest.raises(ValueError):
        refine.refine(fr, a8, guide=np.zeros((2, 4, 3), np.uint8))                       # a guide of another size
    with pytest.raises(ValueError):
        refine.refine(fr, af, transform_info=[{'name': 'resize', 'ori_size': (9, 9)}])   # comes out at another size
    with pytest.raises(ValueError):
        refine.refine(fr, af, transform_info=[{'name': 'resize', 'ori_size': (4, 6)}, {'name': 'padding', 'pad_size': (4, 0)}])   # nothing left
    with pytest.raises(ValueError):
        refine.refine(fr, af, transform_info=[{'name': 'resize', 'ori_size': (4, 6), 'ratio': 0.5}, {'name': 'padding', 'pad_size': (1, 1)}])
    for bad in ({'radius': 0}, {'eps': 2.0}, {'side': 3}):
        with pytest.raises(ValueError):
            cutout.cutout(fr, af, refine=bad)
        with pytest.raises(ValueError):
            matteout.predict_image(None, fr, np.zeros((4, 6), np.uint8), refine=bad)
    for bad in (5, 'yes', {'radius': 2.5}):
        with pytest.raises(TypeError):
            cutout.cutout(fr, af, refine=bad)
        with pytest.raises(TypeError):
            matteout.predict_image(None, fr, np.zeros((4, 6), np.uint8), refine=bad)
    with pytest.raises(ValueError):
        cutout.cutout(fr, af, refine=True, radii=(0, 6))
    assert refine.options(False) is None and refine.options(None) is None and refine.options(True) == {}
    assert refine.options({'radius': 3, 'eps': 1e-6}) == {'radius': 3, 'eps': 1e-6}


def test_no_gpu_means_an_error_not_a_fallback():
    if torch.cuda.is_available():
        return
    fr = np.zeros((4, 6, 3), np.uint8)
    a8 = torch.zeros((2, 2, 3), dtype=torch.uint8)
    for fn in (lambda: refine.refine(fr, a8), lambda: refine.refine(fr, a8, as_float=True, snap=True),
               lambda: cutout.cutout(fr, a8, refine=True), lambda: cutout.cutout(fr, a8, refine={'radius': 3})):
        with pytest.raises(hip.MaggieHipError):
            fn()
