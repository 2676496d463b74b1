"""The host side of the device background chain (maggie_amd.utils.background) and the restatement the device is compared with
(tests/background_restatement.py): the draws against the reference's sequence of calls, the taps, the integer blur against scipy's fp64
correlation within a bound computed from the taps' own quantisation error, the bincount curves against the np.unique / np.interp statement,
the table composite against the literal expression on all 256^3 triples, the fixture, and the order of the errors. No GPU is needed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import background_restatement as R                                    # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import background as B                          # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_background_golden as G                                    # noqa: E402


def _same_position(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------------------
def test_draw_path_is_the_generators_choice():
    paths = ['bg_%d.jpg' % i for i in range(37)]
    for seed in range(20):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        assert B.draw_path(a, paths) == b.choice(paths) and _same_position(a, b)


def test_draw_window_consumes_the_generator_as_the_reference_does():
    fired = unfired = 0
    seen = set()
    for seed in range(200):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        d = B.draw_window(a, (50, 71), (20, 30)) if seed % 2 else B.draw_window(a, (50, 71), (20, 30), 0.5, [5, 15, 25], [1.0, 1.5, 3.0, 5.0])
        blur, x, y = R.window_calls(b, (50, 71), (20, 30))
        assert _same_position(a, b)
        assert (d.x, d.y, d.h, d.w) == (x, y, 20, 30) and 0 <= x < 71 - 30 and 0 <= y < 50 - 20
        assert d.blurred == (blur is not None) and not d.on_device
        if blur is None:
            unfired += 1
            assert d.taps is None and list(d.win[:5]) == [1, x, y, 0, 256] and not d.win[5:].any()
        else:
            fired += 1
            seen.add(blur)
            q = R.taps(*blur)
            assert np.array_equal(d.taps, q) and d.taps.dtype == np.int32
            assert list(d.win[:4]) == [blur[0], x, y, 0] and np.array_equal(d.win[4:4 + blur[0]], q) and not d.win[4 + blur[0]:].any()
    assert fired > 60 and unfired > 60 and len(seen) == 12                 # both branches, every pair of the reference's lists
    # the number of doubles and integers drawn: rand, [choice, choice], randint, randint
    for seed in range(20):
        a, c = np.random.RandomState(seed), np.random.RandomState(seed)
        B.draw_window(a, (9, 9), (3, 4), blur_p=1.0)
        c.rand(); c.choice([5, 15, 25]); c.choice([1.0, 1.5, 3.0, 5.0]); c.randint(0, 5); c.randint(0, 6)   # noqa: E702
        assert _same_position(a, c)


@pytest.mark.parametrize('bg_hw', [(20, 31), (21, 30), (20, 30)], ids=['equal_height', 'equal_width', 'equal'])
def test_draw_window_raises_at_equal_sizes_as_the_reference_does(bg_hw):
    with pytest.raises(ValueError):
        np.random.RandomState(0).randint(0, 0)                             # what the reference runs into
    with pytest.raises(ValueError):
        B.draw_window(np.random.RandomState(0), bg_hw, (20, 30))


def test_draw_histmatch_consumes_the_generator_as_the_reference_does():
    fired = unfired = swapped = 0
    for seed in range(400):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        d, want = B.draw_histmatch(a), R.histmatch_calls(b)
        assert _same_position(a, b)
        if want is None:
            unfired += 1
            assert d is None
        else:
            fired += 1
            swapped += want[1]
            assert (d.ratio, d.match_bg) == want and 0 <= d.ratio < 0.5
            assert d.table.dtype == np.float32 and list(d.table) == [np.float32(want[0]), np.float32(1. - want[0]), float(want[1]), 0.0]
    assert fired > 80 and unfired > 200
    assert sum(B.draw_histmatch(np.random.RandomState(s), 1.0).match_bg for s in range(400)) > 5       # the 5 % branch is reached
    assert B.draw_histmatch(np.random.RandomState(1), 0.0) is None


# ---- the taps ---------------------------------------------------------------------------------------------------------------------------------------
def test_taps_sum_to_256_with_a_positive_centre_for_all_twelve_pairs():
    assert len(R.PAIRS) == 12 and (B.BLUR_KERNEL_SIZES, B.BLUR_SIGMAS) == (R.KERNEL_SIZES, R.SIGMAS)
    for ks, sigma in R.PAIRS:
        q = B.gaussian_taps(ks, sigma)
        assert q.dtype == np.int32 and q.shape == (ks,) and int(q.sum()) == 256 and q.min() >= 0
        assert 20 <= q[ks // 2] <= 102 and np.array_equal(q, q[::-1])       # (15, 3.0): the centre, 32, ends one below its neighbours
        assert np.array_equal(q, R.taps(ks, sigma))
        off_centre = np.arange(ks) != ks // 2
        assert np.abs(q - 256 * R.float_taps(ks, sigma))[off_centre].max() <= 0.5      # rint; the centre takes what is left
    assert list(B.gaussian_taps(1, 2.0)) == [256]


@pytest.mark.parametrize('bad', [(4, 1.0), (27, 1.0), (0, 1.0), (-3, 1.0), (5, 0.0), (5, -1.0), (5, float('nan'))])
def test_gaussian_taps_rejections(bad):
    with pytest.raises(ValueError):
        B.gaussian_taps(*bad)


def test_gaussian_taps_wants_an_int():
    with pytest.raises(TypeError):
        B.gaussian_taps(5.0, 1.0)


# ---- the blur ---------------------------------------------------------------------------------------------------------------------------------------
def _scipy_blur(bg, k):
    from scipy import ndimage
    f = ndimage.correlate1d(bg.astype(np.float64), k, axis=1, mode='mirror')
    return ndimage.correlate1d(f, k, axis=0, mode='mirror')


@pytest.mark.parametrize('pair', R.PAIRS, ids=lambda p: 'ks%d_s%s' % p)
def test_integer_blur_stays_within_the_taps_quantisation_error_of_scipy(pair):
    """With E = sum k_i k_j v the fp64 result and S = sum q_i q_j v the integer sums, out = floor((S + 32768) / 65536) lies within 1/2 of
    S / 65536, and |S / 65536 - E| <= 255 sum_ij |q_i q_j / 65536 - k_i k_j|: the bound comes from the taps alone (an image of 0 and 255
    laid out by the signs of the differences reaches it), plus 1e-9 for scipy's own fp64 sums."""
    pytest.importorskip('scipy')
    ks, sigma = pair
    q, k = R.taps(ks, sigma), R.float_taps(ks, sigma)
    bound = 0.5 + 255 * np.abs(np.outer(q, q) / 65536 - np.outer(k, k)).sum() + 1e-9
    worst = 0.0
    for bg in (R.image(40, 45, 1, 'noise'), R.image(5, 7, 2, 'noise'), R.image(31, 29, 3, 'ramp'), np.full((9, 8, 3), 255, np.uint8)):
        worst = max(worst, np.abs(R.blur(bg, q).astype(np.float64) - _scipy_blur(bg, k)).max())
    print('ks %d sigma %s: observed %.4f, bound %.4f' % (ks, sigma, worst, bound))
    assert worst <= bound
    assert np.array_equal(R.blur(np.full((9, 8, 3), 255, np.uint8), q), np.full((9, 8, 3), 255, np.uint8))   # the taps sum to 256 exactly


def test_r101_is_np_pads_reflect_repeated():
    for n in (1, 2, 3, 5, 7):
        src = np.arange(10, 10 + n)
        for reach in (1, 2, 12):
            if n == 1:
                want = np.full(n + 2 * reach, 10)
            else:
                want = src
                left = reach
                while left > 0:                                             # np.pad reflects at most n - 1 at a time: repeat
                    step = min(left, len(want) - 1)
                    want = np.pad(want, step, mode='reflect')
                    left -= step
            assert np.array_equal(src[R.r101(np.arange(-reach, n + reach), n)], want), (n, reach)


def test_window_without_taps_is_the_slice_and_ks1_is_a_copy():
    bg = R.image(12, 13, 4)
    assert np.array_equal(R.window(bg, None, 2, 3, 5, 6), bg[3:8, 2:8])
    assert np.array_equal(R.blur(bg, np.array([256])), bg)


# ---- the curves -------------------------------------------------------------------------------------------------------------------------------------
def _literal_curve_result(s, t, ratio):
    m = R.match_unique(s.astype(np.float32), t.astype(np.float32)).astype(np.float32)
    return (m * ratio + s.astype(np.float32) * (1. - ratio)).astype(np.uint8)


@pytest.mark.parametrize('name', sorted(R.curve_cases()))
def test_bincount_table_equals_the_unique_interp_statement(name):
    s, t = R.curve_cases()[name]
    for ratio in (0.0, 0.25, 0.3141592653589793, 0.4999):
        lut = R.match_table(np.bincount(s, minlength=256), np.bincount(t, minlength=256), ratio)
        assert np.array_equal(lut[s], _literal_curve_result(s, t, ratio)), ratio
        absent = np.setdiff1d(np.arange(256), s)
        assert np.array_equal(lut[absent], absent)                          # bytes that do not occur: the identity


def test_bincount_table_on_random_cases_and_tiled_templates():
    """Also pins that np.interp of this NumPy is not fused: `interp_written_out` rounds the product and the sum separately."""
    rng = np.random.default_rng(8)
    inexact = 0
    for i in range(120):
        n, m = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        lo, hi = sorted(rng.integers(0, 257, 2))
        s = rng.integers(lo, max(hi, lo + 1), n).astype(np.uint8)
        t = rng.integers(0, 256, m).astype(np.uint8) if i % 3 else rng.choice(rng.integers(0, 256, 4), m).astype(np.uint8)
        ratio = float(rng.uniform(0, 0.5))
        lut = R.match_table(np.bincount(s, minlength=256), np.bincount(t, minlength=256), ratio)
        assert np.array_equal(lut[s], _literal_curve_result(s, t, ratio)), i
        tiled = np.tile(t, 3)                                               # the reference tiles the background over the T frames
        assert np.array_equal(R.match_table(np.bincount(s, minlength=256), np.bincount(tiled, minlength=256), ratio), lut), i
        m64 = R.match_unique(s.astype(np.float32), t.astype(np.float32))
        inexact += int((m64 != np.rint(m64)).any())
    assert inexact > 30                                                     # the interpolating branch was taken, not only exact hits


def test_histmatch_of_frames_equals_the_tables():
    fg, bg = R.clip(3, 9, 11, 1), R.image(9, 11, 2, 'band')
    for hist in ((0.3, False), (0.45, True), (0.0, False)):
        f2, b2 = R.histmatch_literal(fg, np.tile(bg, (3, 1, 1, 1)), *hist)
        l = R.luts(fg, bg, hist)
        assert np.array_equal(R.apply_luts(fg, l[0]), f2) and np.array_equal(R.apply_luts(np.tile(bg, (3, 1, 1, 1)), l[1]), b2)
        ident = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256))
        assert np.array_equal(l[0 if hist[1] else 1], ident)                # the side that is not matched
    assert np.array_equal(R.luts(fg, bg, None), np.broadcast_to(np.arange(256, dtype=np.uint8), (2, 3, 256)))


# ---- the composite ----------------------------------------------------------------------------------------------------------------------------------
def test_table_composite_equals_the_literal_expression_on_all_triples():
    v = np.arange(256, dtype=np.uint8)
    F, Bv = np.meshgrid(v, v, indexing='ij')
    wt = R.weights()
    assert wt.dtype == np.float64 and wt.shape == (256, 2)
    above = 0
    for al in range(256):
        A = np.full_like(F, al)
        assert np.array_equal(R.compose_literal(F[..., None], A, Bv[..., None]), R.compose_table(F[..., None], A, Bv[..., None], wt)), al
        a = A.astype(float) / 255.0
        s = F * a + Bv * (1 - a)
        above += int((s > 255).sum())
        assert s.max() <= 255.00000000000003
    assert above == 11                                                      # the clip acts


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_fixture():
    g = load_golden('background_pinned.npz')
    assert str(g['versions']).startswith('numpy ')
    assert sorted({k.split('.')[0] for k in g.files if '.' in k}) == sorted(G.CASES)
    fired = set()
    for name, case in G.CASES.items():
        got = G.run(case)
        for k, v in got.items():
            assert np.array_equal(g['%s.%s' % (name, k)], v) and g['%s.%s' % (name, k)].dtype == v.dtype, (name, k)
        fired.add((case[6] is not None, case[9] is not None))
    assert len(fired) == 4                                                  # every fired / unfired combination


# ---- records and the order of the errors ----------------------------------------------------------------------------------------------------------------
def test_draw_records():
    d = B.BackgroundDraws(B.gaussian_taps(5, 1.0), 3, 4, 10, 12)
    assert d.blurred and not d.on_device and d.win.dtype == np.int32 and d.win.shape == (B.WIN_TABLE,)
    assert not B.BackgroundDraws(None, 0, 0, 1, 1).blurred
    for bad in (dict(taps=[100, 100, 100]), dict(taps=[128, 128]), dict(taps=[-1, 258, -1]), dict(taps=np.ones(27, np.int32)), dict(x=-1), dict(h=0)):
        kw = dict(taps=None, x=0, y=0, h=4, w=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            B.BackgroundDraws(**kw)
    with pytest.raises(TypeError):
        B.BackgroundDraws(None, 0.5, 0, 4, 4)
    with pytest.raises(ValueError):
        B.HistDraws(1.5)
    h = B.HistDraws(0.25, True)
    assert list(h.table) == [0.25, 0.75, 1.0, 0.0] and not h.on_device
    assert (B.MAX_KSIZE, B.WIN_TABLE, B.TILE_ROWS, B.TILE_COLS) == (25, 32, 16, 64)


def test_argument_errors_come_before_the_no_gpu_error():
    fg, a, bg = np.zeros((2, 8, 9, 3), np.uint8), np.zeros((2, 8, 9), np.uint8), np.zeros((20, 21, 3), np.uint8)
    d, h = B.BackgroundDraws(B.gaussian_taps(5, 1.0), 3, 4, 8, 9), B.HistDraws(0.25)
    with pytest.raises(TypeError):
        B.blur_crop(bg.astype(np.float32), d)
    with pytest.raises(TypeError):
        B.blur_crop(bg, B.gaussian_taps(5, 1.0))                            # taps are not a BackgroundDraws
    with pytest.raises(ValueError):
        B.blur_crop(bg[..., :2], d)
    with pytest.raises(ValueError):
        B.blur_crop(bg[None], d)
    with pytest.raises(ValueError):
        B.blur_crop(bg, B.BackgroundDraws(None, 13, 4, 8, 9))               # x + w > bw
    with pytest.raises(ValueError):
        B.blur_crop(bg, B.BackgroundDraws(None, 3, 13, 8, 9))               # y + h > bh
    with pytest.raises(ValueError):
        B.blur_crop(bg, B.BackgroundDraws(None, 0, 0, 8, 9, win=np.zeros(5, np.int32)))
    with pytest.raises(TypeError):
        B.histograms(fg.astype(np.int32))
    with pytest.raises(ValueError):
        B.histograms(a)
    with pytest.raises(ValueError):
        B.histograms(torch.empty((2 ** 16, 2 ** 15, 1, 3), dtype=torch.uint8, device='meta'))      # 2^31 pixels
    with pytest.raises(TypeError):
        B.match_luts(fg, bg, (0.3, False))
    with pytest.raises(TypeError):
        B.match_luts(fg.astype(np.float32), bg, h)
    with pytest.raises(TypeError):
        B.compose(fg, a.astype(np.float32), bg[:8, :9])
    with pytest.raises(ValueError):
        B.compose(fg, a[..., :8], bg[:8, :9])
    with pytest.raises(ValueError):
        B.compose(fg, a, bg)                                                # a background of another size
    with pytest.raises(ValueError):
        B.compose(fg, a, bg[:8, :9], luts=np.zeros((3, 256), np.uint8))
    with pytest.raises(TypeError):
        B.compose(fg, a, bg[:8, :9], luts=np.zeros((2, 3, 256), np.int32))
    with pytest.raises(ValueError):
        B.random_background(fg, a, bg, B.BackgroundDraws(None, 0, 0, 8, 10), None)                 # the window is not the frames' size
    with pytest.raises(ValueError):
        B.random_background(fg, a[:1], bg, d, h)
    with pytest.raises(TypeError):
        B.random_background(fg, a, bg, d, 0.3)
    with pytest.raises(TypeError):
        B.random_background(fg, a, bg.astype(np.int16), d, h)
    if not torch.cuda.is_available():                                      # well-formed calls: the package's own error, never torch's
        for call in (lambda: B.blur_crop(bg, d), lambda: B.histograms(fg), lambda: B.match_luts(fg, bg, h), lambda: B.match_luts(fg, bg, None),
                     lambda: B.compose(fg, a, bg[:8, :9]), lambda: B.random_background(fg, a, bg, d, h), lambda: d.to(), lambda: h.to()):
            with pytest.raises(hip.MaggieHipError):
                call()


def test_constants_are_the_librarys():
    lib = hip.lib()
    for name in ('mg_bg_blur_crop', 'mg_bg_hist', 'mg_bg_match_lut', 'mg_bg_compose'):
        assert getattr(lib, name) is not None
    v = [hip.c_int() for _ in range(5)]
    assert lib.mg_bg_limits(*[hip.ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [B.MAX_KSIZE, B.WIN_TABLE, B.TILE_ROWS, B.TILE_COLS, B.MAX_SIDE]
    assert lib.mg_bg_limits(*[None] * 5) == -2
