"""Host side of the device RandomAffine (maggie_amd.utils.affine): the fixture against the restatement, `affine.draw` against hand-replayed
RandomState calls, the fixed-point tables (half-to-even ties, negative coordinates), the argument errors. No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import affine_restatement as A                                        # noqa: E402
import geometry_restatement as R                                      # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.hip import MaggieHipError                             # noqa: E402
from maggie_amd.utils import affine, crop                             # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

CASES = list(A.GOLDEN)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
INTERPS = ((affine.LINEAR, A.INTER_LINEAR), (affine.NEAREST, A.INTER_NEAREST))
MATRICES = {
    'identity': [[1, 0, 0], [0, 1, 0]],
    'half_pixel': [[1, 0, 0.5], [0, 1, -0.5]],
    'rot90': [[0, -1, 20], [1, 0, 3]],
    'zoom2': [[2, 0, -7.25], [0, 2, 3.5]],
    'singular': [[1, 2, 3], [2, 4, 5]],
    'far_outside': [[1, 0, 1e7], [0, 1, -1e12]],
}


def _tables(matrix, H, W, flag):
    return np.concatenate(A.tables(np.asarray(matrix, np.float64), H, W, flag))


@pytest.mark.parametrize('name', CASES)
def test_fixture_equals_the_restatement(name):
    d = load_golden('affine_pinned.npz')
    assert os.path.getsize(os.path.join(GOLDEN_DIR, 'affine_pinned.npz')) <= os.path.getsize(os.path.join(GOLDEN_DIR, 'geometry_pinned.npz'))
    c = A.GOLDEN[name]
    r, rs = A.golden_run(name)
    assert sorted(k for k in d.files if k.startswith(name + '.')) == sorted(
        name + '.' + k for k in ('frames', 'alphas', 'info', 'intensity', 'minmax', 'state') + (('matrix',) if r['fired'] else ()))
    assert np.array_equal(R.unpack_rows(d[name + '.frames']), r['frames_u8']) and np.array_equal(R.unpack_rows(d[name + '.alphas']), r['alphas'])
    assert d[name + '.info'].tolist() == [int(r['fired']), -1 if r['form'] is None else r['form'], c['T'], c['n']]
    assert d[name + '.intensity'].tolist() == [r['intensity']] and np.array_equal(d[name + '.minmax'], A.minmax(r['frames_u8']))
    assert np.array_equal(d[name + '.state'], A.state_digest(rs))
    if r['fired']:
        assert d[name + '.matrix'].dtype == np.float64 and np.array_equal(d[name + '.matrix'], r['matrix'])
        # the table-level operators give the same arrays as the code path
        frames, alphas, _ = A.golden_inputs(name)
        lin, near = A.tables(r['matrix'], c['h'], c['w'], A.INTER_LINEAR), A.tables(r['matrix'], c['h'], c['w'], A.INTER_NEAREST)
        assert np.array_equal(np.stack([A.warp_linear(f, lin) for f in frames]), r['frames_u8'])
        assert np.array_equal(np.stack([A.warp_nearest(a, near) for a in alphas]), r['alphas'])
        assert np.array_equal(A.channel_shift(r['frames_u8'], r['intensity']), r['frames']) and r['frames'].dtype == np.float64
    else:
        frames, alphas, _ = A.golden_inputs(name)
        assert np.array_equal(r['frames_u8'], frames) and np.array_equal(r['alphas'], alphas)


@pytest.mark.parametrize('name', CASES)
def test_draw_against_hand_replayed_generator_calls(name):
    """The calls the reference makes, written out by hand from transforms.py:932 and utils.py:142-212 with the loaders' parameters."""
    d = load_golden('affine_pinned.npz')
    c = A.GOLDEN[name]
    fired, form = d[name + '.info'].tolist()[:2]
    hand = np.random.RandomState(c['rs_seed'])
    skip_draw = hand.rand()
    assert (skip_draw > c['p']) == (not fired)
    if fired:
        theta = np.pi / 180 * hand.uniform(-10, 10)
        shear = np.pi / 180 * hand.uniform(-5, 5)
        zx = hand.uniform(.95, 1.05)
        zy = hand.uniform(.95, 1.05)
        which = hand.random()
        assert (which < 0.5) == (form == 0)
        rot = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
        sh = np.array([[1, -np.sin(shear), 0], [0, np.cos(shear), 0], [0, 0, 1]]) if which < 0.5 else \
            np.array([[np.cos(shear), 0, 0], [np.sin(shear), 1, 0], [0, 0, 1]])
        m = np.dot(np.dot(rot, sh), np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]]))
        o_x, o_y = float(c['h']) / 2 + 0.5, float(c['w']) / 2 + 0.5           # h as x, w as y
        m = np.dot(np.dot(np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]]), m), np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]]))
        cvM = np.array([[m[1, 1], m[1, 0], m[1, 2]], [m[0, 1], m[0, 0], m[0, 2]]])
        intensity = hand.uniform(-0.03 * 255., 0.03 * 255.)
    rs = np.random.RandomState(c['rs_seed'])
    draws = affine.draw(rs, c['h'], c['w'], c['p'])
    assert np.array_equal(A.state_digest(rs), A.state_digest(hand)) and np.array_equal(A.state_digest(rs), d[name + '.state'])
    assert draws.fired == bool(fired) and (draws.H, draws.W) == (c['h'], c['w']) and not draws.on_device
    if not fired:
        assert draws.matrix is None and draws.linear is None and draws.nearest is None and draws.shift is None and draws.intensity == 0.0
        return
    assert draws.form == form and draws.intensity == intensity == d[name + '.intensity'][0] and draws.shift.tolist() == [intensity]
    assert draws.matrix.dtype == np.float64 and np.array_equal(draws.matrix, cvM) and np.array_equal(draws.matrix, d[name + '.matrix'])
    for interp, flag in INTERPS:
        t = draws.linear if interp == affine.LINEAR else draws.nearest
        assert t.dtype == np.int32 and np.array_equal(t, _tables(cvM, c['h'], c['w'], flag))
        assert all(np.array_equal(a, b) for a, b in zip(draws.tables_of(interp), A.tables(cvM, c['h'], c['w'], flag)))
    assert draws.staged_ok


def test_draw_without_shear_or_rotation_and_the_identity():
    """shear == 0 draws no shear form; rt, sh, zm = 1 and cs off draw nothing but the skip draw, and the identity has no matrix."""
    rs, hand = np.random.RandomState(5), np.random.RandomState(5)
    d = affine.draw(rs, 24, 40, p=1.0, sh=0)
    hand.rand()
    theta = np.pi / 180 * hand.uniform(-10, 10)
    zx, zy = hand.uniform(.95, 1.05), hand.uniform(.95, 1.05)
    intensity = hand.uniform(-0.03 * 255., 0.03 * 255.)
    assert np.array_equal(A.state_digest(rs), A.state_digest(hand)) and d.form is None and d.intensity == intensity
    fired, cvM, i2, form = A.draws(np.random.RandomState(5), 24, 40, 1.0, sh=0)
    assert fired and form is None and i2 == intensity and np.array_equal(d.matrix, cvM)
    rot = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
    m = A.offset_center(np.dot(rot, np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])), 24, 40)
    assert np.array_equal(d.matrix, np.array([[m[1, 1], m[1, 0], m[1, 2]], [m[0, 1], m[0, 0], m[0, 2]]]))
    rs, hand = np.random.RandomState(6), np.random.RandomState(6)
    d = affine.draw(rs, 24, 40, p=1.0, rt=0, sh=0, zm=(1, 1), cs=0)
    hand.rand()
    assert np.array_equal(A.state_digest(rs), A.state_digest(hand)) and d.fired and d.matrix is None and d.intensity == 0.0
    for interp, flag in INTERPS:                                             # no matrix: the identity's tables
        assert np.array_equal(d.linear if interp == affine.LINEAR else d.nearest, _tables(MATRICES['identity'], 24, 40, flag))


@pytest.mark.parametrize('name', list(MATRICES))
@pytest.mark.parametrize('H,W', [(1, 1), (33, 65), (40, 24)])
def test_tables_equal_the_restatement(name, H, W):
    d = affine.from_matrix(MATRICES[name], H, W, intensity=-2.5)
    assert d.fired and d.intensity == -2.5 and d.shift.dtype == np.float64
    for interp, flag in INTERPS:
        t = d.linear if interp == affine.LINEAR else d.nearest
        assert t.dtype == np.int32 and t.shape == (2 * (H + W),) and np.array_equal(t, _tables(MATRICES[name], H, W, flag))
        assert np.abs(t.astype(np.int64)).max() <= affine.LIMIT + 512
    assert np.array_equal(affine.invert(MATRICES[name]), A.invert(MATRICES[name]))
    if name == 'singular':
        assert np.array_equal(affine.invert(MATRICES[name])[[0, 1, 3, 4]], np.zeros(4))      # D == 0: the zero map, not an error
    assert d.staged_ok == (affine.box_bytes(d.linear, H, W) <= affine.BOX_BYTES)


def test_cv_round_ties_go_to_even():
    """The inverse of diag(1 / (1 + 1/2048)) has M0 = 1 + 1/2048 exactly: adelta[x] = x * 1024 + x / 2 ties at every odd x."""
    m0 = 1 + 1 / 2048
    matrix = [[1 / m0, 0, 0], [0, 1, 0]]
    assert affine.invert(matrix)[0] == m0
    adelta = affine.from_matrix(matrix, 4, 64).tables_of(affine.LINEAR)[0].astype(np.int64)
    x = np.arange(64)
    half = x // 2 + ((x % 2 == 1) & ((x // 2) % 2 == 1))                      # x / 2 rounded half to even
    assert np.array_equal(adelta, x * 1024 + half) and (adelta[1], adelta[3], adelta[5], adelta[7]) == (1024, 3074, 5122, 7172)
    assert np.array_equal(affine.cv_round([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]), [0, 2, 2, 0, -2, -2])
    assert np.array_equal(affine.cv_round([1e300, -1e300]), [affine.LIMIT - 1, -affine.LIMIT])


def test_negative_coordinates_floor():
    """A shift by -0.25 pixel: source x = -0.25 for the first column. Nearest: (-256 + 512) >> 10 = 0. A shift by +0.75 reads x = -0.75:
    (-768 + 512) >> 10 = -1, outside (an `int()` truncation would give 0). Linear at -0.75: sx = -1, fx = 8: a quarter of the first pixel."""
    src = np.full((3, 5), 200, np.uint8)
    near = A.warpAffine(src, np.array([[1, 0, 0.75], [0, 1, 0]]), (5, 3), flags=A.INTER_NEAREST)
    assert near[:, 0].tolist() == [0, 0, 0] and near[:, 1].tolist() == [200, 200, 200]
    assert A.warpAffine(src, np.array([[1, 0, 0.25], [0, 1, 0]]), (5, 3), flags=A.INTER_NEAREST)[:, 0].tolist() == [200, 200, 200]
    lin = A.warpAffine(src, np.array([[1, 0, 0.75], [0, 1, 0]]), (5, 3), flags=A.INTER_LINEAR)
    assert lin[:, 0].tolist() == [50, 50, 50] and lin[:, 1].tolist() == [200, 200, 200]
    t = affine.from_matrix([[1, 0, 0.75], [0, 1, 0]], 3, 5)
    adelta, _, X0, _ = t.tables_of(affine.NEAREST)
    assert (int(X0[0]) + int(adelta[0])) >> 10 == -1 and int(X0[0]) == -768 + 512
    adelta, _, X0, _ = t.tables_of(affine.LINEAR)
    X = (int(X0[0]) + int(adelta[0])) >> 5
    assert (X >> 5, X & 31) == (-1, 8)


def test_restated_warp_on_simple_matrices():
    src = np.random.default_rng(0).integers(1, 256, (7, 9, 3), dtype=np.uint8)
    assert np.array_equal(A.warpAffine(src, np.array(MATRICES['identity'], np.float64), (9, 7)), src)
    for dx, dy in ((2, 0), (-2, 0), (0, 3), (0, -3)):
        for flag in (A.INTER_LINEAR, A.INTER_NEAREST):
            out = A.warpAffine(src, np.array([[1, 0, dx], [0, 1, dy]], np.float64), (9, 7), flags=flag)
            want = np.zeros_like(src)
            want[max(dy, 0):7 + min(dy, 0), max(dx, 0):9 + min(dx, 0)] = src[max(-dy, 0):7 + min(-dy, 0), max(-dx, 0):9 + min(-dx, 0)]
            assert np.array_equal(out, want), (dx, dy, flag)
    s = src[:, :, 0].astype(np.int64)
    half = A.warpAffine(src[:, :, 0], np.array([[1, 0, 0.5], [0, 1, 0]]), (9, 7)).astype(np.int64)
    assert np.array_equal(half[:, 1:], (s[:, :-1] + s[:, 1:] + 1) >> 1) and np.array_equal(half[:, 0], (s[:, 0] + 1) >> 1)


def test_argument_errors_raise_before_the_device():
    rs = np.random.RandomState(0)
    f = np.zeros((1, 32, 48, 3), np.uint8)
    a = np.zeros((2, 32, 48), np.uint8)
    with pytest.raises(TypeError):
        affine.draw(rs, 32.0, 48)
    with pytest.raises(ValueError):
        affine.draw(rs, 0, 48)
    with pytest.raises(ValueError):
        affine.draw(rs, 32, affine.MAX_SIDE + 1)
    assert np.array_equal(A.state_digest(rs), A.state_digest(np.random.RandomState(0)))          # nothing was drawn
    with pytest.raises(ValueError):
        affine.from_matrix(np.zeros((3, 3)), 32, 48)
    with pytest.raises(ValueError):
        affine.from_matrix([[1, 0, np.nan], [0, 1, 0]], 32, 48)
    fired, unfired = affine.from_matrix(MATRICES['half_pixel'], 32, 48), affine.draw(np.random.RandomState(5), 32, 48, p=0.0)
    assert fired.fired and not unfired.fired
    with pytest.raises(TypeError):
        affine.apply(f, a, (0, 0))
    with pytest.raises(ValueError, match='did not fire'):
        affine.apply(f, a, unfired)
    with pytest.raises(TypeError):
        affine.warp(f.astype(np.int32), a, fired)
    with pytest.raises(ValueError):
        affine.warp(np.zeros((1, 32, 48, 4), np.uint8), a, fired)
    with pytest.raises(ValueError):
        affine.warp(np.zeros((1, 32, 40, 3), np.uint8), a, fired)                                # not the size the draws were made for
    with pytest.raises(ValueError):
        affine.warp(f, np.zeros((2, 32, 40), np.uint8), fired)
    with pytest.raises(ValueError):
        affine.warp(f, a, fired, regime='lds')
    big = affine.from_matrix(MATRICES['rot90'], 600, 600)                                        # a quarter turn: a 64-column tile reads 64 rows of 32 columns
    wide = affine.from_matrix([[0.1, 0, 0], [0, 0.1, 0]], 600, 600)
    assert not wide.staged_ok and affine._regime(wide, None) == affine.DIRECT
    with pytest.raises(ValueError, match='staged'):
        affine.warp(np.zeros((1, 600, 600, 3), np.uint8), None, wide, regime='staged')
    assert big.staged_ok and affine._regime(big, None, 1) == affine.DIRECT and affine._regime(big, None, affine.STAGED_MIN_FRAMES) == affine.STAGED
    assert affine._regime(big, 'staged', 1) == affine.STAGED and affine._regime(big, 'direct', 8) == affine.DIRECT
    crop_draws = crop.draw(np.random.RandomState(1), 32, 48, (32, 48), 0.0, 0.5, lambda: (0, 48, -1, 32, -1), lambda w: None)
    with pytest.raises(TypeError):
        DevicePreprocessor().train_item_affine(f, a, a, crop_draws, (1, 2))


def test_no_gpu_raises_maggie_hip_error():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    f = np.zeros((1, 32, 48, 3), np.uint8)
    a = np.zeros((2, 32, 48), np.uint8)
    draws = affine.from_matrix(MATRICES['half_pixel'], 32, 48, 1.5)
    with pytest.raises(MaggieHipError):
        affine.warp(f, a, draws)
    with pytest.raises(MaggieHipError):
        affine.apply(f, a, draws)
    with pytest.raises(MaggieHipError):
        affine.shift_normalize(f, np.zeros((1, 2), np.int32), 1.5)
    with pytest.raises(MaggieHipError):
        draws.to()


def test_c_entries_reject_bad_arguments_before_any_launch():
    from maggie_amd import hip
    I, L = ctypes.c_int, ctypes.c_long
    lib = hip.lib()
    for fn in (lib.mg_affine_warp_planes, lib.mg_affine_warp_frames, lib.mg_affine_shift_normalize, lib.mg_affine_limits):
        fn.restype = ctypes.c_int
    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    fake, other = ctypes.c_void_p(16), ctypes.c_void_p(4096)                  # non-null pointers: never read, the checks come first

    def planes(n=1, H=4, W=4, src=None, dst=None, tab=None):
        return lib.mg_affine_warp_planes(src, dst, tab, L(n), I(H), I(W), None)

    def frames(n=1, H=4, W=4, regime=0, src=None, dst=None, tab=None, mm=None):
        return lib.mg_affine_warp_frames(src, dst, tab, mm, L(n), I(H), I(W), I(regime), None)

    def shift(n=1, H=4, W=4, mean=three, src=None, dst=None, mm=None, inten=None):
        return lib.mg_affine_shift_normalize(src, dst, mm, inten, L(n), I(H), I(W), mean, mean, None)
    assert planes() == frames() == shift() == -2                             # null pointers
    assert planes(n=0) == frames(n=0) == shift(n=0) == 0
    for bad in (dict(n=-1), dict(H=0), dict(W=-1), dict(H=affine.MAX_SIDE + 1), dict(W=affine.MAX_SIDE + 1)):
        assert planes(src=fake, dst=other, tab=fake, **bad) == -2, bad
        assert frames(src=fake, dst=other, tab=fake, mm=fake, **bad) == -2, bad
        assert shift(src=fake, dst=other, mm=fake, inten=fake, **bad) == -2, bad
    assert frames(src=fake, dst=other, tab=fake, mm=fake, regime=2) == -2 and frames(src=fake, dst=other, tab=fake, mm=fake, regime=-1) == -2
    assert planes(src=fake, dst=fake, tab=fake) == -2 and frames(src=fake, dst=fake, tab=fake, mm=fake) == -2       # in place
    assert planes(src=fake, dst=other) == -2 and frames(src=fake, dst=other, tab=fake) == -2
    assert shift(src=fake, dst=other, mm=fake, inten=fake, mean=None) == -2 and shift(src=fake, dst=other, mm=fake) == -2


def test_python_constants_match_the_library():
    from maggie_amd import hip
    a, b, c, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert hip.lib().mg_affine_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
    assert (a.value, b.value, c.value, d.value) == (affine.TILE_ROWS, affine.TILE_COLS, affine.BOX_BYTES, affine.MAX_SIDE)
    assert hip.lib().mg_affine_limits(None, None, None, None) == -2
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, 'include', 'maggie_hip.h')).read()
    assert '#define MG_AFFINE_STAGED %d\n' % affine.STAGED in header and '#define MG_AFFINE_DIRECT %d\n' % affine.DIRECT in header
    assert (affine.LIMIT, affine.AB_BITS) == (A.LIMIT, A.AB_BITS)


def test_reference_extremes_fit_the_staged_box_at_512():
    """+-10 degrees with +-5 degrees of either shear form at the zoom extremes on 512 x 512: every tile's box fits the LDS budget."""
    worst = 0
    for theta in (-10, 10):
        for shear in (-5, 5):
            for form in (0, 1):
                for zx, zy in ((0.95, 0.95), (1.05, 1.05), (0.95, 1.05)):
                    t, s = np.pi / 180 * theta, np.pi / 180 * shear
                    rot = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
                    sh = np.array([[1, -np.sin(s), 0], [0, np.cos(s), 0], [0, 0, 1]]) if form == 0 else \
                        np.array([[np.cos(s), 0, 0], [np.sin(s), 1, 0], [0, 0, 1]])
                    m = A.offset_center(np.dot(np.dot(rot, sh), np.diag([zx, zy, 1.0])), 512, 512)
                    cvM = np.array([[m[1, 1], m[1, 0], m[1, 2]], [m[0, 1], m[0, 0], m[0, 2]]])
                    d = affine.from_matrix(cvM, 512, 512)
                    assert d.staged_ok
                    worst = max(worst, affine.box_bytes(d.linear, 512, 512))
    assert 0 < worst <= affine.BOX_BYTES


def test_signatures():
    """train_item keeps the signature the crop suite pins; the affine wiring is a method of its own."""
    assert str(inspect.signature(DevicePreprocessor.train_item)) == \
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, slot_ids=None, *, transition=None, mask_draws=None, lut=None)'
    assert str(inspect.signature(DevicePreprocessor.train_item_affine)) == \
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, affine_draws, slot_ids=None, *, transition=None, mask_draws=None, lut=None, ' \
        'warp_masks=False)'
    assert str(inspect.signature(affine.draw)) == '(random, H, W, p=0.1, rt=10, sh=5, zm=(0.95, 1.05), cs=7.6499999999999995)'
