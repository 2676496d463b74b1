"""The host side of the device MotionBlur (maggie_amd.utils.motion) and the restatement the device is compared with
(tests/motion_restatement.py): the restatement against scipy's fp64 correlation on every case tests/test_gpu_motion.py runs and against the
fixture scipy wrote, `taps_of` and its rejections, the draws of `draw` against the reference's flow, `line_kernel`, the signatures of the
training item, and the order of the errors. No GPU is needed."""
import inspect
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import motion_restatement as M                                        # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import motion, photometric                      # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_motion_golden as G                                        # noqa: E402


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', M.SHAPES, ids=lambda s: '%dx%d' % s)
def test_restatement_equals_scipy_on_every_device_case(shape):
    pytest.importorskip('scipy')
    h, w = shape
    frames, planes = M.case_frames(h, w), M.case_planes(h, w)
    ties = 0
    for name, K in M.KERNELS.items():
        offs = M.offsets(K)
        assert np.array_equal(M.blur_frames(frames, offs), np.stack([G.scipy_blur(f, K) for f in frames])), name
        assert np.array_equal(M.blur_planes(planes, offs), np.moveaxis(G.scipy_blur(np.moveaxis(planes, 0, -1), K), -1, 0)), name
        if len(offs) % 2 == 0:
            ties += int((2 * (M.sums_plane(planes[0], offs) % len(offs)) == len(offs)).sum())
    assert ties > 0 or h * w < 16                                          # random inputs with an even n do reach exact ties


def test_r101_is_scipys_mirror_below_the_reach():
    pytest.importorskip('scipy')
    from scipy import ndimage
    for length in (1, 2, 3, 5):
        src = np.arange(10, 10 + length, dtype=np.float64)
        for d in range(-24, 25):
            K = np.zeros(49)
            K[24 + d] = 1
            got = ndimage.correlate1d(src, K, mode='mirror')
            assert [src[M.r101(i + d, length)] for i in range(length)] == list(got), (length, d)


def test_rhe_rounds_exact_ties_to_even_and_equals_rint():
    for n in range(1, 50):
        S = np.arange(0, 255 * n + 1)
        assert np.array_equal(M.rhe(S, n), np.rint(S / n).astype(np.int64)), n
    assert list(M.rhe(np.array([1, 3, 5, 7]), 2)) == [0, 2, 2, 4]


def test_restatement_equals_the_fixture():
    g = load_golden('motion_pinned.npz')
    assert str(g['versions']).startswith('scipy ')
    assert sorted(k[:-6] for k in g.files if k.endswith('.input')) == sorted(G.CASES)
    for name, (h, w, kname, kind, seed) in G.CASES.items():
        x, K = g[name + '.input'], g[name + '.kernel']
        assert np.array_equal(x, M.inputs(h, w, kind, seed, 3)) and np.array_equal(K, M.KERNELS[kname])
        assert list(g[name + '.info']) == [h, w, K.shape[0], int(K.sum())]
        assert np.array_equal(M.blur_frames(x, M.offsets(K)), g[name + '.output']), name


# ---- taps_of ---------------------------------------------------------------------------------------------------------------------------------------
def test_taps_of_uint8_and_float_kernels():
    for name, K in M.KERNELS.items():
        offs = M.offsets(K)
        for kernel in (K, K.astype(np.float32) / K.sum(), K.astype(np.float64) / K.sum(), K.astype(bool)):
            t = motion.taps_of(kernel)
            assert t.dtype == np.int32 and t.shape == (motion.TABLE,) and (t[0], t[1]) == (len(offs), K.shape[0]), name
            assert [tuple(p) for p in t[2:2 + 2 * len(offs)].reshape(-1, 2)] == offs and not t[2 + 2 * len(offs):].any(), name
            assert M.clamped_offsets(t) == offs
    assert motion.TABLE == 2 + 2 * 49 and (motion.MAX_KSIZE, motion.MAX_TAPS) == (49, 49)
    assert (motion.RAW, motion.NORM) == (photometric.RAW, photometric.NORM)
    assert (motion.TILE_ROWS, motion.TILE_COLS) == (M.TILE_ROWS, M.TILE_COLS)


def test_constants_are_the_librarys():
    lib = hip.lib()
    v = [hip.c_int() for _ in range(6)]
    assert lib.mg_motion_limits(*[hip.ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [motion.MAX_KSIZE, motion.MAX_TAPS, motion.TILE_ROWS, motion.TILE_COLS, motion.TABLE, motion.MAX_SIDE]
    assert lib.mg_motion_limits(*[None] * 6) == -2


@pytest.mark.parametrize('kernel', [
    np.ones((4, 4), np.uint8),                                             # even side
    np.eye(51, dtype=np.uint8),                                            # side 51
    np.eye(1, dtype=np.uint8),                                             # side 1
    np.array([[0, 0, 0], [0.5, 0.25, 0.25], [0, 0, 0]]),                   # unequal weights
    np.zeros((5, 5), np.uint8),                                            # empty
    np.ones((9, 9), np.uint8),                                             # 81 taps
    np.ones((3, 5), np.uint8),                                             # not square
    np.ones((3, 3, 3), np.uint8),                                          # not 2-D
    -np.eye(3),                                                            # negative weights
], ids=['even', 'side51', 'side1', 'unequal', 'empty', 'too_many', 'not_square', 'not_2d', 'negative'])
def test_taps_of_rejections(kernel):
    with pytest.raises(ValueError):
        motion.taps_of(kernel)
    with pytest.raises(ValueError):
        motion.MotionDraws(kernel)


def test_motion_draws_records():
    assert not motion.MotionDraws().fired and motion.MotionDraws().on_device
    d = motion.MotionDraws(M.KERNELS['k11'])
    assert d.fired and not d.on_device and np.array_equal(d.taps, motion.taps_of(M.KERNELS['k11']))
    assert np.array_equal(motion.MotionDraws(taps=d.taps).taps, d.taps)
    bad = d.taps.copy()
    bad[0] = 60
    for table in (bad, d.taps[:-1], d.taps.astype(np.int64), torch.zeros(motion.TABLE, dtype=torch.int64), torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            motion.MotionDraws(taps=table)
    outside = d.taps.copy()
    outside[2] = 6                                                         # beyond an 11 x 11 kernel
    with pytest.raises(ValueError):
        motion.MotionDraws(taps=outside)
    with pytest.raises(ValueError):
        motion.MotionDraws(M.KERNELS['k11'], d.taps)


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------------------
def test_draw_consumes_the_generator_as_the_reference_does():
    fired = skipped = passed_p = 0
    for seed in range(200):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        calls, stub_calls = [], []

        def kernel_fn():
            calls.append(1)
            return M.KERNELS['k13']
        d = motion.draw(a, kernel_fn=kernel_fn) if seed % 2 else motion.draw(a, 0.3, kernel_fn)
        M.reference_call(b, 0.3, lambda: stub_calls.append(1))
        assert len(calls) == len(stub_calls) == int(d.fired) <= 1
        assert all(np.array_equal(u, v) for u, v in zip(a.get_state()[1:], b.get_state()[1:]))      # the same position in the stream
        # 1 value when rand() > p, else 4: the position equals that of a generator that drew exactly that many doubles
        c = np.random.RandomState(seed)
        first = c.rand()
        for _ in range(0 if first > 0.3 else 3):
            c.uniform(0, 1)
        assert a.get_state()[2] == c.get_state()[2] and np.array_equal(a.get_state()[1], c.get_state()[1])
        fired += d.fired
        skipped += first > 0.3
        passed_p += (first <= 0.3) and not d.fired
        if d.fired:
            assert np.array_equal(d.taps, motion.taps_of(M.KERNELS['k13']))
    assert fired > 20 and skipped > 100 and passed_p > 0                   # every path of the flow was taken
    # p = 1 with a generator whose firing draw passes: the kernel is needed
    with pytest.raises(ValueError):
        for seed in range(50):
            motion.draw(np.random.RandomState(seed), 1.0)


def test_line_kernel_properties():
    rng = random.Random(5)
    for _ in range(300):
        ksize = rng.choice(range(3, 50, 2))
        p0, p1 = (rng.randrange(ksize), rng.randrange(ksize)), (rng.randrange(ksize), rng.randrange(ksize))
        K = motion.line_kernel(ksize, p0, p1)
        assert K.dtype == np.uint8 and K.shape == (ksize, ksize) and set(np.unique(K)) <= {0, 1}
        assert K[p0[1], p0[0]] == 1 and K[p1[1], p1[0]] == 1               # points are (x, y), as cv2.line takes them
        assert int(K.sum()) == max(abs(p1[0] - p0[0]), abs(p1[1] - p0[1])) + 1
        ys, xs = np.nonzero(K)
        order = np.lexsort((ys, xs)) if abs(p1[0] - p0[0]) >= abs(p1[1] - p0[1]) else np.lexsort((xs, ys))
        ys, xs = ys[order], xs[order]                                       # along the longer axis: every step moves at most one pixel each way
        assert (np.abs(np.diff(ys)) <= 1).all() and (np.abs(np.diff(xs)) <= 1).all()
        assert motion.taps_of(K)[0] == K.sum()
    for bad in ((4, (0, 0), (1, 1)), (51, (0, 0), (1, 1)), (5, (0, 0), (5, 1)), (5, (-1, 0), (1, 1))):
        with pytest.raises(ValueError):
            motion.line_kernel(*bad)


def test_draw_kernel_follows_the_published_draw():
    sizes = set()
    for seed in range(300):
        a, b = random.Random(seed), random.Random(seed)
        K = motion.draw_kernel(a)
        ksize = b.choice(list(range(3, 50, 2)))
        xs, xe = b.randint(0, ksize - 1), b.randint(0, ksize - 1)
        ys, ye = b.sample(range(ksize), 2) if xs == xe else (b.randint(0, ksize - 1), b.randint(0, ksize - 1))
        assert a.getstate() == b.getstate()
        assert np.array_equal(K, motion.line_kernel(ksize, (xs, ys), (xe, ye))) and K.sum() >= 1
        sizes.add(ksize)
        motion.MotionDraws(K)
    assert min(sizes) == 3 and max(sizes) == 49 and all(s % 2 for s in sizes)
    assert motion.draw_kernel(random.Random(1), (5, 5)).shape == (5, 5)


# ---- the training item's signatures ------------------------------------------------------------------------------------------------------------------
def test_the_new_signature_and_the_three_old_ones():
    sig = lambda f: str(inspect.signature(f))                              # noqa: E731
    assert sig(DevicePreprocessor.train_item_motion) == (
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, motion, photo=None, affine_draws=None, slot_ids=None, *, transition=None, '
        'mask_draws=None, lut=None, warp_masks=False)')
    assert sig(DevicePreprocessor.train_item) == (
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, slot_ids=None, *, transition=None, mask_draws=None, lut=None)')
    assert sig(DevicePreprocessor.train_item_affine) == (
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, affine_draws, slot_ids=None, *, transition=None, mask_draws=None, lut=None, '
        'warp_masks=False)')
    assert sig(DevicePreprocessor.train_item_photo) == (
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, photo, affine_draws=None, slot_ids=None, *, transition=None, mask_draws=None, '
        'lut=None, warp_masks=False)')
    assert sig(motion.apply) == ("(frames_u8, alphas_u8, draws, *, normalize=False, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), "
                                 "device=None)")


# ---- the order of the errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_no_gpu_error():
    d = motion.MotionDraws(M.KERNELS['k3_n2'])
    f, a = np.zeros((2, 8, 9, 3), np.uint8), np.zeros((2, 8, 9), np.uint8)
    with pytest.raises(TypeError):
        motion.apply(f.astype(np.float32), a, d)
    with pytest.raises(TypeError):
        motion.apply(f, a.astype(np.int16), d)
    with pytest.raises(TypeError):
        motion.apply(f, a, motion.taps_of(M.KERNELS['k3_n2']))             # a table is not a MotionDraws
    with pytest.raises(ValueError):
        motion.apply(f[..., :2], a, d)
    with pytest.raises(ValueError):
        motion.apply(f, a[..., :8], d)                                     # alphas of another size
    with pytest.raises(ValueError):
        motion.apply(np.zeros((3,), np.uint8), None, d)
    with pytest.raises(ValueError):
        motion.blur_planes(np.zeros((1, motion.MAX_SIDE + 1), np.uint8), d)
    with pytest.raises(ValueError):
        motion.blur_frames(f, motion.MotionDraws())                        # nothing to blur with
    with pytest.raises(ValueError):
        motion.blur_planes(a, motion.MotionDraws())
    with pytest.raises(TypeError):
        DevicePreprocessor().train_item_motion(f, a, a, None, 'kernel')
    if not torch.cuda.is_available():                                      # well-formed calls: the package's own error, never torch's
        for call in (lambda: motion.apply(f, a, d), lambda: motion.apply(f, a, motion.MotionDraws()), lambda: motion.apply(f, None, d, normalize=True),
                     lambda: motion.blur_frames(f, d), lambda: motion.blur_planes(a, d), lambda: d.to()):
            with pytest.raises(hip.MaggieHipError):
                call()
