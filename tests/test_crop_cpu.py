"""Host side of the device training crop (maggie_amd.utils.crop): the fixture against the restatement, `crop.draw` against hand-replayed
RandomState calls, the speculative window draws, the padding-branch tables, the argument errors. No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import crop_restatement as C                                          # noqa: E402
import geometry_restatement as R                                      # noqa: E402
from helpers import load_golden, unpack_bits                         # noqa: E402
from maggie_amd.hip import MaggieHipError                             # noqa: E402
from maggie_amd.utils import crop, geometry, maskgen                  # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

CASES = list(C.GOLDEN)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _draw(name, calls=None):
    """`crop.draw` on a case with the restated box and hit test; `calls` collects what was asked."""
    c = C.GOLDEN[name]
    _, alphas, _ = C.golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])

    def box():
        if calls is not None:
            calls.append('bbox')
        return C.bbox(alphas)

    def hits(windows):
        if calls is not None:
            calls.append(list(windows))
        return C.first_hit(alphas, windows, c['crop'])
    return crop.draw(rs, c['h'], c['w'], c['crop'], c['pp'], c['fp'], box, hits), rs


@pytest.mark.parametrize('name', CASES)
def test_fixture_equals_the_restatement(name):
    d = load_golden('crop_pinned.npz')
    assert os.path.getsize(os.path.join(GOLDEN_DIR, 'crop_pinned.npz')) <= os.path.getsize(os.path.join(GOLDEN_DIR, 'geometry_pinned.npz'))
    r, rs = C.golden_run(name)
    assert np.array_equal(R.unpack_rows(d[name + '.frames']), r['frames']) and np.array_equal(R.unpack_rows(d[name + '.alphas']), r['alphas'])
    assert np.array_equal(unpack_bits(d[name + '.masks'], r['masks'].shape) * 255, r['masks'])
    x0, y0 = r['window'] if r['branch'] == 'crop' else (0, 0)
    assert d[name + '.info'].tolist() == [int(r['branch'] == 'pad'), x0, y0, r['pairs'], int(r['flip'])] + list(r['box'])
    assert np.array_equal(d[name + '.state'], C.state_digest(rs))
    # the table-level operators give the same arrays as the code path
    frames, alphas, masks = C.golden_inputs(name)
    c = C.GOLDEN[name]
    if r['branch'] == 'crop':
        got = [C.gather(x, r['window'], c['crop'], r['flip']) for x in (frames, alphas, masks)]
    else:
        got = [C.padresize(frames, c['crop'], r['flip'], R.INTER_LINEAR), C.padresize(alphas, c['crop'], r['flip'], R.INTER_LINEAR),
               C.padresize(masks, c['crop'], r['flip'], R.INTER_NEAREST)]
    assert all(np.array_equal(g, r[k]) for g, k in zip(got, ('frames', 'alphas', 'masks')))


@pytest.mark.parametrize('name', CASES)
def test_draw_against_hand_replayed_generator_calls(name):
    """The calls the reference makes, written out by hand from transforms.py:197-215,242,292 with the fixture's window count."""
    d = load_golden('crop_pinned.npz')
    c = C.GOLDEN[name]
    pad, x0, y0, pairs, flip, min_x, max_x, min_y, max_y = d[name + '.info'].tolist()
    ch, cw = c['crop']
    hand = np.random.RandomState(c['rs_seed'])
    branch_draw = hand.rand()
    assert (branch_draw > c['pp']) == (not pad)
    windows = []
    if not pad:
        hi_x, hi_y = max(max_x - cw, min_x + 1), max(max_y - ch, min_y + 1)
        for _ in range(pairs):
            x = hand.randint(min_x, hi_x)
            y = hand.randint(min_y, hi_y)
            windows.append((min(x, c['w'] - cw), min(y, c['h'] - ch)))
    flip_draw = hand.rand()
    calls = []
    draws, rs = _draw(name, calls)
    assert np.array_equal(C.state_digest(rs), C.state_digest(hand)) and np.array_equal(C.state_digest(rs), d[name + '.state'])
    assert draws.flip == bool(flip) == (flip_draw < c['fp']) and (draws.H, draws.W) == (c['h'], c['w'])
    if pad:
        assert calls == [] and draws.branch == 'pad' and draws.window is None                    # no box, no hit test on the padding branch
        assert (draws.out_h, draws.out_w) == (cw, ch)                                            # dsize = (ch, cw): ch wide, cw high
    else:
        assert calls[0] == 'bbox' and len(calls) == 2 and len(calls[1]) == 3 and calls[1][:pairs] == windows
        assert draws.branch == 'crop' and draws.pairs == pairs and draws.window.dtype == np.int32
        assert draws.window.tolist() == [x0, y0, flip] == list(windows[-1]) + [flip]
        assert draws.box == (min_x, max_x, min_y, max_y) and (draws.out_h, draws.out_w) == (ch, cw)


def test_speculative_draws_leave_the_sequential_state():
    """Whatever the hit test answers, three candidates drawn ahead and `pairs` of them replayed leave the state of drawing `pairs` in sequence."""
    for answer, pairs in ((0, 1), (1, 2), (2, 3), (None, 3)):
        for box in ((40, 20, 130, 10, 80), (0, 160, -1, 96, -1), (1, 159, 159, 95, 95)):
            rs, seq = np.random.RandomState(77), np.random.RandomState(77)
            asked = []
            draws = crop.draw(rs, 96, 160, (64, 48), 0.0, 0.5, lambda: box, lambda w: asked.append(list(w)) or answer)
            seq.rand()
            min_x, max_x, min_y, max_y = (box[1], box[2], box[3], box[4]) if box[0] else (0, 160, 0, 96)
            hi_x, hi_y = max(max_x - 48, min_x + 1), max(max_y - 64, min_y + 1)
            wins = [(min(seq.randint(min_x, hi_x), 160 - 48), min(seq.randint(min_y, hi_y), 96 - 64)) for _ in range(pairs)]
            flip = seq.rand() < 0.5
            assert np.array_equal(C.state_digest(rs), C.state_digest(seq))
            assert draws.pairs == pairs and draws.window.tolist() == list(wins[-1]) + [int(flip)] and asked[0][:pairs] == wins
    with pytest.raises(ValueError):
        crop.draw(np.random.RandomState(1), 96, 160, (64, 48), 0.0, 0.5, lambda: (1, 3, 3, 3, 3), lambda w: 3)


@pytest.mark.parametrize('H,W,crop_size', [(96, 70, (64, 64)), (96, 157, (48, 80)), (64, 64, (64, 64)), (99, 157, (16, 33))])
def test_padding_tables_are_the_resize_axes_of_the_padded_size(H, W, crop_size):
    ch, cw = crop_size
    for flip in (False, True):
        pad_h, pad_w, out_h, out_w, linear, nearest = crop.pad_tables(H, W, crop_size, flip)
        assert (pad_h, pad_w) == ((0, (H - W) // 2) if H > W else ((W - H) // 2, 0)) == crop.pad_amounts(H, W)
        assert (out_h, out_w) == (cw, ch) and linear.dtype == nearest.dtype == np.int32
        Hp, Wp = H + 2 * pad_h, W + 2 * pad_w
        x = np.stack([a.astype(np.int32) for a in maskgen.resize_axis(Wp, out_w, 1.0 / (out_w / Wp))], 1)
        y = np.stack([a.astype(np.int32) for a in maskgen.resize_axis(Hp, out_h, 1.0 / (out_h / Hp))], 1)
        nx, ny = geometry.nearest_axis(Wp, out_w), geometry.nearest_axis(Hp, out_h)
        if flip:
            x, nx = x[::-1], nx[::-1]
        assert np.array_equal(linear, np.concatenate([x.reshape(-1), y.reshape(-1)]))
        assert np.array_equal(nearest, np.concatenate([nx, ny]))
        # the tables, read the way the kernel reads them, give the restated pad-and-resize
        a = np.random.default_rng(H + W).integers(0, 256, (1, H, W), dtype=np.uint8)
        padded = np.pad(a[0], ((pad_h, pad_h), (pad_w, pad_w))).astype(np.int32)
        xt, yt = linear[:3 * out_w].reshape(out_w, 3), linear[3 * out_w:].reshape(out_h, 3)
        rows = padded[:, xt[:, 0]] * xt[:, 1] + padded[:, np.minimum(xt[:, 0] + 1, Wp - 1)] * xt[:, 2]
        lin = (((yt[:, 1, None] * (rows[yt[:, 0]] >> 4)) >> 16) + ((yt[:, 2, None] * (rows[np.minimum(yt[:, 0] + 1, Hp - 1)] >> 4)) >> 16) + 2) >> 2
        assert np.array_equal(lin.astype(np.uint8), C.padresize(a, crop_size, flip, R.INTER_LINEAR)[0])
        near = padded[nearest[out_w:][:, None], nearest[:out_w][None, :]]
        assert np.array_equal(near.astype(np.uint8), C.padresize(a, crop_size, flip, R.INTER_NEAREST)[0])


def test_argument_errors_raise_before_the_device():
    rs = np.random.RandomState(0)
    f = np.zeros((1, 32, 48, 3), np.uint8)
    a = np.zeros((2, 32, 48), np.uint8)
    with pytest.raises(ValueError, match=r'Crop size \[64, 64\] is larger than image size \(32, 48\)'):
        crop.draw(rs, 32, 48, [64, 64], 0.5, 0.5, None, None)
    with pytest.raises(ValueError, match=r'Crop size \(16, 64\) is larger than image size \(32, 48\)'):
        crop.draw_on_device(rs, a, (16, 64))
    assert np.array_equal(C.state_digest(rs), C.state_digest(np.random.RandomState(0)))          # nothing was drawn
    with pytest.raises(ValueError, match=r'Crop size'):
        C.crop_flip(f, a, None, (64, 64), rs, 0.5, 0.5)
    with pytest.raises(TypeError):
        crop.draw(rs, 32, 48, 16, 0.5, 0.5, None, None)
    with pytest.raises(TypeError):
        crop.draw(rs, 32, 48, (16.0, 16), 0.5, 0.5, None, None)
    with pytest.raises(TypeError):
        crop.draw_on_device(rs, a.astype(np.float32), (16, 16))
    with pytest.raises(ValueError):
        crop.draw_on_device(rs, np.zeros((0, 32, 48), np.uint8), (16, 16))
    draws = crop.draw(np.random.RandomState(1), 32, 48, (16, 16), 0.0, 0.5, lambda: (0, 48, -1, 32, -1), lambda w: None)
    pads = crop.draw(np.random.RandomState(1), 32, 48, (16, 16), 1.0, 0.5, None, None)
    assert draws.branch == 'crop' and pads.branch == 'pad' and not draws.on_device and not pads.on_device
    with pytest.raises(TypeError):
        crop.apply(f, a, None, (0, 0, 0))
    with pytest.raises(TypeError):
        crop.apply(f.astype(np.int32), a, None, draws)
    with pytest.raises(ValueError):
        crop.apply(np.zeros((1, 32, 48, 4), np.uint8), a, None, draws)
    with pytest.raises(ValueError):
        crop.apply(np.zeros((1, 32, 40, 3), np.uint8), a, None, draws)                           # not the size the draws were made for
    with pytest.raises(ValueError):
        crop.apply(f, np.zeros((2, 32, 40), np.uint8), None, draws)
    with pytest.raises(ValueError):
        crop.apply(f, a, np.zeros((2, 30, 48), np.uint8), pads)
    with pytest.raises(ValueError):
        crop.apply(f, a, None, draws, lut=np.zeros((256,), np.uint8))
    with pytest.raises(ValueError):
        crop.apply(f, a, None, draws, lut=np.zeros((3, 256), np.int32))
    with pytest.raises(ValueError):
        crop.window_hits(a, [(0, 0)] * 4, (16, 16))
    with pytest.raises(ValueError):
        DevicePreprocessor().train_item(f[0], a, None, draws)


def test_no_gpu_raises_maggie_hip_error():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    f = np.zeros((1, 32, 48, 3), np.uint8)
    a = np.zeros((2, 32, 48), np.uint8)
    draws = crop.draw(np.random.RandomState(1), 32, 48, (16, 16), 0.0, 0.5, lambda: (0, 48, -1, 32, -1), lambda w: None)
    with pytest.raises(MaggieHipError):
        crop.apply(f, a, None, draws)
    with pytest.raises(MaggieHipError):
        crop.draw_on_device(np.random.RandomState(3), a, (16, 16), padding_prob=0.0)
    with pytest.raises(MaggieHipError):
        draws.to()
    with pytest.raises(MaggieHipError):
        DevicePreprocessor().train_item(f, a, a, draws)
    # the padding branch asks the device nothing: it draws without one
    pads = crop.draw_on_device(np.random.RandomState(3), a, (16, 16), padding_prob=1.0)
    assert pads.branch == 'pad'


def test_c_entries_reject_bad_arguments_before_any_launch():
    from maggie_amd import hip
    I, L = ctypes.c_int, ctypes.c_long
    lib = hip.lib()
    for fn in (lib.mg_crop_bbox, lib.mg_crop_hits, lib.mg_crop_gather, lib.mg_crop_padresize):
        fn.restype = ctypes.c_int
    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def box(P=1, H=4, W=4):
        return lib.mg_crop_bbox(None, None, L(P), I(H), I(W), None)

    def hits(n=1, P=1, H=4, W=4, ch=2, cw=2):
        return lib.mg_crop_hits(None, None, None, I(n), L(P), I(H), I(W), I(ch), I(cw), None)

    def gather(images=1, C=1, H=4, W=4, ch=2, cw=2, epi=0, mean=None, lut=None):
        return lib.mg_crop_gather(None, None, None, lut, L(images), I(C), I(H), I(W), I(ch), I(cw), I(epi), mean, mean, None)

    def pad(images=1, C=1, H=4, W=4, ph=0, pw=0, dh=2, dw=2, interp=0, epi=0, mean=None, lut=None):
        return lib.mg_crop_padresize(None, None, None, None, lut, L(images), I(C), I(H), I(W), I(ph), I(pw), I(dh), I(dw), I(interp), I(epi), mean,
                                     mean, None)
    assert box() == hits() == gather() == pad() == -2                       # null pointers
    assert hits(n=0) == gather(images=0) == pad(images=0) == 0
    for bad in (dict(P=0), dict(P=crop.MAX_PLANES + 1), dict(H=0), dict(W=-1)):
        assert box(**bad) == -2 and hits(**bad) == -2, bad
    for bad in (dict(n=-1), dict(n=4), dict(ch=5), dict(cw=5), dict(ch=0)):
        assert hits(**bad) == -2, bad
    fake = ctypes.c_void_p(16)                                                # a non-null lut: never read, the shape checks come first
    for bad in (dict(C=2), dict(H=0), dict(ch=5), dict(cw=0), dict(epi=2), dict(epi=1), dict(epi=1, C=3), dict(epi=1, C=1, mean=three),
                dict(lut=fake), dict(images=-1)):
        assert gather(**bad) == -2, bad
    for bad in (dict(C=4), dict(W=0), dict(ph=-1), dict(pw=-1), dict(dh=0), dict(dw=0), dict(interp=2), dict(epi=3), dict(epi=1),
                dict(epi=1, C=1, mean=three), dict(lut=fake), dict(images=-1)):
        assert pad(**bad) == -2, bad


def test_python_constants_match_the_library():
    from maggie_amd import hip
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert hip.lib().mg_crop_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert (a.value, b.value, c.value) == (crop.MAX_WINDOWS, crop.MAX_PLANES, crop.CHUNK)
    assert hip.lib().mg_crop_limits(None, None, None) == -2
    header = open(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, 'include', 'maggie_hip.h')).read()
    assert '#define MG_CROP_RAW %d\n' % crop.RAW in header and '#define MG_CROP_NORM %d\n' % crop.NORM in header
    assert (crop.LINEAR, crop.NEAREST) == (geometry.LINEAR, geometry.NEAREST)


def test_call_signature_is_unchanged():
    sig = inspect.signature(DevicePreprocessor.__call__)
    assert str(sig) == '(self, frames_u8, alphas_u8=None, masks_u8=None, slot_ids=None, *, transition=None, trimap=False, mask_draws=None)'
    assert str(inspect.signature(DevicePreprocessor.eval_item)) == \
        '(self, frames_u8, ori_alphas_u8, masks_u8=None, *, short_size=768, divisor=64, trimap=True)'
    assert str(inspect.signature(DevicePreprocessor.predict_item)) == '(self, frame_u8, instance_masks_u8, *, short_size=576, divisor=64)'
    assert str(inspect.signature(DevicePreprocessor.train_item)) == \
        '(self, frames_u8, alphas_u8, masks_u8, crop_draws, slot_ids=None, *, transition=None, mask_draws=None, lut=None)'
