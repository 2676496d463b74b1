"""The device cut-outs (maggie_amd.utils.cutout, csrc/cutout.hip) against the NumPy statement of tests/cutout_restatement.py, which
tests/test_cutout_cpu.py holds against SciPy's uniform filter and against a scene with a known foreground. Every comparison is exact
(`torch.equal`): the window sums are integers and the formula is fp64 with every operation rounded on its own, on both sides."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cutout_restatement as C                                        # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import cutout, matteout, postprocessing        # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 5), (3, 2), (5, 7), (64, 65), (67, 257), (200, 331)]
RADII = [(90, 6), (1, 1), (2, 7), (255, 3)]
_SCENES = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene(H, W, T=1, P=2, seed=0):
    """(frames (T, H, W, 3) uint8, alpha (T, P, H, W) uint8): distinct planes, each with 0, 255 and everything between. Computed once, never changed."""
    key = (H, W, T, P, seed)
    if key not in _SCENES:
        rs = np.random.RandomState(1000 * seed + 7 * H + W)
        frames = rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        planes = []
        for k in range(T * P):
            cy, cx = rs.uniform(0.2, 0.8) * H, rs.uniform(0.2, 0.8) * W
            soft = np.clip(1.6 - np.hypot(yy - cy, xx - cx) / (0.25 * max(H, W) + 1.0), 0.0, 1.0)
            a = np.floor(soft * 255.0 + 0.5)
            noisy = rs.random_sample((H, W)) < 0.15
            a[noisy] = rs.randint(0, 256, size=int(noisy.sum()))
            planes.append(a.astype(np.uint8))
        _SCENES[key] = (frames, np.stack(planes).reshape(T, P, H, W))
    return _SCENES[key]


@pytest.mark.parametrize('radii', RADII, ids=lambda r: 'r%d_%d' % r)
@pytest.mark.parametrize('H,W', SIZES)
def test_estimate_equals_the_statement(H, W, radii):
    frames, alpha = scene(H, W)
    got = cutout.estimate_foreground(frames, dev(alpha), radii=radii)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1, 2, H, W, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(C.estimate_all(frames, alpha, radii)))


@pytest.mark.parametrize('H,W', [(5, 7), (67, 257)])
def test_planes_of_two_frames_and_three_instances(H, W):
    frames, alpha = scene(H, W, T=2, P=3, seed=1)
    want = torch.from_numpy(C.estimate_all(frames, alpha))
    got = cutout.estimate_foreground(dev(frames), dev(alpha))
    assert tuple(got.shape) == (2, 3, H, W, 3) and torch.equal(got.cpu(), want)
    assert torch.equal(cutout.estimate_foreground(frames, dev(alpha[None])).cpu(), want)                 # (..., P, H, W) with T * P planes
    one = cutout.estimate_foreground(frames[1], dev(alpha[1]))                                            # a single frame (H, W, 3)
    assert tuple(one.shape) == (1, 3, H, W, 3) and torch.equal(one.cpu()[0], want[1])


def test_chunks_of_planes_give_the_same_bytes(monkeypatch):
    frames, alpha = scene(67, 257, T=2, P=3, seed=1)
    want = cutout.cutout(frames, dev(alpha))
    for planes in (1, 4):                                               # six planes as 1 + 1 + ... and as 3 + 3
        monkeypatch.setattr(cutout, 'SCRATCH_BYTES', planes * 28 * 67 * 257)
        assert torch.equal(cutout.cutout(frames, dev(alpha)), want), planes
    monkeypatch.setattr(cutout, 'SCRATCH_BYTES', 2 * 28 * 67 * 257)     # three planes as 2 + 1: a last chunk that is not full
    assert torch.equal(cutout.cutout(frames[1], dev(alpha[1])), want[1:]), 'a short last chunk'
    assert torch.equal(want.cpu(), torch.from_numpy(C.cutout_all(frames, alpha)))


@pytest.mark.parametrize('radii', [(90, 6), (2, 7)], ids=lambda r: 'r%d_%d' % r)
def test_float_alpha_is_taken_as_its_unit_byte(radii):
    H, W = 64, 65
    frames, a8 = scene(H, W)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    edge = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)), [np.nan, -0.5, 1.5, -0.0, np.inf, -np.inf]]).astype(np.float32)
    x = (a8.astype(np.float32) / np.float32(255)).copy()
    x[0, 1].reshape(-1)[:edge.size] = edge
    assert np.isnan(x).any() and (x == -0.5).any() and (x == 1.5).any()
    want_bytes = np.stack([C.alpha_byte(p) for p in x[0]])[None]
    got = cutout.estimate_foreground(frames, dev(x), radii=radii)
    assert torch.equal(got.cpu(), torch.from_numpy(C.estimate_all(frames, want_bytes, radii)))
    rgba = cutout.cutout(frames, dev(x), radii=radii).cpu()
    assert torch.equal(rgba[..., 3], torch.from_numpy(want_bytes))
    assert torch.equal(rgba, torch.from_numpy(C.cutout_all(frames, x, radii)))


def test_alpha_all_zero_and_all_opaque():
    frames, _ = scene(64, 65)
    for v in (0, 255):
        a = np.full((1, 2, 64, 65), v, np.uint8)
        est = cutout.estimate_foreground(frames, dev(a)).cpu()
        assert torch.equal(est, torch.from_numpy(C.estimate_all(frames, a)))
        rgba = cutout.cutout(frames, dev(a)).cpu().numpy()
        if v == 255:
            assert np.array_equal(est.numpy(), np.broadcast_to(frames[:, None], est.shape))
            assert np.array_equal(rgba[..., :3], est.numpy()) and (rgba[..., 3] == 255).all()
        else:
            assert not rgba.any()


def test_a_frame_view_that_is_not_contiguous():
    frames, alpha = scene(67, 257)
    wide = np.zeros((1, 67, 300, 4), np.uint8)
    wide[:, :, 20:277, 1:] = frames
    view = dev(wide)[:, :, 20:277, 1:]
    assert not view.is_contiguous()
    a = dev(np.concatenate([alpha, alpha], 1))[:, ::2]                   # every other plane of a wider tensor
    assert not a.is_contiguous()
    want = torch.from_numpy(C.estimate_all(frames, alpha[:, [0, 0]]))
    assert torch.equal(cutout.estimate_foreground(view, a).cpu(), want)


def test_cutout_is_rgba_with_hidden_colour_removed():
    frames, alpha = scene(67, 257, T=2, P=3, seed=1)
    got = cutout.cutout(frames, dev(alpha)).cpu().numpy()
    assert got.shape == (2, 3, 67, 257, 4)
    assert np.array_equal(got[..., 3], alpha)
    est = cutout.estimate_foreground(frames, dev(alpha)).cpu().numpy()
    hidden = alpha == 0
    assert hidden.any() and not got[..., :3][hidden].any()
    assert np.array_equal(got[..., :3][~hidden], est[~hidden])
    assert est[hidden].any()                                            # the estimate itself has colour there: the rule did something
    assert np.array_equal(got, C.cutout_all(frames, alpha))


@pytest.mark.parametrize('snap', [False, True])
def test_cutout_behind_the_reverse_transform(snap):
    rs = np.random.RandomState(31)
    info = [{'name': 'resize', 'ori_size': (37, 61)}, {'name': 'padding', 'pad_size': (5, 8)}]
    frames = rs.randint(0, 256, size=(2, 37, 61, 3)).astype(np.uint8)
    x = dev(np.clip(rs.uniform(-0.3, 1.3, size=(1, 2, 3, 40, 56)), 0, 1).astype(np.float32))
    full = postprocessing.reverse_transform_tensor(x, info, snap=snap)
    assert tuple(full.shape) == (1, 2, 3, 37, 61)
    got = cutout.cutout(frames, x, transform_info=info, snap=snap)
    assert tuple(got.shape) == (2, 3, 37, 61, 4)
    assert torch.equal(got.cpu(), torch.from_numpy(C.cutout_all(frames, full.cpu().numpy()[0])))


def test_cutout_replays_from_a_graph():
    """Resident inputs, one chain of launches (the byte conversion, then four per chunk), nothing read back."""
    rs = np.random.RandomState(3)
    info = [{'name': 'resize', 'ori_size': (37, 61)}, {'name': 'padding', 'pad_size': (5, 8)}]
    frames = dev(rs.randint(0, 256, size=(2, 37, 61, 3)).astype(np.uint8))
    x = dev(rs.random_sample((2, 3, 40, 56)).astype(np.float32))
    eager = cutout.cutout(frames, x, transform_info=info, snap=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cutout.cutout(frames, x, transform_info=info, snap=True)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x2 = dev(rs.random_sample((2, 3, 40, 56)).astype(np.float32))
    want = cutout.cutout(frames, x2, transform_info=info, snap=True)
    x.copy_(x2)                                                         # a replay reads what its input holds now
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_no_planes_no_launch():
    frames, _ = scene(5, 7)
    e = cutout.estimate_foreground(frames, torch.empty((1, 0, 5, 7), dtype=torch.uint8, device='cuda'))
    assert tuple(e.shape) == (1, 0, 5, 7, 3) and e.dtype == torch.uint8
    c = cutout.cutout(frames, torch.empty((0, 5, 7), dtype=torch.float32, device='cuda'))
    assert tuple(c.shape) == (1, 0, 5, 7, 4)


def test_errors_are_raised_before_any_launch():
    frames, alpha = scene(5, 7)
    a = dev(alpha)
    with pytest.raises(TypeError):
        cutout.estimate_foreground(dev(frames).float(), a)
    with pytest.raises(TypeError):
        cutout.estimate_foreground(frames, a.half())
    with pytest.raises(TypeError):
        cutout.cutout(frames, alpha)                                    # an array: the alpha is a device tensor
    with pytest.raises(ValueError):
        cutout.estimate_foreground(frames, a[..., :6])
    with pytest.raises(ValueError):
        cutout.cutout(frames, a, radii=(256, 6))
    with pytest.raises(ValueError):
        cutout.cutout(frames, a, radii=(90, 0))
    with pytest.raises(ValueError):
        cutout.cutout(frames, a.float(), transform_info=[{'name': 'resize', 'ori_size': (9, 9)}])      # comes out at another size
    L = hip.lib()
    P, I, Lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    f = dev(frames)
    rows = torch.zeros((2, 7, 5, 7), dtype=torch.int32, device='cuda')
    fb = torch.zeros((2, 2, 5, 7, 3), dtype=torch.uint8, device='cuda')
    out = torch.zeros((2, 5, 7, 4), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()

    def est(fr=f.data_ptr(), al=a.data_ptr(), T=1, n=2, H=5, W=7, r0=90, r1=6, rw=rows.data_ptr(), f1=fb[0].data_ptr(), b1=fb[1].data_ptr(), chunk=2,
            o=out.data_ptr(), ch=4):
        return L.mg_cutout_estimate(P(fr), P(al), Lg(T), I(n), I(H), I(W), I(r0), I(r1), P(rw), P(f1), P(b1), Lg(chunk), P(o), I(ch), P(None))

    assert est(fr=None) == -2 and est(al=None) == -2 and est(rw=None) == -2 and est(f1=None) == -2 and est(b1=None) == -2 and est(o=None) == -2
    assert est(r0=0) == -2 and est(r0=256) == -2 and est(r1=0) == -2 and est(r1=256) == -2 and est(H=0) == -2 and est(W=0) == -2
    assert est(H=cutout.MAX_SIDE + 1) == -2 and est(ch=2) == -2 and est(ch=5) == -2 and est(chunk=0) == -2 and est(T=-1) == -2 and est(n=-1) == -2
    assert est(rw=rows.data_ptr() + 2) == -2 and est(o=out.data_ptr() + 1) == -2
    assert L.mg_cutout_alpha_bytes(P(None), Lg(4), P(out.data_ptr()), P(None)) == -2
    assert L.mg_cutout_alpha_bytes(P(rows.data_ptr() + 1), Lg(4), P(out.data_ptr()), P(None)) == -2
    assert est(T=0) == 0                                                # nothing to do is not an error, and launches nothing
    torch.cuda.synchronize()
    assert not bool(rows.any()) and not bool(fb.any()) and not bool(out.any())
    v = [ctypes.c_int() for _ in range(5)]
    assert L.mg_cutout_limits(*[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v][3:] == [cutout.MAX_RADIUS, cutout.MAX_SIDE]


def stub_model(batch):
    """A fixed smooth function of batch['mask'] with values in [0, 1] (the stub of tests/test_gpu_matteout.py)."""
    m = batch['mask'].float()
    s = torch.nn.functional.avg_pool2d(m.reshape((-1, 1) + tuple(m.shape[-2:])), 31, 1, 15, count_include_pad=True).reshape(m.shape)
    return {'refined_masks': torch.clamp(1.5 * s - 0.2, 0.0, 1.0)}


@pytest.mark.parametrize('post', [False, True])
def test_predict_image_returns_the_cutouts_of_its_alpha(post):
    rs = np.random.RandomState(12)
    frame = rs.randint(0, 256, size=(40, 56, 3)).astype(np.uint8)
    label = np.zeros((40, 56), np.uint8)
    label[5:30, 4:25], label[12:38, 30:52], label[0:3, 50:56] = 4, 9, 9
    plain = matteout.predict_image(stub_model, frame, label, postprocess=post)
    assert sorted(plain) == ['alpha', 'composites']                      # the default is unchanged
    r = matteout.predict_image(stub_model, frame, label, postprocess=post, cutouts=True)
    assert torch.equal(r['alpha'], plain['alpha']) and torch.equal(r['composites'], plain['composites'])
    assert tuple(r['cutouts'].shape) == (2, 40, 56, 4) and r['cutouts'].dtype == torch.uint8
    assert torch.equal(r['cutouts'], cutout.cutout(frame, r['alpha'])[0])
    assert np.array_equal(r['cutouts'].cpu().numpy(), C.cutout_all(frame[None], r['alpha'].cpu().numpy()[None])[0])
    empty = matteout.predict_image(stub_model, frame, np.zeros((40, 56), np.uint8), cutouts=True)
    assert tuple(empty['cutouts'].shape) == (0, 40, 56, 4)


def test_save_cutouts_writes_rgba_files(tmp_path):
    frames, alpha = scene(67, 257, T=1, P=2)
    c = cutout.cutout(frames, dev(alpha))[0]
    paths = cutout.save_cutouts(c, str(tmp_path / 'cut'), 'frame0007')
    assert paths == [str(tmp_path / 'cut' / ('%02d_frame0007.png' % i)) for i in range(2)]
    for p, want in zip(paths, c.cpu().numpy()):
        im = Image.open(p)
        assert im.mode == 'RGBA' and np.array_equal(np.asarray(im), want)
        with open(p, 'rb') as f:
            assert f.read() == C.encode_colour(want)[0]
    assert cutout.save_cutouts(c[:0], str(tmp_path / 'none'), 'x') == []
