"""The device matte refinement (maggie_amd.utils.refine, csrc/refine.hip) against the NumPy statement of tests/refine_restatement.py, which
tests/test_refine_cpu.py holds against SciPy's uniform filter, NumPy's solver and a scene with a known alpha. Every comparison is exact
(`torch.equal` / `array_equal`): the window sums are integers and everything behind them is fp64 with every operation rounded on its own, on
both sides."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cutout_restatement as C                                        # noqa: E402
import refine_restatement as R                                        # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import cutout, geometry, matteout, refine       # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [((1, 1), (1, 1), 5), ((1, 1), (3, 2), 5), ((5, 7), (11, 13), 64), ((5, 7), (3, 4), 5), ((9, 8), (9, 8), 2), ((64, 65), (131, 257), 5),
         ((67, 257), (200, 331), 5)]
PARAMS = [(5, 1e-4), (1, 1e-2), (3, 1e-6), (64, 1.0)]
_SCENES = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene(h, w, H, W, T=1, P=2, seed=0):
    """(frames (T, H, W, 3), guides (T, h, w, 3), alpha (T, P, h, w)), all uint8: planes that follow the guide (so the coefficients are not
    small), with 0, 255 and everything between, and noise. Computed once, never changed."""
    key = (h, w, H, W, T, P, seed)
    if key not in _SCENES:
        rs = np.random.RandomState(1000 * seed + 131 * h + 7 * w + 3 * H + W)
        frames = rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        smooth = 128.0 + 90.0 * np.sin(xx / 3.0 + 0.3 * yy)[..., None] * np.array([1.0, -0.6, 0.3])
        guides = np.clip(smooth[None] + rs.normal(0, 25, (T, h, w, 3)), 0, 255).astype(np.uint8)
        planes = []
        for k in range(T * P):
            g = guides[k // P].astype(np.float64)
            a = np.clip(2.0 * (g[..., k % 3] - 64.0) + 0.5 * (g[..., (k + 1) % 3] - 128.0), 0, 255)
            noisy = rs.random_sample((h, w)) < 0.1
            a[noisy] = rs.randint(0, 256, size=int(noisy.sum()))
            planes.append(a.astype(np.uint8))
        _SCENES[key] = (frames, guides, np.stack(planes).reshape(T, P, h, w))
    return _SCENES[key]


@pytest.mark.parametrize('r,eps', PARAMS, ids=lambda v: str(v))
@pytest.mark.parametrize('lo,hi,own_r', SIZES, ids=lambda v: str(v).replace(' ', ''))
def test_refine_equals_the_statement(lo, hi, own_r, r, eps):
    (h, w), (H, W) = lo, hi
    frames, guides, alpha = scene(h, w, H, W)
    for rr in sorted({r, own_r}):
        got = refine.refine(frames, dev(alpha), guide=guides, radius=rr, eps=eps)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1, 2, H, W)
        assert torch.equal(got.cpu(), torch.from_numpy(R.refine_all(frames, guides, alpha, rr, eps))), rr


def test_the_frames_are_their_own_guide_at_equal_sizes():
    frames, _, alpha = scene(9, 8, 9, 8)
    got = refine.refine(frames, dev(alpha), radius=2)
    assert torch.equal(got.cpu(), torch.from_numpy(R.refine_all(frames, frames, alpha, 2, R.EPS)))


def test_padding_is_cropped_and_the_guide_is_the_resized_frame():
    plan = geometry.plan(270, 480, 144, 64)
    assert (plan.rh, plan.rw, plan.pad_h, plan.pad_w) == (144, 256, 48, 0)
    rs = np.random.RandomState(9)
    frames, guides, alpha = scene(144, 256, 270, 480, P=2, seed=2)
    x = np.full((1, 2, 192, 256), np.nan, np.float32)                   # poisoned padding rows
    x[:, :, :144] = alpha.astype(np.float32) / np.float32(255) + rs.uniform(0, 0.003, alpha.shape).astype(np.float32)
    bytes_ = np.stack([C.alpha_byte(p) for p in x[0, :, :144]])[None]
    info = plan.transform_info
    guide = geometry.resize(dev(frames), (256, 144), 'linear', channels=3)
    assert tuple(guide.shape) == (1, 144, 256, 3)
    own = refine.refine(frames, dev(x), transform_info=info)
    given = refine.refine(frames, dev(x), transform_info=info, guide=guide)
    assert tuple(own.shape) == (1, 2, 270, 480) and torch.equal(own, given)
    assert torch.equal(own.cpu(), torch.from_numpy(R.refine_all(frames, guide.cpu().numpy(), bytes_)))
    poisoned = x.copy()
    poisoned[:, :, 144:] = 7.0
    assert torch.equal(refine.refine(frames, dev(poisoned), transform_info=info), own)
    with pytest.raises(ValueError):
        refine.refine(frames, dev(x), transform_info=info, guide=frames)           # a guide at the frame's size where the alpha is smaller


def test_planes_of_two_frames_and_three_instances(monkeypatch):
    h, w, H, W = 67, 257, 200, 331
    frames, guides, alpha = scene(h, w, H, W, T=2, P=3, seed=1)
    want = torch.from_numpy(R.refine_all(frames, guides, alpha))
    got = refine.refine(dev(frames), dev(alpha), guide=dev(guides))
    assert tuple(got.shape) == (2, 3, H, W) and torch.equal(got.cpu(), want)
    assert torch.equal(refine.refine(frames, dev(alpha[None]), guide=guides).cpu(), want)                 # (..., P, h, w) with T * P planes
    one = refine.refine(frames[1], dev(alpha[1]), guide=guides[1])                                        # a single frame (H, W, 3)
    assert tuple(one.shape) == (1, 3, H, W) and torch.equal(one.cpu()[0], want[1])
    monkeypatch.setattr(refine, 'SCRATCH_BYTES', (72 + 96 * 3) * h * w)                                   # the clip in chunks of one frame
    assert torch.equal(refine.refine(frames, dev(alpha), guide=guides).cpu(), want)
    none = refine.refine(frames, torch.empty((2, 0, h, w), dtype=torch.uint8, device='cuda'), guide=guides)
    assert tuple(none.shape) == (2, 0, H, W) and none.dtype == torch.uint8
    nonef = refine.refine(frames[0], torch.empty((0, h, w), dtype=torch.float32, device='cuda'), as_float=True)
    assert tuple(nonef.shape) == (1, 0, H, W) and nonef.dtype == torch.float32


def test_views_that_are_not_contiguous():
    h, w, H, W = 64, 65, 131, 257
    frames, guides, alpha = scene(h, w, H, W)
    wide = np.zeros((1, H, 300, 4), np.uint8)
    wide[:, :, 20:277, 1:] = frames
    fview = dev(wide)[:, :, 20:277, 1:]
    gwide = np.zeros((1, h, 80, 4), np.uint8)
    gwide[:, :, 5:70, :3] = guides
    gview = dev(gwide)[:, :, 5:70, :3]
    a = dev(np.concatenate([alpha, alpha], 1))[:, ::2]                  # every other plane of a wider tensor
    assert not fview.is_contiguous() and not gview.is_contiguous() and not a.is_contiguous()
    want = torch.from_numpy(R.refine_all(frames, guides, alpha[:, [0, 0]]))
    assert torch.equal(refine.refine(fview, a, guide=gview).cpu(), want)


@pytest.mark.parametrize('snap', [False, True])
def test_float_alpha_is_taken_as_its_unit_byte(snap):
    h, w, H, W = 64, 65, 131, 257
    frames, guides, a8 = scene(h, w, H, W)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    edge = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)), [np.nan, -0.5, 1.5, -0.0, np.inf, -np.inf]]).astype(np.float32)
    x = (a8.astype(np.float32) / np.float32(255)).copy()
    x[0, 1].reshape(-1)[:edge.size] = edge
    assert np.isnan(x).any() and (x == -0.5).any() and (x == 1.5).any() and np.isinf(x).any()
    want_bytes = np.stack([C.alpha_byte(p) for p in x[0]])[None]
    want = R.refine_all(frames, guides, want_bytes, snap=snap)
    got = refine.refine(frames, dev(x), guide=guides, snap=snap)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(got, refine.refine(frames, dev(want_bytes), guide=guides, snap=snap))
    asf = refine.refine(frames, dev(x), guide=guides, snap=snap, as_float=True)
    assert asf.dtype == torch.float32 and tuple(asf.shape) == (1, 2, H, W)
    assert np.array_equal(asf.cpu().numpy(), want.astype(np.float32) / np.float32(255))
    assert np.array_equal((asf.cpu().numpy() * np.float32(255)).astype(np.uint8), want)          # what `cutout` makes of it: the same bytes


def test_snap_moves_only_the_neighbouring_bytes():
    G = np.full((1, 1, 8, 3), 50, np.uint8)
    p = np.array([[[[0, 1, 2, 128, 253, 254, 255, 1]]]], np.uint8)
    assert refine.refine(G, dev(p), radius=1, eps=1.0).cpu().numpy().tolist() == p.tolist()
    assert refine.refine(G, dev(p), radius=1, eps=1.0, snap=True).cpu().numpy().ravel().tolist() == [0, 0, 2, 128, 253, 255, 255, 0]
    for v in (0, 255):
        frames, guides, _ = scene(64, 65, 131, 257)
        out = refine.refine(frames, torch.full((1, 1, 64, 65), v, dtype=torch.uint8, device='cuda'), guide=guides)
        assert bool((out == v).all())


def test_large_coefficients():
    G = np.full((8, 8, 3), 100, np.uint8)
    G[:, 4:, 0] = 101
    p = np.zeros((8, 8), np.uint8)
    p[:, 4:] = 255
    want, amax = R.refine(G, G, p, 3, 1e-6, with_max=True)
    assert amax > 128
    assert np.array_equal(refine.refine(G, dev(p[None]), radius=3, eps=1e-6).cpu().numpy()[0, 0], want)
    rs = np.random.RandomState(4)
    big = rs.randint(0, 256, (21, 19, 3)).astype(np.uint8)             # and applied to a frame that is not the guide
    want = R.refine(big, G, p, 3, 1e-6)
    assert np.array_equal(refine.refine(big, dev(p[None]), guide=G, radius=3, eps=1e-6).cpu().numpy()[0, 0], want)


def test_refine_replays_from_a_graph():
    """Resident inputs and tables, one chain of launches (the guide's resize, the byte conversion, six at low resolution, one at full size)."""
    plan = geometry.plan(270, 480, 144, 64)
    rs = np.random.RandomState(3)
    frames = dev(rs.randint(0, 256, size=(1, 270, 480, 3)).astype(np.uint8))
    x = dev(rs.random_sample((1, 2, 192, 256)).astype(np.float32))
    eager = refine.refine(frames, x, transform_info=plan.transform_info, snap=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = refine.refine(frames, x, transform_info=plan.transform_info, snap=True)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x2 = dev(rs.random_sample((1, 2, 192, 256)).astype(np.float32))
    want = refine.refine(frames, x2, transform_info=plan.transform_info, snap=True)
    x.copy_(x2)                                                         # a replay reads what its input holds now
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_c_entries_refuse_bad_arguments_before_any_launch():
    L = hip.lib()
    Ptr, I, Lg, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    h, w, H, W = 5, 7, 11, 13
    frames, guides, alpha = scene(h, w, H, W)
    f, g, a = dev(frames), dev(guides), dev(alpha)
    xi, xf, yi, yf = refine._tables(h, w, H, W, f.device)
    u32 = torch.zeros((4, 9, h, w), dtype=torch.int32, device='cuda')           # grows, gsums, prows, coef (the last two use 2 x 4 planes)
    wide = torch.zeros((2, 2, 4, h, w), dtype=torch.float64, device='cuda')
    out = torch.zeros((2, H, W), dtype=torch.uint8, device='cuda')
    outf = torch.zeros((2, H, W), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()

    def coef(gd=g.data_ptr(), al=a.data_ptr(), T=1, n=2, hh=h, ww=w, r=5, eps=1e-4, s0=u32[0].data_ptr(), s1=u32[1].data_ptr(), s2=u32[2].data_ptr(),
             s3=u32[3].data_ptr(), s4=wide[0].data_ptr(), s5=wide[1].data_ptr()):
        return L.mg_refine_coefficients(Ptr(gd), Ptr(al), Lg(T), I(n), I(hh), I(ww), I(r), D(eps), Ptr(s0), Ptr(s1), Ptr(s2), Ptr(s3), Ptr(s4), Ptr(s5),
                                        Ptr(None))

    def app(fr=f.data_ptr(), mn=wide[1].data_ptr(), T=1, n=2, hh=h, ww=w, HH=H, WW=W, a0=xi.data_ptr(), a1=xf.data_ptr(), a2=yi.data_ptr(),
            a3=yf.data_ptr(), o=out.data_ptr(), of=outf.data_ptr()):
        return L.mg_refine_apply(Ptr(fr), Ptr(mn), Lg(T), I(n), I(hh), I(ww), I(HH), I(WW), Ptr(a0), Ptr(a1), Ptr(a2), Ptr(a3), I(0), Ptr(o), Ptr(of),
                                 Ptr(None))

    assert all(coef(**{k: None}) == -2 for k in ('gd', 'al', 's0', 's1', 's2', 's3', 's4', 's5'))
    assert coef(r=0) == -2 and coef(r=refine.MAX_RADIUS + 1) == -2 and coef(eps=9e-7) == -2 and coef(eps=1.5) == -2 and coef(eps=float('nan')) == -2
    assert coef(hh=0) == -2 and coef(ww=0) == -2 and coef(hh=refine.MAX_SIDE + 1) == -2 and coef(T=-1) == -2 and coef(n=-1) == -2
    assert coef(s0=u32[0].data_ptr() + 2) == -2 and coef(s3=u32[3].data_ptr() + 1) == -2 and coef(s4=wide[0].data_ptr() + 4) == -2
    assert coef(s5=wide[1].data_ptr() + 4) == -2
    assert all(app(**{k: None}) == -2 for k in ('fr', 'mn', 'a0', 'a1', 'a2', 'a3'))
    assert app(o=None, of=None) == -2 and app(hh=0) == -2 and app(WW=0) == -2 and app(HH=refine.MAX_SIDE + 1) == -2 and app(T=-1) == -2
    assert app(mn=wide[1].data_ptr() + 4) == -2 and app(a1=xf.data_ptr() + 4) == -2 and app(a2=yi.data_ptr() + 2) == -2
    assert app(of=outf.data_ptr() + 2) == -2
    assert coef(T=0) == 0 and coef(n=0) == 0 and app(T=0) == 0 and app(n=0) == 0          # nothing to do is not an error, and launches nothing
    torch.cuda.synchronize()
    assert not bool(u32.any()) and not bool(wide.any()) and not bool(out.any()) and not bool(outf.any())
    v = [ctypes.c_int() for _ in range(6)]
    assert L.mg_refine_limits(*[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v][3:5] == [refine.MAX_RADIUS, refine.MAX_SIDE] and v[5].value % 4 == 0
    assert L.mg_refine_limits(None, *[ctypes.byref(x) for x in v[1:]]) == -2
    assert coef() == 0 and app() == 0                                   # and the good call is good: the bytes of the statement
    torch.cuda.synchronize()
    want = R.refine_all(frames, guides, alpha)
    assert np.array_equal(out.cpu().numpy(), want[0])
    assert np.array_equal(outf.cpu().numpy(), want[0].astype(np.float32) / np.float32(255))


# ---- the wiring ---------------------------------------------------------------------------------------------------------------------------------------
def test_cutout_takes_the_refined_bytes():
    plan = geometry.plan(270, 480, 144, 64)
    rs = np.random.RandomState(21)
    frames = rs.randint(0, 256, size=(1, 270, 480, 3)).astype(np.uint8)
    x = dev(rs.random_sample((1, 2, 192, 256)).astype(np.float32))
    info = plan.transform_info
    for opts, kw in ((True, {}), ({'radius': 3, 'eps': 1e-3}, {'radius': 3, 'eps': 1e-3})):
        for snap in (False, True):
            fine = refine.refine(frames, x, transform_info=info, snap=snap, **kw)
            got = cutout.cutout(frames, x, transform_info=info, snap=snap, refine=opts)
            assert tuple(got.shape) == (1, 2, 270, 480, 4)
            assert torch.equal(got[..., 3], fine)
            assert torch.equal(got, cutout.cutout(frames, fine))
    plain = cutout.cutout(frames, x, transform_info=info, snap=True)
    assert torch.equal(plain, cutout.cutout(frames, x, transform_info=info, snap=True, refine=False))
    assert not torch.equal(plain, got)


def stub_model(batch):
    """A fixed smooth function of batch['mask'] with values in [0, 1] (the stub of tests/test_gpu_matteout.py)."""
    m = batch['mask'].float()
    s = torch.nn.functional.avg_pool2d(m.reshape((-1, 1) + tuple(m.shape[-2:])), 31, 1, 15, count_include_pad=True).reshape(m.shape)
    return {'refined_masks': torch.clamp(1.5 * s - 0.2, 0.0, 1.0)}


@pytest.mark.parametrize('post', [False, True])
def test_predict_image_with_the_refined_alpha_is_its_pieces(post):
    from maggie_amd.utils import postprocessing
    from maggie_amd.utils.preprocess import DevicePreprocessor
    rs = np.random.RandomState(12)
    frame = rs.randint(0, 256, size=(80, 112, 3)).astype(np.uint8)
    label = np.zeros((80, 112), np.uint8)
    label[10:60, 8:50], label[24:76, 60:104], label[0:6, 100:112] = 4, 9, 9
    r = matteout.predict_image(stub_model, frame, label, postprocess=post, cutouts=True, refine=True)
    assert sorted(r) == ['alpha', 'composites', 'cutouts']
    planes = matteout.label_planes(label)[1]
    batch, info = DevicePreprocessor().predict_item(dev(frame), planes)
    pred = stub_model(batch)['refined_masks']
    bytes_ = refine.refine(frame, pred.float(), transform_info=info, snap=True)
    alpha = refine.refine(frame, pred.float(), transform_info=info, snap=True, as_float=True)[0]
    assert np.array_equal(alpha.cpu().numpy(), bytes_[0].cpu().numpy().astype(np.float32) / np.float32(255))    # one IEEE division a byte
    if post:
        alpha = postprocessing.postprocess(alpha)
    assert r['alpha'].dtype == torch.float32 and tuple(r['alpha'].shape) == (2, 80, 112) and torch.equal(r['alpha'], alpha)
    assert torch.equal(r['composites'], matteout.composite(frame, alpha)[0])
    assert torch.equal(r['cutouts'], cutout.cutout(frame, alpha)[0])
    if not post:
        assert torch.equal(r['cutouts'], cutout.cutout(frame, bytes_)[0])              # (k / 255f) 255f truncates back to k
    opt = matteout.predict_image(stub_model, frame, label, postprocess=post, refine={'radius': 3, 'eps': 1e-3})
    want = refine.refine(frame, pred.float(), transform_info=info, snap=True, as_float=True, radius=3, eps=1e-3)[0]
    assert torch.equal(opt['alpha'], postprocessing.postprocess(want) if post else want)
    empty = matteout.predict_image(stub_model, frame, np.zeros((80, 112), np.uint8), cutouts=True, refine=True)
    assert tuple(empty['alpha'].shape) == (0, 80, 112) and tuple(empty['cutouts'].shape) == (0, 80, 112, 4)


@pytest.mark.parametrize('post', [False, True])
def test_predict_image_without_the_argument_is_unchanged(post):
    from maggie_amd.utils import postprocessing
    from maggie_amd.utils.preprocess import DevicePreprocessor
    rs = np.random.RandomState(12)
    frame = rs.randint(0, 256, size=(80, 112, 3)).astype(np.uint8)
    label = np.zeros((80, 112), np.uint8)
    label[10:60, 8:50], label[24:76, 60:104] = 4, 9
    r = matteout.predict_image(stub_model, frame, label, postprocess=post)
    assert sorted(r) == ['alpha', 'composites']
    off = matteout.predict_image(stub_model, frame, label, postprocess=post, refine=False)
    assert torch.equal(r['alpha'], off['alpha']) and torch.equal(r['composites'], off['composites'])
    batch, info = DevicePreprocessor().predict_item(dev(frame), matteout.label_planes(label)[1])
    pred = stub_model(batch)['refined_masks']
    if post:                                                            # the two forms of the code before `refine=` existed
        alpha = postprocessing.postprocess(postprocessing.reverse_transform_tensor(pred, info, snap=True)).reshape(2, 80, 112)
        comp = matteout.composite(frame, alpha)[0]
    else:
        comp, alpha = matteout.composite(frame, pred.float(), transform_info=info, snap=True, return_alpha=True)
        comp, alpha = comp[0], alpha[0]
    assert torch.equal(r['alpha'], alpha) and torch.equal(r['composites'], comp)
