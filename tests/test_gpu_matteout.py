"""The device matte output (maggie_amd.utils.matteout, csrc/matteout.hip) against the NumPy restatement of tests/matteout_restatement.py, whose
overlay tests/test_matteout_cpu.py holds against Pillow and whose grid it shows to tell a contracted evaluation from the reference's. Every
comparison is exact equality, except where the alpha is compared with the existing reverse transform (2e-6, the bar of
test_postprocess_alpha_matches_reference_fixture_and_oracle)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jpegenc_restatement as JR                                      # noqa: E402
import matteout_restatement as R                                      # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import matteout, postprocessing                 # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor           # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
_GRID = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def grid_case():
    """(image, alpha, backgrounds, [restated composite per background]): computed once, never modified."""
    if not _GRID:
        image, alpha = R.grid()
        bgs = R.backgrounds(image.shape)
        _GRID['v'] = (image, alpha, bgs, [R.composite(image, alpha, b) for b in bgs])
    return _GRID['v']


# ---- 1. the discriminating grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(4))
def test_grid_exact(k):
    image, alpha, bgs, wants = grid_case()
    got = matteout.composite(image, dev(alpha)[None], bgs[k])
    assert got.shape == (1, 1) + image.shape and got.dtype == torch.uint8
    assert np.array_equal(got[0, 0].cpu().numpy(), wants[k])


# ---- 2. edge geometries, between guards ----------------------------------------------------------------------------------------------------
def raw_composite(frames, alpha, bg, off=0, aoff=0, snap=False, crop=None, out_hw=None):
    """mg_matte_composite itself: the frames, the background image and the output based `off` bytes behind a 16-byte boundary, the alpha and the
    returned alpha `aoff` bytes; the output and the returned alpha between guards of 0xA5, which must stay intact."""
    T, H, W, _ = frames.shape
    TP, h, w = alpha.shape
    P = TP // T
    crop = (h, w) if crop is None else crop
    assert out_hw is None or out_hw == (H, W)

    def based(x, o):
        buf = torch.zeros((x.nbytes + 32,), dtype=torch.uint8, device='cuda')
        v = buf[o:o + x.nbytes]
        v.copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8)))
        assert v.data_ptr() % 16 == o % 16
        return v

    def guarded(nbytes, o):
        buf = torch.full((2 * GUARD + nbytes + 32,), 0xA5, dtype=torch.uint8, device='cuda')
        assert buf.data_ptr() % 16 == 0
        return buf[GUARD + o:GUARD + o + nbytes], (buf[:GUARD + o], buf[GUARD + o + nbytes:])

    f, a = based(frames, off), based(alpha, aoff)
    image = None if np.ndim(bg) == 1 else based(bg, off)
    out, g1 = guarded(T * P * H * W * 3, off)
    aout, g2 = guarded(T * P * H * W * 4, aoff)
    r, g, b = (int(v) for v in bg) if image is None else (0, 0, 0)
    fn = hip.lib().mg_matte_composite
    fn.restype = ctypes.c_int
    rc = fn(hip.ptr(a), ctypes.c_long(T), P, h, w, crop[0], crop[1], H, W, int(snap), hip.ptr(f), hip.ptr(image),
            ctypes.c_long(0 if image is None else (bg.shape[0] if bg.ndim == 4 else 1)), r, g, b, hip.ptr(out), hip.ptr(aout), hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    for gd in g1 + g2:
        assert bool((gd == 0xA5).all()), 'a guard byte was overwritten'
    return out.cpu().numpy().reshape(T, P, H, W, 3), aout.cpu().numpy().view(np.float32).reshape(T, P, H, W)


SIZES = [(1, 1), (1, 17), (17, 1), (2, 3), (5, 16), (7, 21), (16, 16), (33, 65)]


@pytest.mark.parametrize('H,W', SIZES)
def test_edge_geometries(H, W):
    rs = np.random.RandomState(100 * H + W)
    for T in (1, 3):
        frames = rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)
        for P in (1, 3, 10):
            alpha = rs.random_sample((T, P, H, W)).astype(np.float32)
            alpha[rs.random_sample(alpha.shape) < 0.2] = rs.choice([0.0, 1.0])
            for bg in ((0, 255, 0), rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8), rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)):
                tag = (T, P, np.shape(bg))
                want = R.composites(frames, alpha, bg)
                got, aout = raw_composite(frames, alpha.reshape(T * P, H, W), bg)
                assert np.array_equal(got, want), tag
                assert np.array_equal(aout.view(np.uint32), alpha.view(np.uint32)), tag
                api = matteout.composite(frames if T > 1 else frames[0], dev(alpha), bg)
                assert np.array_equal(api.cpu().numpy(), want), tag
    assert any((h * w * 3) % 16 for h, w in SIZES) and any((h * w * 3) % 16 == 0 for h, w in SIZES)


@pytest.mark.parametrize('H,W', [(7, 21), (33, 65), (16, 16)])
def test_bases_at_byte_offsets(H, W):
    """The frame, the background image and the output one byte behind a 16-byte boundary, the alpha and the returned alpha four bytes: every
    wide access of the kernel runs unaligned."""
    rs = np.random.RandomState(H)
    T, P = 2, 3
    frames = rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)
    alpha = rs.random_sample((T, P, H, W)).astype(np.float32)
    for bg in ((17, 99, 203), rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)):
        got, aout = raw_composite(frames, alpha.reshape(T * P, H, W), bg, off=1, aoff=4)
        assert np.array_equal(got, R.composites(frames, alpha, bg))
        assert np.array_equal(aout, alpha)


def test_c_entry_argument_errors():
    fn = hip.lib().mg_matte_composite
    fn.restype = ctypes.c_int
    x = torch.zeros((64,), dtype=torch.uint8, device='cuda')
    a = torch.zeros((16,), dtype=torch.float32, device='cuda')
    L = ctypes.c_long
    ok = [hip.ptr(a), L(1), 1, 2, 2, 2, 2, 2, 2, 0, hip.ptr(x), None, L(0), 0, 255, 0, hip.ptr(x), None, hip.stream()]
    for pos, bad in ((0, None), (10, None), (16, None), (5, 3), (6, 0), (3, 0), (8, 0), (14, 256), (12, L(2))):
        args = list(ok)
        args[pos] = bad
        if pos == 12:
            args[11] = hip.ptr(x)
        assert fn(*args) == -2, pos
    assert fn(*(ok[:1] + [L(70000)] + ok[2:])) == -3
    ov = hip.lib().mg_matte_overlay
    ov.restype = ctypes.c_int
    assert ov(hip.ptr(x), hip.ptr(x), L(1), 2, 2, 255, 0, 255, ctypes.c_float(1.5), hip.ptr(x), hip.stream()) == -2
    assert ov(hip.ptr(x), None, L(1), 2, 2, 255, 0, 255, ctypes.c_float(0.5), hip.ptr(x), hip.stream()) == -2
    ids = hip.lib().mg_matte_label_ids
    ids.restype = ctypes.c_int
    assert ids(hip.ptr(x), 2, L(4), hip.ptr(a), hip.stream()) == -2
    pl = hip.lib().mg_matte_label_planes
    pl.restype = ctypes.c_int
    assert pl(hip.ptr(x), 1, L(4), None, 1, hip.ptr(x), hip.stream()) == -2
    assert pl(hip.ptr(x), 1, L(4), (ctypes.c_uint8 * 1)(1), 257, hip.ptr(x), hip.stream()) == -2
    torch.cuda.synchronize()


# ---- 3. the fused reverse transform --------------------------------------------------------------------------------------------------------
def _crop_of(info, h, w):
    for tr in info or []:
        if tr['name'] == 'padding' or tr['name'] == ['padding']:
            h, w = h - int(tr['pad_size'][0]), w - int(tr['pad_size'][1])
    return h, w


def _fused_cases():
    gold = load_golden('postprocess_pinned.npz')
    rs = np.random.RandomState(21)                                  # the draws of test_postprocess_alpha_matches_reference_fixture_and_oracle
    pinned = {'resize_pad': ((2, 3, 40, 56), [{'name': ['resize'], 'ori_size': (torch.tensor(37), torch.tensor(61))},
                                              {'name': ['padding'], 'pad_size': (torch.tensor(5), torch.tensor(8))}]),
              'pad_resize_same': ((1, 2, 32, 48), [{'name': 'resize', 'ori_size': (29, 48)}, {'name': 'padding', 'pad_size': (3, 0)}]),
              'resize_only': ((3, 24, 24), [{'name': 'resize', 'ori_size': (50, 33)}])}
    cases = []
    for key, (shape, info) in pinned.items():
        cases.append((key, rs.uniform(-0.05, 1.05, size=shape).astype(np.float32), info, gold[key]))
    rs = np.random.RandomState(22)
    more = {'down': ((2, 2, 40, 56), [{'name': 'resize', 'ori_size': (9, 13)}]),
            'one_row': ((1, 2, 8, 8), [{'name': 'resize', 'ori_size': (1, 5)}, {'name': 'padding', 'pad_size': (2, 1)}]),
            'one_column': ((1, 2, 8, 8), [{'name': 'resize', 'ori_size': (5, 1)}]),
            'padding_only': ((2, 16, 24), [{'name': 'padding', 'pad_size': (3, 5)}]),
            'no_transform': ((2, 7, 21), None)}
    for key, (shape, info) in more.items():
        cases.append((key, rs.uniform(-0.05, 1.05, size=shape).astype(np.float32), info, None))
    return cases


@pytest.mark.parametrize('fused', [True, None], ids=['one_launch', 'default'])
@pytest.mark.parametrize('case', _fused_cases(), ids=lambda c: c[0])
def test_fused_reverse_transform(case, fused):
    """`fused=True` is the single launch from the network-size alpha; the default form puts `reverse_transform_tensor` in front wherever a resize
    is undone (it measured faster: DESIGN.md section 29). Both meet the same checks."""
    key, x, info, gold = case
    xd = dev(x)
    if gold is None:
        gold = (postprocessing.reverse_transform_tensor(xd, info) if info else xd).cpu().numpy()
    P, h, w = x.shape[-3:]
    T = x.size // (P * h * w)
    H, W = gold.shape[-2:]
    frames = np.random.RandomState(5).randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)
    bg = (17, 99, 203)
    # (a) without snapping: the alpha of the existing reverse transform (the fixture, where there is one)
    comp, a = matteout.composite(frames, xd, bg, transform_info=info, return_alpha=True, fused=fused)
    a_np = a.cpu().numpy()
    assert a_np.shape == (T, P, H, W) and comp.shape == (T, P, H, W, 3)
    err = float(np.abs(a_np - gold.reshape(T, P, H, W)).max())
    print('%s: max |alpha - reference| %.3g' % (key, err))
    assert err <= 2e-6, key
    # (c) the bytes are the restatement's for the alpha that was returned
    assert np.array_equal(comp.cpu().numpy(), R.composites(frames, a_np, bg)), key
    # (b) with snapping
    comp_s, a_s = matteout.composite(frames, xd, bg, transform_info=info, snap=True, return_alpha=True, fused=fused)
    s_np, g = a_s.cpu().numpy(), gold.reshape(T, P, H, W)
    flip = (np.abs(g - 1 / 255.0) < 1e-5) | (np.abs(g - 254 / 255.0) < 1e-5)           # knife-edge values may snap either way
    assert np.abs(s_np - R.snap(g))[~flip].max() <= 2e-6, key
    assert not ((s_np != 0.0) & (s_np <= 1.0 / 255.0)).any() and not ((s_np != 1.0) & (s_np >= 254.0 / 255.0)).any(), key
    assert np.array_equal(s_np, R.snap(a_np)), key                                      # the same value, then the snapping
    assert np.array_equal(comp_s.cpu().numpy(), R.composites(frames, s_np, bg)), key
    # (d) nothing beyond the crop is read
    ch, cw = _crop_of(info, h, w)
    if (ch, cw) != (h, w):
        poisoned = x.copy()
        poisoned[..., ch:, :] = np.nan
        poisoned[..., :, cw:] = np.nan
        again = matteout.composite(frames, dev(poisoned), bg, transform_info=info, snap=True, fused=fused)
        assert torch.equal(again, comp_s), key
    # (e) size == crop: the alpha itself, bit for bit
    if (ch, cw) == (H, W):
        assert np.array_equal(a_np.view(np.uint32), np.ascontiguousarray(x.reshape(T, P, h, w)[..., :ch, :cw]).view(np.uint32)), key


def test_two_resizes_go_through_the_reverse_transform_first():
    rs = np.random.RandomState(9)
    x = dev(rs.random_sample((2, 12, 12)).astype(np.float32))
    info = [{'name': 'resize', 'ori_size': (7, 9)}, {'name': 'resize', 'ori_size': (10, 14)}, {'name': 'padding', 'pad_size': (2, 0)}]
    frame = rs.randint(0, 256, size=(7, 9, 3)).astype(np.uint8)
    comp, a = matteout.composite(frame, x, transform_info=info, snap=True, return_alpha=True)
    want = postprocessing.reverse_transform_tensor(x, info, snap=True)
    assert torch.equal(a[0], want)
    assert np.array_equal(comp.cpu().numpy(), R.composites(frame[None], a.cpu().numpy()))


# ---- 4. alphas outside [0, 1] --------------------------------------------------------------------------------------------------------------
def test_out_of_range_alpha_is_clamped_like_the_restatement():
    rs = np.random.RandomState(4)
    frames = rs.randint(0, 256, size=(2, 7, 21, 3)).astype(np.uint8)
    alpha = rs.uniform(-0.05, 1.05, size=(2, 2, 7, 21)).astype(np.float32)
    assert (alpha < 0).any() and (alpha > 1).any()
    for bg in ((0, 255, 0), (255, 255, 255)):
        assert np.array_equal(matteout.composite(frames, dev(alpha), bg).cpu().numpy(), R.composites(frames, alpha, bg))


# ---- 5. the overlay ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', [0.5, 0.3, 1.0 / 3.0, 0.0, 1.0])
def test_overlay_all_pairs(alpha):
    v = np.arange(256, dtype=np.uint8)
    image = np.broadcast_to(v[None, :, None], (256, 256, 3)).copy()
    mask = np.broadcast_to(np.array([0, 1, 255], np.uint8)[np.arange(256) % 3][:, None], (256, 256)).copy()
    image_d, mask_d = dev(image), dev(mask)
    for c in range(0, 256, 3):                                      # in2 = c, c + 1, c + 2 (and 0 where the mask is off) against every in1
        colour = (c, min(c + 1, 255), min(c + 2, 255))
        got = matteout.overlay(image_d, mask_d, colour, alpha)
        assert np.array_equal(got.cpu().numpy(), R.overlay(image, mask, colour, alpha)), (alpha, colour)


@pytest.mark.parametrize('H,W', [(1, 1), (5, 17), (33, 65)])
def test_overlay_geometries(H, W):
    rs = np.random.RandomState(H)
    frames = rs.randint(0, 256, size=(3, H, W, 3)).astype(np.uint8)
    masks = rs.choice(np.array([0, 1, 255], np.uint8), size=(3, H, W))
    for alpha in (0.5, 0.3):
        got = matteout.overlay(frames, masks, alpha=alpha)
        assert got.shape == frames.shape
        assert np.array_equal(got.cpu().numpy(), np.stack([R.overlay(f, m, (255, 0, 255), alpha) for f, m in zip(frames, masks)]))
    one = matteout.overlay(frames[0], masks[0])
    assert np.array_equal(one.cpu().numpy(), R.overlay(frames[0], masks[0]))


# ---- 6. label maps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(1, 1), (5, 17), (33, 65)])
@pytest.mark.parametrize('dtype', [np.uint8, np.int32])
def test_label_planes(H, W, dtype):
    rs = np.random.RandomState(W)
    m = rs.choice(np.array([0, 3, 7, 255]), size=(H, W), p=[0.4, 0.2, 0.2, 0.2]).astype(dtype)
    if H * W == 1:
        m[...] = 7
    else:
        m.reshape(-1)[:4] = [0, 3, 7, 255]                         # every id is there, whatever the draw
    ids, planes = matteout.label_planes(m)
    want_ids, want = R.label_planes(m)
    assert ids == want_ids and planes.dtype == torch.uint8 and np.array_equal(planes.cpu().numpy(), want)
    ids_d, planes_d = matteout.label_planes(dev(m))                # a device map
    assert ids_d == ids and torch.equal(planes_d, planes)


def test_label_planes_without_instances_and_out_of_range():
    ids, planes = matteout.label_planes(np.zeros((5, 17), np.uint8))
    assert ids == [] and tuple(planes.shape) == (0, 5, 17) and planes.dtype == torch.uint8
    m = np.zeros((5, 17), np.int32)
    m[4, 16] = 256
    with pytest.raises(ValueError):
        matteout.label_planes(m)
    m[4, 16] = -1
    with pytest.raises(ValueError):
        matteout.label_planes(m)
    every = np.arange(256, dtype=np.int32).reshape(16, 16)         # all 256 ids at once
    ids, planes = matteout.label_planes(every)
    assert ids == list(range(1, 256)) and np.array_equal(planes.cpu().numpy(), R.label_planes(every)[1])


# ---- 7. the files --------------------------------------------------------------------------------------------------------------------------
def test_save_composites_and_overlay_write_pillows_files(tmp_path):
    rs = np.random.RandomState(7)
    frame = rs.randint(0, 256, size=(17, 23, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:17, 0:23]
    alpha = np.stack([np.clip((xx - 4) / 12.0, 0, 1), np.clip(1.2 - np.hypot(yy - 8, xx - 11) / 7.0, 0, 1)]).astype(np.float32)
    comp = matteout.composite(frame, dev(alpha))[0]
    want = R.composites(frame[None], alpha[None])[0]
    paths = matteout.save_composites(comp, str(tmp_path / 'matte'), 'frame0007')
    assert paths == [str(tmp_path / 'matte' / ('%02d_frame0007.jpg' % i)) for i in range(2)]
    for p, w in zip(paths, want):
        with open(p, 'rb') as f:
            assert f.read() == JR.file_bytes(w, 75), p
    mask = (alpha[1] > 0.3).astype(np.uint8)
    ov = matteout.overlay(frame, mask)
    paths = matteout.save_overlay(ov, str(tmp_path / 'vis'), '00001_video0')
    assert paths == [str(tmp_path / 'vis' / '00001_video0.jpg')]
    with open(paths[0], 'rb') as f:
        assert f.read() == JR.file_bytes(R.overlay(frame, mask), 75)


# ---- 8. predict_image ----------------------------------------------------------------------------------------------------------------------
def stub_model(batch):
    """A fixed smooth function of batch['mask'] with values in [0, 1]."""
    m = batch['mask'].float()
    s = torch.nn.functional.avg_pool2d(m.reshape((-1, 1) + tuple(m.shape[-2:])), 31, 1, 15, count_include_pad=True).reshape(m.shape)
    return {'refined_masks': torch.clamp(1.5 * s - 0.2, 0.0, 1.0)}


@pytest.mark.parametrize('post', [False, True])
def test_predict_image_is_the_chain_of_its_pieces(post):
    rs = np.random.RandomState(12)
    frame = rs.randint(0, 256, size=(40, 56, 3)).astype(np.uint8)
    label = np.zeros((40, 56), np.uint8)
    label[5:30, 4:25], label[12:38, 30:52], label[0:3, 50:56] = 4, 9, 9
    planes = R.label_planes(label)[1]
    pre = DevicePreprocessor()
    batch, info = pre.predict_item(frame, planes)
    pred = stub_model(batch)['refined_masks']
    assert float(pred.min()) >= 0.0 and float(pred.max()) <= 1.0 and tuple(pred.shape[:3]) == (1, 1, 2)
    if post:
        alpha = postprocessing.postprocess(postprocessing.reverse_transform_tensor(pred, info, snap=True)).reshape(2, 40, 56)
    else:
        alpha = matteout.composite(frame, pred, transform_info=info, snap=True, return_alpha=True)[1][0]
    want = R.composites(frame[None], alpha.cpu().numpy()[None])[0]
    for instances in (label, planes, dev(planes)):
        r = matteout.predict_image(stub_model, frame, instances, postprocess=post)
        assert tuple(r['alpha'].shape) == (2, 40, 56) and tuple(r['composites'].shape) == (2, 40, 56, 3)
        assert torch.equal(r['alpha'], alpha)
        assert np.array_equal(r['composites'].cpu().numpy(), want)
    assert float(alpha.max()) == 1.0 and float(alpha.min()) == 0.0                  # the snapping took place
    empty = matteout.predict_image(stub_model, frame, np.zeros((40, 56), np.uint8))
    assert tuple(empty['alpha'].shape) == (0, 40, 56) and tuple(empty['composites'].shape) == (0, 40, 56, 3)


# ---- 9. the video writer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clips', [1, 2, 4])
def test_video_matte_writer(clips, tmp_path):
    rs = np.random.RandomState(clips)
    H, W, n = 8, 12, 2
    info = [{'name': 'resize', 'ori_size': (H, W)}, {'name': 'padding', 'pad_size': (0, 8)}]
    frames = rs.randint(0, 256, size=(clips + 2, H, W, 3)).astype(np.uint8)
    names = ['video0/%05d.jpg' % k for k in range(clips + 2)]
    out_dir = str(tmp_path / 'matte')
    writer = matteout.VideoMatteWriter(out_dir)
    pushes, got = [], []
    for c in range(clips):
        clip = dev(rs.random_sample((1, 3, n, 16, 32)).astype(np.float32) ** 2)
        first, last = c == 0, c == clips - 1
        alpha = postprocessing.postprocess(postprocessing.reverse_transform_tensor(clip, info, snap=True))[0].cpu().numpy()
        pushes.append((alpha, frames[c:c + 3], names[c:c + 3], first, last))
        paths = writer.push(clip, info, frames[c:c + 3], [[nm] for nm in names[c:c + 3]], first, last)      # the loader's one-element lists
        got.append([(p, open(p, 'rb').read()) for p in paths])
    want = R.writer_loop(pushes, out_dir)
    assert len(want[-1]) == n * (3 if clips == 1 else 4)
    for c in range(clips):
        assert [p for p, _ in got[c]] == [p for p, _ in want[c]], c
        for (p, data), (_, comp) in zip(got[c], want[c]):
            assert data == JR.file_bytes(comp, 75), (c, p)


# ---- 10. graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, None], ids=['one_launch', 'default'])
def test_composite_replays_from_a_graph(fused):
    """One kernel, or two behind one another: no parallel branches either way."""
    rs = np.random.RandomState(3)
    frames = dev(rs.randint(0, 256, size=(2, 37, 61, 3)).astype(np.uint8))
    x = dev(rs.random_sample((2, 3, 40, 56)).astype(np.float32))
    info = [{'name': 'resize', 'ori_size': (37, 61)}, {'name': 'padding', 'pad_size': (5, 8)}]
    eager, eager_a = matteout.composite(frames, x, transform_info=info, snap=True, return_alpha=True, fused=fused)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, a = matteout.composite(frames, x, transform_info=info, snap=True, return_alpha=True, fused=fused)
    out.zero_()
    a.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(a, eager_a)
    x2 = dev(rs.random_sample((2, 3, 40, 56)).astype(np.float32))
    want = matteout.composite(frames, x2, transform_info=info, snap=True, fused=fused)
    x.copy_(x2)                                                     # a replay reads what its input holds now
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
