"""Ground-truth maps on the device (csrc/morph.hip, maggie_amd.utils.groundtruth): grey-scale ellipse dilation / erosion, the training
transition maps (image and video rule) and the evaluation trimap, against the NumPy restatement (tests/groundtruth_restatement.py) and the
reference's own glue (tests/golden/groundtruth_pinned.npz). Integer work: every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import groundtruth_restatement as R                                   # noqa: E402
from helpers import load_golden, unpack_bits                         # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_K = [(k, n) for k in (2, 3, 4) for n in (1, 2, 5, 14)]
LARGE_K = [(5, 1), (11, 1), (25, 1), (31, 1)]
# 1 x 1, a strip, the fixture's odd size, the training crop, and sizes on both sides of the 64-wide tile
SIZES = [(1, 1), (7, 300), (253, 331), (512, 512), (63, 65), (64, 64), (65, 129), (128, 63)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _planes(seed, H, W):
    """(2, H, W): uniform noise with 0 / 255 planted in the corners, and a soft ellipse cut by the border with a 255 / 0 pair on the border."""
    rng = np.random.default_rng(seed)
    soft = R.soft_ellipse(rng, H, W, cy=0.1 * H, cx=0.9 * W)
    soft[0, 0], soft[-1, -1] = 255, 0
    return np.stack([R.noise_planes(seed, 1, H, W)[0], soft])


def _ref_morph(planes, k, n):
    return (np.stack([R.dilate(p, k, n) for p in planes]), np.stack([R.erode(p, k, n) for p in planes]))


@pytest.mark.parametrize('k,n', SMALL_K + LARGE_K)
def test_dilate_erode_match_the_restatement(k, n):
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    for si, (H, W) in enumerate(SIZES):
        planes = _planes(1000 + 37 * si + k, H, W)
        rd, re = _ref_morph(planes, k, n)
        x = _T(planes, dev)
        d, e = G.dilate(x, k, n), G.erode(x, k, n)
        assert d.dtype == torch.uint8 and d.shape == x.shape
        assert torch.equal(d.cpu(), torch.from_numpy(rd)), (k, n, H, W, 'dilate', int((d.cpu().numpy() != rd).sum()))
        assert torch.equal(e.cpu(), torch.from_numpy(re)), (k, n, H, W, 'erode', int((e.cpu().numpy() != re).sum()))
        d2, e2 = G.dilate_erode(x, k, n)
        assert torch.equal(d2, d) and torch.equal(e2, e)


@pytest.mark.parametrize('k,n', [(4, 14), (2, 5), (3, 2), (25, 1), (31, 1)])
def test_dilate_erode_on_a_full_resolution_plane(k, n):
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    planes = _planes(77 + k, 1080, 1927)[None]                        # (1, 2, H, W): the (F, n_i, H, W) layout, W odd
    rd, re = _ref_morph(planes[0], k, n)
    d, e = G.dilate_erode(_T(planes, dev), k, n)
    assert torch.equal(d[0].cpu(), torch.from_numpy(rd)) and torch.equal(e[0].cpu(), torch.from_numpy(re))


def test_more_planes_than_a_grid_dimension():
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 256, (70000, 3, 5), dtype=np.uint8)
    d = G.dilate(_T(planes, dev), 3, 2).cpu().numpy()
    for p in (0, 1, 65535, 65536, 69999):
        assert np.array_equal(d[p], R.dilate(planes[p], 3, 2)), p


def test_per_frame_tables_equal_separate_calls():
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    ks, ns = [2, 25, 4, 3, 1, 31], [5, 1, 14, 9, 3, 1]
    x = _T(np.stack([_planes(300 + f, 131, 197) for f in range(len(ks))]), dev)             # (6, 2, H, W)
    d, e = G.dilate_erode(x, ks, ns)
    for f, (k, n) in enumerate(zip(ks, ns)):
        d1, e1 = G.dilate_erode(x[f:f + 1], k, n)
        assert torch.equal(d[f:f + 1], d1) and torch.equal(e[f:f + 1], e1), (f, k, n)
        rd, re = _ref_morph(x[f].cpu().numpy(), k, n)
        assert torch.equal(d[f].cpu(), torch.from_numpy(rd)) and torch.equal(e[f].cpu(), torch.from_numpy(re)), (f, k, n)
    t = G.transition_gt(x, ks, ns, thresh=5)
    for f, (k, n) in enumerate(zip(ks, ns)):
        assert torch.equal(t[f:f + 1], G.transition_gt(x[f:f + 1], k, n, thresh=5)), (f, k, n)


def test_transition_train_rule_matches_restatement_and_fixture():
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    c = R.GOLDEN['train']
    raw = R.soft_planes(c['seed'], c['n'], c['H'], c['W'])[None]      # before the `< 5 -> 0` rule: the kernel applies it
    alpha, mask = R.golden_inputs('train')
    out = G.transition_gt(_T(raw, dev), c['k_size'], c['iterations'], thresh=5, n_slots=c['max_inst'], slot_ids=c['chosen_ids'])
    assert out.dtype == torch.float32 and out.shape == (1, c['max_inst'], c['H'], c['W'])
    g = load_golden('groundtruth_pinned.npz')
    pinned = unpack_bits(g['train'], tuple(g['train.shape'])).astype(np.float32)
    assert torch.equal(out.cpu(), torch.from_numpy(pinned))
    ref = R.him_train_item(alpha, mask, c['chosen_ids'], c['max_inst'], c['k_size'], c['iterations'])
    assert torch.equal(out.cpu(), ref)
    empty = [s for s in range(c['max_inst']) if s not in c['chosen_ids']]
    assert empty and not out[:, empty].any()
    assert 0.01 <= float(out[:, c['chosen_ids']].mean()) <= 0.5
    # every draw of the image loader (k in 2..4, 5..14 passes) at the training crop, 3 instances in 10 slots
    rng = np.random.default_rng(8)
    raw = R.soft_planes(9, 3, 512, 512)[None]
    for k, n in ((2, 5), (3, 14), (4, 14), (4, 5)):
        ids = [int(i) for i in rng.choice(10, 3, replace=False)]
        out = G.transition_gt(_T(raw, dev), k, n, thresh=5, n_slots=10, slot_ids=ids)
        assert torch.equal(out.cpu(), torch.from_numpy(R.transition_planes(R.threshold(raw), k, n, 10, ids))), (k, n)


def test_trimap_matches_restatement_and_fixture():
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    ori = R.golden_inputs('eval')
    tri = G.trimap(_T(ori, dev))
    assert tri.dtype == torch.float32 and tri.shape == ori.shape
    g = load_golden('groundtruth_pinned.npz')
    assert torch.equal(tri.cpu(), torch.from_numpy(g['eval'].astype(np.float32)))
    assert torch.equal(tri.cpu(), R.eval_item(ori))
    assert set(np.unique(tri.cpu().numpy())) == {0.0, 1.0, 2.0}
    # a clip at an odd full resolution, values 1..4 present (no `< 5` rule on ori_alphas) and 127 / 128 side by side
    ori = R.clip_planes(31, 2, 2, 407, 723)
    ori[:, :, 200, 100:110] = np.asarray([1, 2, 3, 4, 5, 126, 127, 128, 129, 255], np.uint8)
    tri = G.trimap(_T(ori, dev))
    assert torch.equal(tri.cpu(), torch.from_numpy(R.trimap_planes(ori)))


@pytest.mark.parametrize('T', [3, 8])
def test_diff_transition_matches_restatement(T):
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    raw = R.clip_planes(40 + T, T, 3, 253, 331)
    for k, n in ((2, 3), (3, 6), (4, 6)):
        out = G.diff_transition(_T(raw, dev), k, n, thresh=5, n_slots=10)
        assert out.dtype == torch.float32 and out.shape == (T, 10, 253, 331)
        assert bool((out[0] == 1).all())
        assert all(torch.equal(out[:, s], out[:, 0]) for s in range(10))
        ref = R.vim_train_item(R.threshold(raw), [7, 2, 5], 10, k, n)
        assert torch.equal(out.cpu(), ref), (k, n)
        assert torch.equal(out.cpu(), torch.from_numpy(R.diff_planes(R.threshold(raw), k, n, 10)))
        assert 0.001 < float(out[1:].mean()) < 0.5


def test_diff_transition_matches_fixture():
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    c = R.GOLDEN['diff']
    raw = R.clip_planes(c['seed'], c['T'], c['n'], c['H'], c['W'])
    out = G.diff_transition(_T(raw, dev), c['k_size'], c['iterations'], thresh=5, n_slots=c['max_inst'])
    g = load_golden('groundtruth_pinned.npz')
    pinned = unpack_bits(g['diff'], tuple(g['diff.shape'])).astype(np.float32)
    assert torch.equal(out.cpu(), torch.from_numpy(pinned))


def test_preprocessor_adds_exactly_one_key():
    from maggie_amd.utils.preprocess import DevicePreprocessor
    dev = _dev()
    rng = np.random.default_rng(3)
    H, W = 128, 192
    pp = DevicePreprocessor(max_inst=10, device=dev)
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    alphas = R.soft_planes(4, 3, H, W)[None]
    masks = ((alphas > 127) * 255).astype(np.uint8)
    ids = [6, 1, 8]
    base = pp(frames, alphas, masks, slot_ids=ids)
    assert set(base) == {'image', 'alpha', 'mask'}
    tr = pp(frames, alphas, masks, slot_ids=ids, transition=(4, 9))
    assert set(tr) == {'image', 'alpha', 'mask', 'transition'}
    assert all(torch.equal(tr[key], base[key]) for key in base)
    assert torch.equal(tr['transition'].cpu(), torch.from_numpy(R.transition_planes(R.threshold(alphas), 4, 9, 10, ids)))
    ev = DevicePreprocessor(max_inst=10, downscale_mask=False, device=dev)
    base = ev(frames, alphas, masks)
    tm = ev(frames, alphas, masks, trimap=True)
    assert set(tm) == {'image', 'alpha', 'mask', 'trimap'} and all(torch.equal(tm[key], base[key]) for key in base)
    assert torch.equal(tm['trimap'].cpu(), torch.from_numpy(R.trimap_planes(alphas)))
    # a clip: the video rule
    T = 4
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    clip = R.clip_planes(6, T, 2, H, W)
    masks = ((clip > 127) * 255).astype(np.uint8)
    base = pp(frames, clip, masks, slot_ids=[3, 9])
    tr = pp(frames, clip, masks, slot_ids=[3, 9], transition=(3, 4))
    assert set(tr) == {'image', 'alpha', 'mask', 'transition'} and all(torch.equal(tr[key], base[key]) for key in base)
    assert torch.equal(tr['transition'].cpu(), R.vim_train_item(R.threshold(clip), [3, 9], 10, 3, 4))


def test_device_transition_drives_a_training_step():
    """The shape / dtype contract with MaGGIe.forward_inputs: (b, n_f, max_inst, h, w) fp32 next to 'alpha'."""
    from maggie_amd.network import build_model
    from maggie_amd.utils import config, synth
    from maggie_amd.utils import groundtruth as G
    from helpers import reference_layout_state_dict, seed_all
    dev = _dev()
    model, _ = build_model(config.model_config('image'))
    model.load_state_dict(reference_layout_state_dict('image'))
    model.to(dev).train(True)
    batch = synth.synthetic_batch(1, 1, 2, 128, 128, seed=11, train=True, it=10000, max_inst=10)
    a8 = torch.round(batch['alpha'][0, :, :2] * 255).to(torch.uint8)                       # (1, 2, h, w): the real instances sit in slots 0, 1
    trans = G.transition_gt(a8.to(dev), 3, 7, thresh=5, n_slots=10, slot_ids=[0, 1])
    assert trans.shape == batch['transition'].shape[1:] and trans.dtype == batch['transition'].dtype
    assert 0.01 <= float(trans[:, :2].mean()) <= 0.5
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    batch['transition'] = trans[None]
    seed_all(3)
    out, loss = model(batch)
    loss['total'].backward()
    assert np.isfinite(float(loss['total']))
    assert any(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in model.parameters())


def test_graph_capture_replays_and_is_deterministic():
    from maggie_amd.utils import groundtruth as G
    dev = _dev()
    a1 = R.soft_planes(21, 3, 253, 331)[None]
    a2 = R.noise_planes(22, 3, 253, 331)[None]
    clip1, clip2 = R.clip_planes(23, 3, 2, 130, 170), R.clip_planes(24, 3, 2, 130, 170)
    static, sclip = _T(a1, dev), _T(clip1, dev)
    dr = G.draws(4, 7, 1)
    dd = G.draws(3, 5, 3)
    eager = [G.transition_gt(static, dr, thresh=5), G.trimap(static), G.diff_transition(sclip, dd, None)]
    again = [G.transition_gt(static, dr, thresh=5), G.trimap(static), G.diff_transition(sclip, dd, None)]
    assert all(torch.equal(x, y) for x, y in zip(eager, again))
    assert torch.equal(eager[0].cpu(), torch.from_numpy(R.transition_planes(R.threshold(a1), 4, 7)))
    tri_draws = G.draws(25, 1, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        G.transition_gt(static, tri_draws, _mode=G.MODE_TRIMAP)                               # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y_tr = G.transition_gt(static, dr, thresh=5)
        y_tri = G.transition_gt(static, tri_draws, _mode=G.MODE_TRIMAP)
        y_diff = G.diff_transition(sclip, dd, None)
    for a, clip in ((a2, clip2), (a1, clip1)):
        static.copy_(_T(a, dev))
        sclip.copy_(_T(clip, dev))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_tr.cpu(), torch.from_numpy(R.transition_planes(R.threshold(a), 4, 7)))
        assert torch.equal(y_tri.cpu(), torch.from_numpy(R.trimap_planes(a)))
        assert torch.equal(y_diff.cpu(), torch.from_numpy(R.diff_planes(R.threshold(clip), 3, 5)))
    assert torch.equal(y_tr, eager[0]) and torch.equal(y_tri, eager[1]) and torch.equal(y_diff, eager[2])
    # new draws between replays: written into the device table, within the bound it was made for
    dr.kn.copy_(torch.tensor([[2, 9]], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_tr.cpu(), torch.from_numpy(R.transition_planes(R.threshold(a1), 2, 9)))
    del g
