"""Guidance-mask synthesis on the device (csrc/maskgen.hip, maggie_amd.utils.maskgen): bit-packed rectangular morphology, the fused 1/8
down / up resize, cut, statistics and drop-out, against the NumPy restatement (tests/maskgen_restatement.py) and the reference's own classes
(tests/golden/maskgen_pinned.npz). Integer work: every comparison is exact."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import groundtruth_restatement as G                                   # noqa: E402
import maskgen_restatement as M                                       # noqa: E402
from helpers import load_golden, unpack_bits                         # noqa: E402

pytestmark = pytest.mark.gpu

# 1 x 1, a strip, sizes on both sides of the 64-wide tile, the fixtures' odd size, the training crop
MORPH_SIZES = [(1, 1), (7, 300), (64, 64), (65, 129), (253, 331), (512, 512)]
K_PAIRS = [(29, 29), (2, 31), (1, 1), (4, 7), (30, 3), (31, 2)]           # (k_dilate, k_erode): even / odd mixes, the largest reach, the identity
RESIZE_SIZES = [(8, 8), (5, 5), (12, 20), (64, 64), (96, 160), (253, 331), (512, 512)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq(out, ref):
    return torch.equal(out.cpu(), torch.from_numpy(np.ascontiguousarray(ref)))


def _grey(seed, n, H, W):
    """Grey noise and soft ellipses cut by the border, alternating."""
    rng = np.random.default_rng(seed)
    noise = G.noise_planes(seed, n, H, W)
    for p in range(1, n, 2):
        noise[p] = G.soft_ellipse(rng, H, W, cy=rng.uniform(0, H), cx=rng.uniform(0, W))
    return noise


def _ref_morph(planes, table):
    return np.stack([M.binarize_morph(pl, *row) for pl, row in zip(planes, np.asarray(table).tolist())])


# ---- morphology ------------------------------------------------------------------------------------------------------------------------------------
def test_every_k_for_dilate_and_for_erode():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    H, W = 63, 65
    ks = list(range(1, 32))
    rng = np.random.default_rng(1)
    planes = G.noise_planes(11, 2 * len(ks), H, W)
    thresh = rng.uniform(0.1, 0.95, 2 * len(ks)) * 255                 # noise: any threshold leaves a busy binary image
    thresh[::7] = 230.0                                                # and some sparse ones, where a wide dilation is not all ones
    table = MG.morph_table(thresh, ks + ks, ks + ks, ['dilate'] * len(ks) + ['erode'] * len(ks), 2 * len(ks))
    out = MG.binarize_morph(_T(planes, dev), thresh, ks + ks, ks + ks, ['dilate'] * len(ks) + ['erode'] * len(ks))
    ref = _ref_morph(planes, table)
    for p in range(len(planes)):
        assert np.array_equal(out[p].cpu().numpy(), ref[p]), table[p].tolist()


@pytest.mark.parametrize('H,W', MORPH_SIZES)
def test_four_orders_with_mixed_kernel_sizes(H, W):
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    pairs = K_PAIRS[:2] if H * W > 100000 else K_PAIRS                  # the full-resolution case: the two largest reaches
    combos = [(kd, ke, o) for kd, ke in pairs for o in M.ORDERS]
    planes = _grey(H * 7 + W, len(combos), H, W)
    rng = np.random.default_rng(H + W)
    thresh = rng.uniform(0.1, 0.95, len(combos)) * 255
    kd, ke, orders = [c[0] for c in combos], [c[1] for c in combos], [c[2] for c in combos]
    out = MG.binarize_morph(_T(planes, dev), thresh, kd, ke, orders).cpu().numpy()
    ref = _ref_morph(planes, MG.morph_table(thresh, kd, ke, orders, len(combos)))
    for p, c in enumerate(combos):
        assert np.array_equal(out[p], ref[p]), c
    assert set(np.unique(out)) <= {0, 255}


def test_threshold_is_floor_of_the_float_and_strict():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 16, 16).repeat(4, 0)
    out = MG.binarize_morph(_T(ramp, dev), [100.0, 100.99, 0.0, 254.5], 1, 1, 'dilate').cpu().numpy()
    assert [int((o > 0).sum()) for o in out] == [155, 155, 255, 1]
    assert np.array_equal(out, _ref_morph(ramp, [[100, 1, 1, 2], [100, 1, 1, 2], [0, 1, 1, 2], [254, 1, 1, 2]]))


def test_per_plane_parameters_equal_separate_calls():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    planes = _T(_grey(31, 6, 70, 131), dev)
    thresh, kd, ke = [40.5, 200.0, 127.0, 90.2, 25.5, 240.0], [3, 29, 8, 1, 16, 31], [31, 2, 8, 5, 1, 30]
    orders = ['dilate_erode', 'erode_dilate', 'dilate', 'erode', 'erode_dilate', 'dilate_erode']
    whole = MG.binarize_morph(planes, thresh, kd, ke, orders)
    for p in range(6):
        assert torch.equal(whole[p], MG.binarize_morph(planes[p], thresh[p], kd[p], ke[p], orders[p]))
    assert _eq(whole, _ref_morph(planes.cpu().numpy(), MG.morph_table(thresh, kd, ke, orders, 6)))


def test_more_planes_than_a_grid_dimension():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    P = 65536
    rng = np.random.default_rng(2)
    planes = rng.integers(0, 256, (P, 1, 1), dtype=np.uint8)
    thresh = rng.integers(0, 255, P).astype(np.float64) + 0.5
    kd, ke, orders = rng.integers(1, 32, P).tolist(), rng.integers(1, 32, P).tolist(), rng.integers(0, 4, P).tolist()
    out = MG.binarize_morph(_T(planes, dev), thresh, kd, ke, orders)
    # a 1 x 1 plane: every window holds the one pixel, whatever the operator
    assert _eq(out, ((planes[:, 0, 0] > np.floor(thresh)) * 255).astype(np.uint8).reshape(P, 1, 1))


# ---- down / up -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', RESIZE_SIZES)
def test_down_up_matches_the_restatement(H, W):
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    noise = G.noise_planes(H + 3 * W, 2, H, W)
    mask = M.noisy_ellipse(H * 31 + W, H, W)
    planes = np.stack([noise[0], mask, np.full((H, W), 127, np.uint8), np.full((H, W), 128, np.uint8), noise[1], mask])
    apply = [1, 1, 1, 1, 0, 0]
    out = MG.down_up(_T(planes, dev), apply)
    ref = np.stack([M.downup(pl) if a else pl for pl, a in zip(planes, apply)])
    assert _eq(out, ref)
    assert int(out[2].max()) == 0 and int(out[3].min()) == 255            # constant planes come back as they are: 127 is not > 127, 128 is
    assert _eq(MG.down_up(_T(planes, dev)), np.stack([M.downup(pl) for pl in planes]))
    assert _eq(MG.down_up(_T(planes, dev), False), planes)


# ---- cut -------------------------------------------------------------------------------------------------------------------------------------------
def test_cut_copies_and_swaps():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    H, W = 70, 90
    planes = G.noise_planes(41, 6, H, W)
    rects = np.full((6, 8), 0, np.int32)
    rects[:, 0] = -1
    rects[0] = (0, 10, 12, 14, 20, 17, 22, 0)                              # internal, source and destination overlap
    rects[1] = (1, H - 9, W - 11, 0, 0, 9, 11, 0)                          # destination in the bottom-right corner, source in the top-left
    rects[2] = (4, 30, 5, 30, 5, 20, 70, 0)                                # external: planes 2 and 4 swap the same rectangle
    rects[4] = (2, 30, 5, 30, 5, 20, 70, 0)
    rects[5] = (5, 3, 3, 8, 8, 0, 7, 0)                                    # an empty rectangle (randint(h // 8, h // 4) may draw 0 on small planes)
    ref = M.cut(planes, rects)
    out = MG.cut(_T(planes, dev), rects)
    assert _eq(out, ref)
    assert _eq(out[3], planes[3]) and _eq(out[5], planes[5]) and not _eq(out[0], planes[0])
    assert np.array_equal(ref[2, 30:50, 5:75], planes[4, 30:50, 5:75]) and np.array_equal(ref[4, 30:50, 5:75], planes[2, 30:50, 5:75])
    assert _eq(MG.cut(_T(planes, dev), _T(rects, dev)), ref)               # the table already on the device


# ---- statistics and drop-out -----------------------------------------------------------------------------------------------------------------------
def test_stats_and_drop():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    H, W = 96, 160
    blobs = ((G.soft_planes(51, 2, H, W) > 127) * 255).astype(np.uint8)
    single = np.zeros((H, W), np.uint8)
    single[37, 101] = 9                                                  # `> 0`, not `== 255`
    noise = ((G.noise_planes(52, 1, H, W)[0] > 250) * 255).astype(np.uint8)
    planes = np.stack([np.zeros((H, W), np.uint8), single, blobs[0], blobs[1], noise])
    st = MG.stats(_T(planes, dev))
    ref_st = M.stats(planes)
    assert st.dtype == torch.int32 and _eq(st, ref_st)
    assert ref_st[0].tolist() == [0, W, -1, H, -1] and ref_st[1].tolist() == [1, 101, 101, 37, 37]
    counts = ref_st[:, 0].tolist()
    for sel in ([[2, 0, 5, 9], [3, counts[3] - 1, 4, 6], [1, 0, 1, 1], [-1, 0, 0, 0]],
                [[4, counts[4] // 2, 7, 3], [2, counts[2] - 1, 11, 13], [3, 0, 2, 30], [-5, 0, 0, 0]],
                [[2, counts[2], 5, 5], [0, 0, 3, 3]]):                   # idx past the count; an empty plane: nothing to anchor to
        sel = np.asarray(sel, np.int32)
        live = np.asarray([e for e in sel.tolist() if e[0] >= 0 and e[1] < counts[e[0]]], np.int32).reshape(-1, 4)
        ref = M.drop(planes, live, ref_st)
        out = MG.drop(_T(planes, dev), sel, st)
        assert _eq(out, ref)
        assert len(live) == 0 or not np.array_equal(ref, planes)
    x = _T(planes, dev)
    assert MG.drop(x, np.asarray([[2, 0, 5, 9]], np.int32), ref_st, inplace=True).data_ptr() == x.data_ptr() and not _eq(x, planes)


# ---- the whole chain -------------------------------------------------------------------------------------------------------------------------------
def _case_draws(name):
    from maggie_amd.utils import maskgen as MG
    c = M.GOLDEN[name]
    rs = np.random.RandomState(c['rs_seed'])
    return MG.draw_chain(rs, random.Random(c['py_seed']), c['n'], c['H'], c['W'], c['max_k'], c['p'], dropout=c['video'], from_alpha=c['video']), rs


@pytest.mark.parametrize('name', sorted(M.GOLDEN))
def test_synthesize_matches_the_reference_fixture(name):
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    g = load_golden('maskgen_pinned.npz')
    pinned = unpack_bits(g[name], tuple(g[name + '.shape'])) * np.uint8(255)
    planes = M.golden_inputs(name)
    draws, rs = _case_draws(name)
    state = rs.get_state()
    out = MG.synthesize(_T(planes, dev), draws, rs)
    assert out.dtype == torch.uint8 and _eq(out, pinned)
    rs.set_state(state)
    assert _eq(MG.synthesize(planes.reshape(1, *planes.shape), draws.to(dev), rs)[0], pinned)       # host planes, device-resident draws, (1, P, H, W)


def test_from_alpha_matches_the_restatement():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    for seed, shape in ((61, (3, 96, 160)), (62, (2, 2, 37, 51))):
        a = G.soft_planes(seed, int(np.prod(shape[:-2])), *shape[-2:]).reshape(shape)
        flat = a.reshape(-1, *shape[-2:])
        assert _eq(MG.from_alpha(_T(a, dev)), M.from_alpha(flat).reshape(shape))
        assert _eq(MG.from_alpha(_T(a, dev), down_up=False), ((a > 127) * 255).astype(np.uint8))


def test_preprocessor_changes_only_the_mask():
    from maggie_amd.utils import maskgen as MG
    from maggie_amd.utils.preprocess import DevicePreprocessor
    dev = _dev()
    rng = np.random.default_rng(3)
    H, W = 128, 192
    pp = DevicePreprocessor(max_inst=10, device=dev)
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    alphas = G.soft_planes(4, 3, H, W)[None]
    ids = [6, 1, 8]
    draws = MG.draw_chain(np.random.RandomState(5), random.Random(5), 3, H, W)
    base = pp(frames, alphas, alphas, slot_ids=ids, transition=(4, 9))
    got = pp(frames, alphas, alphas, slot_ids=ids, transition=(4, 9), mask_draws=draws)
    assert set(got) == set(base) == {'image', 'alpha', 'mask', 'transition'}
    assert all(torch.equal(got[key], base[key]) for key in base if key != 'mask')
    restated = M.chain(alphas[0], draws)[None]
    assert torch.equal(got['mask'], pp(frames, alphas, restated, slot_ids=ids)['mask'])           # the existing nearest down-scale of the restated chain
    assert got['mask'].shape == (1, 10, H // 8, W // 8) and not torch.equal(got['mask'], base['mask'])
    # a clip with the drop-out: (MaskDraws, RandomState)
    T = 3
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    clip = G.clip_planes(6, T, 2, H, W)
    rs = np.random.RandomState(0)                                                         # a seed whose drop-out zeroes two rectangles
    draws = MG.draw_chain(rs, random.Random(0), T * 2, H, W, dropout=True, from_alpha=True)
    ref_rs = np.random.RandomState(0)
    ref_rs.set_state(rs.get_state())
    got = pp(frames, clip, clip, slot_ids=[3, 9], mask_draws=(draws, rs))
    m = M.chain(clip.reshape(T * 2, H, W), draws)
    st = M.stats(m)
    sel = MG.draw_dropout(ref_rs, st)
    assert (sel[:, 0] >= 0).sum() == 2
    restated = M.drop(m, sel, st).reshape(T, 2, H, W)
    assert torch.equal(got['mask'], pp(frames, clip, restated, slot_ids=[3, 9])['mask'])
    assert rs.rand() == ref_rs.rand()


def test_device_mask_drives_a_training_step():
    """The shape / dtype contract with MaGGIe.forward_inputs: (b, n_f, max_inst, h / 8, w / 8) fp32 in {0, 1}."""
    from maggie_amd.network import build_model
    from maggie_amd.utils import config, synth
    from maggie_amd.utils import maskgen as MG
    from maggie_amd.utils.preprocess import scale_planes
    from helpers import reference_layout_state_dict, seed_all
    dev = _dev()
    model, _ = build_model(config.model_config('image'))
    model.load_state_dict(reference_layout_state_dict('image'))
    model.to(dev).train(True)
    batch = synth.synthetic_batch(1, 1, 2, 128, 128, seed=11, train=True, it=10000, max_inst=10)
    a8 = torch.round(batch['alpha'][0, :, :2] * 255).to(torch.uint8)                       # (1, 2, h, w): the real instances sit in slots 0, 1
    draws = MG.draw_chain(np.random.RandomState(2), random.Random(2), 2, 128, 128)
    mask = scale_planes(MG.synthesize(a8.to(dev), draws), 10, [0, 1], (16, 16), 0, dev)
    assert mask.shape == batch['mask'].shape[1:] and mask.dtype == batch['mask'].dtype
    assert set(torch.unique(mask).tolist()) <= {0.0, 1.0} and 0.01 <= float(mask[:, :2].mean()) <= 0.9
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    batch['mask'] = mask[None]
    seed_all(3)
    out, loss = model(batch)
    loss['total'].backward()
    assert np.isfinite(float(loss['total']))
    assert any(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in model.parameters())


def test_graph_capture_replays_with_new_planes_and_new_draws():
    from maggie_amd.utils import maskgen as MG
    dev = _dev()
    P, H, W = 4, 130, 170
    a1, a2 = G.soft_planes(71, P, H, W), _grey(72, P, H, W)
    d1 = MG.draw_chain(np.random.RandomState(12), random.Random(12), P, H, W)
    d2 = MG.draw_chain(np.random.RandomState(15), random.Random(15), P, H, W)
    assert not np.array_equal(d1.morph, d2.morph) and not np.array_equal(d1.cut, d2.cut)
    static, dd = _T(a1, dev), d1.to(dev)
    eager = MG.synthesize(static, dd)                                                      # warm-up off the capture: the resize tables are uploaded
    assert _eq(eager, M.chain(a1, d1))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = MG.synthesize(static, dd)
    for a in (a2, a1):
        static.copy_(_T(a, dev))
        g.replay()
        torch.cuda.synchronize()
        assert _eq(y, M.chain(a, d1))
    assert torch.equal(y, eager)
    # new draws between replays: written into the device tables
    dd.morph.copy_(torch.from_numpy(d2.morph))
    dd.downup.copy_(torch.from_numpy(d2.downup))
    dd.cut.copy_(torch.from_numpy(d2.cut))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(y, M.chain(a1, d2))
    del g
