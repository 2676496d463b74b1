"""Host side of the guidance-mask chain (maggie_amd.utils.maskgen): the restated OpenCV operators against independent formulations, the
draws and the restated chain against the reference's own classes (tests/golden/maskgen_pinned.npz), the resize tables, the argument errors.
No GPU."""
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
from maggie_amd.utils import maskgen                                  # noqa: E402


def test_rect_filters_match_scipy_for_every_k():
    from scipy import ndimage
    plane = G.noise_planes(5, 1, 40, 53)[0]
    binary = (plane > 200).astype(np.uint8)                            # sparse enough that a 31-wide window is not all ones
    for k in range(1, 32):
        for src in (plane, binary):
            assert np.array_equal(M.rect_dilate(src, k), ndimage.maximum_filter(src, size=k, mode='constant', cval=0)), k
            assert np.array_equal(M.rect_erode(src, k), ndimage.minimum_filter(src, size=k, mode='constant', cval=255)), k


def _golden_case(name):
    """The case through the product's draws and the restated operators."""
    c = M.GOLDEN[name]
    planes = M.golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])
    draws = maskgen.draw_chain(rs, random.Random(c['py_seed']), c['n'], c['H'], c['W'], c['max_k'], c['p'], dropout=c['video'],
                               from_alpha=c['video'])
    if not c['video']:
        return M.chain(planes, draws)
    m = M.chain(planes, draws)
    st = M.stats(m)
    return M.drop(m, maskgen.draw_dropout(rs, st), st)


@pytest.mark.parametrize('name', sorted(M.GOLDEN))
def test_draws_and_restatement_match_the_reference_fixture(name):
    g = load_golden('maskgen_pinned.npz')
    pinned = unpack_bits(g[name], tuple(g[name + '.shape'])) * np.uint8(255)
    assert np.array_equal(_golden_case(name), pinned)


def test_fixture_cases_cover_every_branch():
    """What the generator asserted when the fixture was made, from the draws alone."""
    orders, flags, cuts, drops = set(), set(), set(), set()
    for name, c in M.GOLDEN.items():
        rs = np.random.RandomState(c['rs_seed'])
        d = maskgen.draw_chain(rs, random.Random(c['py_seed']), c['n'], c['H'], c['W'], c['max_k'], c['p'], dropout=c['video'], from_alpha=c['video'])
        orders.update(d.morph[:, 3].tolist())
        flags.update(d.downup.tolist())
        live = [(p, r) for p, r in enumerate(d.cut.tolist()) if r[0] >= 0]
        cuts.update('internal' if r[0] == p else 'external' for p, r in live)
        if not live:
            cuts.add('neither')
        assert (d.morph[:, 0] == 127).all() if c['video'] else np.array_equal(d.morph[:, 0], np.floor(d.thresh).astype(np.int32))
        if c['video']:
            m = M.chain(M.golden_inputs(name), d)
            sel = maskgen.draw_dropout(rs, M.stats(m))
            drops.update('zeroed' if e[0] >= 0 else 'skipped' for e in sel.tolist())
    assert orders == {0, 1, 2, 3} and flags == {0, 1} and cuts == {'internal', 'external', 'neither'} and drops == {'zeroed', 'skipped'}


def _apply_tables(src, ax_x, ax_y):
    """One 8-bit bilinear resize from (ofs, c0, c1) axes: the arithmetic of the kernel, in NumPy."""
    (xo, a0, a1), (yo, b0, b1) = ax_x, ax_y
    H, W = src.shape
    S = src.astype(np.int32)
    rows = S[:, xo] * a0.astype(np.int32)[None] + S[:, np.minimum(xo + 1, W - 1)] * a1.astype(np.int32)[None]
    R0, R1 = rows[yo], rows[np.minimum(yo + 1, H - 1)]
    return ((((b0.astype(np.int32)[:, None] * (R0 >> 4)) >> 16) + ((b1.astype(np.int32)[:, None] * (R1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


@pytest.mark.parametrize('H,W', [(64, 64), (96, 160), (253, 331), (512, 512)])
def test_resize_tables_match_a_float_formulation(H, W):
    """Fixed point against float64 with exact weights and no rounding of the small image. The two may differ by the rounding of the small image
    (0.5 level), of the coefficients (2 x 255 / 4096 per pass) and of the result (0.5): under 1.0 in all, so the thresholded results must agree
    wherever the float value is farther than 1.0 from 127.5, and such close calls must be rare (<= 0.5 % of the pixels)."""
    t = maskgen.resize_tables(H, W, 0.125)
    for name, (src, dst, scale) in {'down_x': (W, t['dw'], 8.0), 'down_y': (H, t['dh'], 8.0), 'up_x': (t['dw'], W, 1.0 / (W / t['dw'])),
                                    'up_y': (t['dh'], H, 1.0 / (H / t['dh']))}.items():
        for mine, theirs in zip(t[name], M.resize_axis(src, dst, scale)):                     # vectorised against index-by-index
            assert np.array_equal(np.asarray(mine, np.int64), np.asarray(theirs, np.int64)), name
        assert (t[name][1].astype(np.int32) + t[name][2] == maskgen.COEF_ONE).all()
    assert t['tab'].dtype == np.int32 and t['tab'].shape == (3 * (t['dw'] + t['dh'] + W + H),)
    m = M.noisy_ellipse(H * 1000 + W, H, W)
    small = _apply_tables(m, t['down_x'], t['down_y'])
    assert small.shape == (t['dh'], t['dw'])
    fixed = _apply_tables(small, t['up_x'], t['up_y'])
    assert np.array_equal((fixed > 127) * np.uint8(255), M.downup(m))
    flt = M.resize_float(M.resize_float(m, (0, 0), 0.125, 0.125), (W, H))
    assert np.abs(fixed.astype(np.float64) - flt).max() < 1.0
    decided = np.abs(flt - 127.5) > 1.0
    assert np.array_equal((fixed > 127)[decided], (flt > 127.5)[decided])
    assert 1.0 - decided.mean() <= 0.005


def test_resize_geometry_and_same_size_copy():
    assert (maskgen.resize_tables(20, 12)['dh'], maskgen.resize_tables(20, 12)['dw']) == (2, 2)       # 2.5 and 1.5: round half to even
    assert (maskgen.resize_tables(5, 5)['dh'], maskgen.resize_tables(253, 331)['dw']) == (1, 41)
    a = G.noise_planes(3, 1, 17, 23)[0]
    assert np.array_equal(M.resize(a, (23, 17)), a)                                           # GenMaskFromAlpha's resize


def test_argument_errors_come_before_the_device():
    x = torch.zeros((2, 16, 16), dtype=torch.uint8)
    for k in (0, 32, -3):
        with pytest.raises(ValueError):
            maskgen.binarize_morph(x, 100.0, k, 3, 'dilate')
        with pytest.raises(ValueError):
            maskgen.binarize_morph(x, 100.0, 3, k, 'erode')
    with pytest.raises(ValueError):
        maskgen.binarize_morph(x, 100.0, 3, 3, 'open')
    with pytest.raises(ValueError):
        maskgen.binarize_morph(x, 100.0, [3, 3, 3], 3, 'dilate')                              # three entries for two planes
    with pytest.raises(ValueError):
        maskgen.draw_chain(np.random.RandomState(0), random.Random(0), 2, 64, 64, binarize_max_k=64)     # draws k > 31 for some plane
    with pytest.raises(ValueError):
        maskgen.resize_tables(3, 64)                                                        # round(0.375) = 0 rows
    with pytest.raises(ValueError):
        maskgen.down_up(torch.zeros((1, 64, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        maskgen.from_alpha(torch.zeros((1, 2, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        maskgen.resize_tables(64, 64, 2.0)
    for bad in (torch.zeros((2, 16, 16)), np.zeros((2, 16, 16), np.int32)):
        for fn in (lambda v: maskgen.binarize_morph(v, 100.0), maskgen.down_up, maskgen.from_alpha, maskgen.stats,
                   lambda v: maskgen.cut(v, np.full((2, 8), -1, np.int32))):
            with pytest.raises(TypeError):
                fn(bad)
    draws = maskgen.draw_chain(np.random.RandomState(1), random.Random(1), 2, 16, 16)
    with pytest.raises(ValueError):
        maskgen.synthesize(torch.zeros((3, 16, 16), dtype=torch.uint8), draws)                # three planes, draws for two
    with pytest.raises(TypeError):
        maskgen.synthesize(x, None)
    drop = maskgen.draw_chain(np.random.RandomState(1), random.Random(1), 2, 16, 16, dropout=True)
    with pytest.raises(ValueError):
        maskgen.synthesize(x, drop)                                                         # drop-out without its RandomState
    with pytest.raises(ValueError):
        maskgen.cut(x, np.zeros((3, 8), np.int32))
    with pytest.raises(ValueError):
        maskgen.drop(x, np.asarray([[1, 0, 2, 2], [1, 3, 2, 2]], np.int32), np.zeros((2, 5), np.int32))     # the same plane twice


def test_cut_draws_raise_the_references_error_on_tiny_planes():
    """randint(h // 8, h // 4) has an empty range below 4 rows / columns (0 .. 0); the error is numpy's own, as in the reference. The branch is
    random: every seed either raises or skips the cut, and some seed of the first eight raises. The boundary is 4, not 8: for 4 <= h < 8
    the reference's randint(h // 8, h // 4) is randint(0, 1), which draws a rectangle of height 0 -- a cut that changes nothing, not an
    error -- so draw_chain follows it and raises nothing there."""
    raised = 0
    for seed in range(8):
        try:
            d = maskgen.draw_chain(np.random.RandomState(seed), random.Random(seed), 3, 3, 64)
            assert (d.cut[:, 0] == -1).all()
        except ValueError:                                                                  # numpy's own: the wording is its version's
            raised += 1
    assert raised > 0
    d = maskgen.draw_chain(np.random.RandomState(0), random.Random(0), 3, 8, 8)                 # every branch draws a rectangle that is not empty from 8 on
    assert d.cut.shape == (3, 8)


def test_draw_order_is_the_references():
    """The streams are consumed call by call as transforms.py does: replaying the same calls by hand lands on the same generator state."""
    for seed in range(6):
        rs, ref = np.random.RandomState(seed), np.random.RandomState(seed)
        py, pyref = random.Random(seed), random.Random(seed)
        P, H, W = 4, 40, 72
        d = maskgen.draw_chain(rs, py, P, H, W)
        for p in range(P):
            t = ref.uniform(0.1, 0.95) * 255
            kd, ke = ref.randint(1, 30), ref.randint(1, 30)
            o = ref.choice(['dilate_erode', 'erode_dilate', 'dilate', 'erode'])
            assert d.thresh[p] == t and d.morph[p].tolist() == [int(np.floor(t)), kd, ke, M.ORDERS.index(o)]
        assert d.downup.tolist() == [int(ref.rand() < 0.5) for _ in range(P)]
        if ref.random() < 0.5:
            for p in range(P):
                if ref.rand() < 0.5:
                    ph, pw = ref.randint(H // 8, H // 4), ref.randint(W // 8, W // 4)
                    x, y, x1, y1 = ref.randint(0, H - ph), ref.randint(0, W - pw), ref.randint(0, H - ph), ref.randint(0, W - pw)
                    assert d.cut[p].tolist() == [p, x, y, x1, y1, ph, pw, 0]
                else:
                    assert d.cut[p, 0] == -1
        elif ref.rand() < 0.5:
            i, j = pyref.sample(list(range(P)), k=2)
            ph, pw = ref.randint(H // 8, H // 4), ref.randint(W // 8, W // 4)
            x, y = ref.randint(0, H - ph), ref.randint(0, W - pw)
            assert d.cut[i].tolist() == [j, x, y, x, y, ph, pw, 0] and d.cut[j].tolist() == [i, x, y, x, y, ph, pw, 0]
        assert rs.rand() == ref.rand() and py.random() == pyref.random()


def test_draw_dropout_skips_and_selects():
    st = np.asarray([[0, 64, -1, 48, -1], [500, 10, 60, 5, 44], [30, 3, 12, 3, 40], [900, 0, 63, 0, 47], [400, 8, 40, 8, 40], [77, 1, 30, 2, 30]], np.int32)
    seen = set()
    for seed in range(40):
        rs = np.random.RandomState(seed)
        sel = maskgen.draw_dropout(rs, st)
        assert sel.dtype == np.int32 and sel.shape[1] == 4
        for i, idx, ph, pw in sel.tolist():
            if i < 0:
                assert -i - 1 in (0, 2) and (idx, ph, pw) == (0, 0, 0)                      # the empty plane; the 10-pixel-wide one
                seen.add('skipped')
            else:
                count, xmin, xmax, ymin, ymax = st[i].tolist()
                assert 0 <= idx < count and (ymax - ymin + 1) // 16 <= ph < (ymax - ymin + 1) // 8 and (xmax - xmin + 1) // 16 <= pw < (xmax - xmin + 1) // 8
                seen.add('live')
        live = [e[0] for e in sel.tolist() if e[0] >= 0]
        assert len(set(live)) == len(live) and sel.shape[0] <= 2                            # randint(1, P // 2) planes, without replacement
        if sel.shape[0] == 0:
            seen.add('not taken')
    assert seen == {'skipped', 'live', 'not taken'}
    assert maskgen.draw_dropout(np.random.RandomState(0), st[:5]).shape == (0, 4)              # P // 2 < 3: never


def test_no_gpu_means_an_error_not_a_fallback():
    if torch.cuda.is_available():
        return
    from maggie_amd.hip import MaggieHipError
    x = torch.zeros((2, 16, 16), dtype=torch.uint8)
    draws = maskgen.draw_chain(np.random.RandomState(1), random.Random(1), 2, 16, 16)
    for fn in (lambda: maskgen.synthesize(x, draws), lambda: maskgen.from_alpha(x), lambda: maskgen.binarize_morph(x, 100.0, 3, 3),
               lambda: maskgen.down_up(x), lambda: maskgen.stats(x), lambda: draws.to('cuda')):
        with pytest.raises(MaggieHipError):
            fn()
