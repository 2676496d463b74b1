"""The launch sequence of the training item's wiring (DevicePreprocessor.train_item / train_item_affine / train_item_photo): which kernels run,
in which order, for every combination of {photo: none / lut only / fired} x {affine: none / unfired / fired} x {warp_masks} x {the masks are
the alphas / separate masks}, on the two crop fixture cases that reach both crop branches.

The expected sequences below were RECORDED ON THE PARENT COMMIT of the change that merged the three wirings into one (the commit that still
had three method bodies), by running `record` of this file on an MI355X; they are not derived from the code under test. The two cases
recorded the same table; only the crop's kernel differs (CROP_KERNEL). A change that adds, drops or reorders a launch for any combination
fails here: with no kernel and no launch argument changed, equal sequences are the evidence that the device time of an item is what it was."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import crop_restatement as C                                          # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import affine, crop, photometric                # noqa: E402
from maggie_amd.utils import maskgen as MG                            # noqa: E402
from maggie_amd.utils.preprocess import DevicePreprocessor            # noqa: E402

pytestmark = pytest.mark.gpu

PHOTO, AFFINE = ('none', 'lut', 'fired'), ('none', 'unfired', 'fired')
COLUMNS = [(wm, masks) for wm in (False, True) for masks in ('alphas', 'separate')]       # the four entries of a row of EXPECTED

CROP_KERNEL = {'first_hit': 'mg_crop_gather', 'pad_wide_odd': 'mg_crop_padresize'}          # 'crop' below: the case's branch
# every item ends with: alpha into the slots, the mask chain, the masks into the slots, the transition band
ASSEMBLE = ('mg_preprocess_planes', 'mg_mask_morph', 'mg_mask_downup', 'mg_mask_cut', 'mg_preprocess_planes', 'mg_transition_gt')
JPEG, WARP = ('mg_jpeg_ycc', 'mg_jpeg_rgb'), ('mg_affine_warp_frames', 'mg_affine_warp_planes', 'mg_affine_shift_normalize')
# the eight distinct sequences the parent took: the crop of the frames and the alphas, and of separate masks when the mask chain reads them
SEQUENCES = {
    'A': ('crop', 'crop') + ASSEMBLE,
    'B': ('crop', 'crop', 'crop') + ASSEMBLE,
    'C': ('crop', 'crop') + WARP + ASSEMBLE,
    'D': ('crop', 'crop', 'crop') + WARP + ASSEMBLE,
    'E': ('crop', 'crop') + JPEG + ASSEMBLE,
    'F': ('crop', 'crop', 'crop') + JPEG + ASSEMBLE,
    'G': ('crop', 'crop') + JPEG + WARP + ASSEMBLE,
    'H': ('crop', 'crop', 'crop') + JPEG + WARP + ASSEMBLE,
}
# (photo, affine) -> the sequence of each of COLUMNS: warp_masks False (masks alphas, separate), warp_masks True (masks alphas, separate)
EXPECTED = {
    ('none', 'none'): 'A B A B',
    ('none', 'unfired'): 'A B A B',
    ('none', 'fired'): 'C D C C',
    ('lut', 'none'): 'A B A B',
    ('lut', 'unfired'): 'A B A B',
    ('lut', 'fired'): 'C D C C',
    ('fired', 'none'): 'E F E F',
    ('fired', 'unfired'): 'E F E F',
    ('fired', 'fired'): 'G H G G',
}


def _inputs(name, dev):
    c = C.GOLDEN[name]
    frames, alphas, masks = C.golden_inputs(name)
    T, n = c['T'], c['n']
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)          # noqa: E731
    f, a, m = up(frames), up(alphas.reshape(T, n, c['h'], c['w'])), up(masks.reshape(T, n, c['h'], c['w']))
    cd = crop.draw_on_device(np.random.RandomState(c['rs_seed']), alphas, c['crop'], c['pp'], c['fp']).to(dev)
    oh, ow = cd.out_h, cd.out_w
    fired, unfired = affine.draw(np.random.RandomState(7), oh, ow, p=1.0), affine.draw(np.random.RandomState(5), oh, ow, p=0.1)
    assert fired.fired and fired.matrix is not None and not unfired.fired
    crop_lut = np.random.default_rng(1).integers(0, 256, (3, 256), dtype=np.uint8)
    photo_lut = np.random.default_rng(2).integers(0, 256, (3, 256), dtype=np.uint8)
    noise = np.random.default_rng(3).integers(-40, 41, (oh, ow, 1)).astype(np.int16)
    return dict(f=f, a=a, m=m, cd=cd, ids=[4, 1][:n], crop_lut=crop_lut, both=np.stack([photo_lut[ch][crop_lut[ch]] for ch in range(3)]),
                md=MG.draw_chain(np.random.RandomState(9), random.Random(9), T * n, oh, ow, from_alpha=T > 1),
                affine={'none': None, 'unfired': unfired, 'fired': fired},
                photo={'none': None, 'lut': photometric.PhotoDraws(lut=photo_lut), 'fired': photometric.PhotoDraws(photo_lut, noise, 35)})


def _recorded(monkeypatch, fn):
    """(what `fn` returns, the names of the kernels it launched): every stage launches through `hip.call(name, ...)`."""
    names, real = [], hip.call

    def call(name, *args, **kwargs):
        names.append(name)
        return real(name, *args, **kwargs)
    with monkeypatch.context() as mp:
        mp.setattr(hip, 'call', call)
        out = fn()
    return out, tuple(names)


def record(name, monkeypatch, dev):
    """{(photo, affine, warp_masks, masks): (item, launches)} of `train_item_photo`, the one method that takes every combination."""
    x = _inputs(name, dev)
    pre = DevicePreprocessor(max_inst=6, device=dev)
    out = {}
    for p in PHOTO:
        for ad in AFFINE:
            for wm, masks in COLUMNS:
                out[(p, ad, wm, masks)] = _recorded(monkeypatch, lambda: pre.train_item_photo(
                    x['f'], x['a'], x['a'] if masks == 'alphas' else x['m'], x['cd'], x['photo'][p], x['affine'][ad], x['ids'],
                    transition=(3, 2), mask_draws=x['md'], lut=x['crop_lut'], warp_masks=wm))
    return x, pre, out


def _same(got, want):
    return list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize('name', ['first_hit', 'pad_wide_odd'])
def test_every_combination_takes_the_parents_launches_and_equals_its_public_method(name, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    dev = torch.device('cuda:0')
    x, pre, got = record(name, monkeypatch, dev)
    for p in PHOTO:
        for ad in AFFINE:
            row = EXPECTED[(p, ad)].split()
            for (wm, masks), letter in zip(COLUMNS, row):
                item, launches = got[(p, ad, wm, masks)]
                print(name, p, ad, wm, masks, ' '.join(launches))
                assert launches == tuple(CROP_KERNEL[name] if k == 'crop' else k for k in SEQUENCES[letter]), (p, ad, wm, masks)
                assert list(item) == ['image', 'alpha', 'mask', 'transition']
                # the narrowest public method that takes this combination: the same item through the same launches
                mk = x['a'] if masks == 'alphas' else x['m']
                kw = dict(transition=(3, 2), mask_draws=x['md'])
                lut = x['both'] if p == 'lut' else x['crop_lut']                  # a lone photo.lut is the crop's table followed by it
                via_affine, same_launches = _recorded(monkeypatch, lambda: pre.train_item_affine(
                    x['f'], x['a'], mk, x['cd'], x['affine'][ad], x['ids'], lut=lut, warp_masks=wm, **kw))
                if p == 'fired':                                                  # only train_item_photo takes it; the planes never see the steps
                    assert all(torch.equal(item[k], via_affine[k]) for k in ('alpha', 'mask', 'transition'))
                    assert not torch.equal(item['image'], via_affine['image'])
                    continue
                assert _same(item, via_affine) and same_launches == launches
                if ad != 'fired':
                    plain, same_launches = _recorded(monkeypatch, lambda: pre.train_item(x['f'], x['a'], mk, x['cd'], x['ids'], lut=lut, **kw))
                    assert _same(item, plain) and same_launches == launches
