"""Generate tests/golden/pngenc_pinned.npz FROM THE REFERENCE (build container only; run it in its own interpreter):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pngenc_golden.py

The reference's own `save_visualization` (maggie/engine/test.py) runs on seeded inputs with a recording stand-in for cv2 (as make_conn_golden.py
stubs it): `cv2.imwrite(path, array)` keeps the path relative to save_dir and the array, and creates an empty file so that the reference's
"skip if the file exists" sees what it would have seen. Three calls: 'named' (alpha names given, with diff_pred and inc_bin_maps, 2 frames x 3
instances of 24 x 40 behind a same-size resize and a padding of (2, 3); called twice, so that the second call's skipped files are pinned too), 'numbered' (no alpha
names, 3 instances) and 'single' (one instance).

Stored per call: '<call>.image_names', '.alpha_names', '.alphas', '.diff_pred', '.inc_bin_maps' (the inputs), '.pad' and '.paths' /
'.plane_<i>' (what imwrite was handed, in order)."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

CALLS = []


def _imwrite(path, array):
    CALLS.append((path, np.array(array, copy=True)))
    with open(path, 'wb'):
        pass
    return True


def install_standins():
    cv2 = types.ModuleType('cv2')
    cv2.imwrite = _imwrite
    cv2.INTER_LINEAR = 1
    sys.modules['cv2'] = cv2
    if 'skimage' not in sys.modules:                           # postprocessing.py binds skimage.measure.label at import; nothing here calls it
        sk, meas = types.ModuleType('skimage'), types.ModuleType('skimage.measure')
        meas.label = None
        sk.measure = meas
        sys.modules['skimage'], sys.modules['skimage.measure'] = sk, meas


def inputs(tag):
    import torch
    rng = np.random.RandomState({'named': 1, 'numbered': 2, 'single': 3}[tag])
    T, n_i, H, W, pad = 2, (1 if tag == 'single' else 3), 24, 40, (2, 3)
    yy, xx = np.mgrid[0:H, 0:W]
    alphas = np.zeros((1, T, n_i, H, W), np.float32)
    for t in range(T):
        for i in range(n_i):
            d = np.hypot((yy - 8 - 3 * i - t) / 7.0, (xx - 12 - 6 * i) / 9.0)
            alphas[0, t, i] = np.clip((1.2 - d) / 0.5, 0, 1)
    alphas = (np.round(alphas * 255) / 255).astype(np.float32)
    r = dict(image_names=['data/val/clip_%s/%04d.png' % (tag, t) for t in range(T)], alphas=alphas, pad=np.asarray(pad))
    if tag == 'named':
        r['alpha_names'] = ['inst_%d.png' % i for i in range(n_i)]
        r['diff_pred'] = torch.from_numpy(rng.rand(1, T, 1, H + pad[0], W + pad[1]).astype(np.float32))
        r['inc_bin_maps'] = torch.from_numpy((rng.rand(1, T, 1, H + pad[0], W + pad[1]) > 0.4).astype(np.float32))
    return r


def main():
    from oracle import ref_loader
    ref_loader.load_reference()                                # registers the reference's packages (and its own stand-ins for the model path)
    install_standins()                                         # engine/test.py binds cv2 at import
    import importlib
    import maggie
    eng = types.ModuleType('maggie.engine')                    # the package without its __init__, which pulls the trainer in (wandb)
    eng.__path__ = [os.path.join(list(maggie.__path__)[0], 'engine')]
    sys.modules['maggie.engine'] = eng
    if 'maggie.dataloader' not in sys.modules:                 # its transforms need albumentations; save_visualization needs none of it
        sys.modules['maggie.dataloader'] = types.ModuleType('maggie.dataloader')
    for mod, attr in (('maggie.dataloader', 'build_dataset'), ('maggie.network', 'build_model')):
        if not hasattr(sys.modules[mod], attr):                # names engine/test.py imports and save_visualization never calls
            setattr(sys.modules[mod], attr, None)
    E = importlib.import_module('maggie.engine.test')
    out = {}
    for tag in ('named', 'numbered', 'single'):
        r = inputs(tag)
        H, W = r['alphas'].shape[-2:]                          # a resize to the size the crop leaves: exact in both implementations
        info = [{'name': 'resize', 'ori_size': (H, W)}, {'name': 'padding', 'pad_size': (int(r['pad'][0]), int(r['pad'][1]))}]
        output = {}
        if 'diff_pred' in r:
            output = {'diff_pred': r['diff_pred'], 'inc_bin_maps': [r['inc_bin_maps']]}
        names = [[n] for n in r['image_names']]
        anames = [[n] for n in r['alpha_names']] if 'alpha_names' in r else None
        del CALLS[:]
        with tempfile.TemporaryDirectory() as d:
            for _ in range(2 if tag == 'named' else 1):
                E.save_visualization(names, anames, r['alphas'], info, output, d)
            rel = [os.path.relpath(p, d) for p, _ in CALLS]
        out[tag + '.paths'] = np.asarray(rel)
        for i, (_, a) in enumerate(CALLS):
            assert a.dtype == np.uint8 and a.ndim == 2
            out['%s.plane_%d' % (tag, i)] = a
        for k, v in r.items():
            out[tag + '.' + k] = np.asarray(v)
    np.savez_compressed(os.path.join(HERE, 'pngenc_pinned.npz'), **out)
    print('wrote pngenc_pinned.npz', {k: v.shape for k, v in out.items() if not k.split('.')[1].startswith('plane_')})
    print(out['named.paths'])


if __name__ == '__main__':
    main()
