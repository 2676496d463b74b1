"""Child process of tests/test_gpu_losses.py::test_first_forms_give_the_bits_of_the_batched_forms: the small cases of tests/losses_reference.py
and the large one (fixed seeds, with and without pvalid) through whatever forms of the pyramid / Sobel-adjoint stencils the environment selects --
MG_LOSS_BATCHED is read once per process, so the first forms need a process of their own. Per case: the per-kernel pipeline on scale 0
and the three-scale pipeline; the per-pixel outputs G0..G2 (planes without weight zeroed: the kernels leave them unwritten), dpred, and
the three loss values. The parent calls outputs() in its own process (the default forms) and requires the same per-pixel bits.
usage: python tests/loss_forms_worker.py <out.npz>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                  # noqa: E402
import torch                        # noqa: E402

import losses_reference as LR       # noqa: E402


CASES = LR.SMALL + [LR.LARGE]        # the large case takes the first pyr_lap_fwd through the `break` of its 4-way unrolled loop


def run_single(case, s, with_valid, dev):
    """The per-kernel C ABI path on scale s -> values (3,), dpred (P, H, W), [G0, G1, G2] (weightless planes zeroed)."""
    from maggie_amd import functional as MF
    pd = case['preds'][s].to(dev).requires_grad_(True)
    pv = case['pvalid'].to(dev) if with_valid else None
    out = MF.MattingLosses.apply(pd, case['target'].to(dev), case['weights'][s].to(dev), pv)
    saved = out.grad_fn.saved_tensors
    flags, Gs = saved[3], [g.clone() for g in saved[5:8]]
    for g in Gs:
        g[flags == 0] = 0
    (out * torch.tensor(LR.GOUT, device=dev)).sum().backward()
    return out.detach(), LR.planes(pd.grad), Gs


def run_multi(case, with_valid, dev):
    """The three scales in one set of launches -> values (S, 3), [dpred per scale], [G0, G1, G2] over S * P planes."""
    from maggie_amd import functional as MF
    pds = [p.to(dev).requires_grad_(True) for p in case['preds']]
    pv = case['pvalid'].to(dev) if with_valid else None
    out = MF.MattingLossesMulti.apply(case['target'].to(dev), pv, *pds, *[w.to(dev) for w in case['weights']])
    saved = out.grad_fn.saved_tensors
    flags, Gs = saved[1], [g.clone() for g in saved[3:6]]
    for g in Gs:
        g[flags == 0] = 0
    (out * torch.tensor(LR.GOUT, device=dev)[None, :]).sum().backward()
    return out.detach(), [LR.planes(p.grad) for p in pds], Gs


def outputs():
    dev = torch.device('cuda:0')
    out = {}

    def put(name, t):
        out[name] = t.detach().cpu().numpy().copy()

    for c in CASES:
        case = LR.make_case(*c)
        for wv in (0, 1):
            tag = '%s_pv%d' % (LR.case_id(c), wv)
            vals, dp, Gs = run_single(case, 0, bool(wv), dev)
            put(tag + '_single_values', vals)
            put(tag + '_single_dpred', dp)
            for l, g in enumerate(Gs):
                put(tag + '_single_G%d' % l, g)
            vals, dps, Gs = run_multi(case, bool(wv), dev)
            put(tag + '_multi_values', vals)
            for s, dp in enumerate(dps):
                put(tag + '_multi_dpred%d' % s, dp)
            for l, g in enumerate(Gs):
                put(tag + '_multi_G%d' % l, g)
    torch.cuda.synchronize()
    return out


if __name__ == '__main__':
    np.savez(sys.argv[1], **outputs())
    print('DONE MG_LOSS_BATCHED=%s' % os.environ.get('MG_LOSS_BATCHED', '-'))
