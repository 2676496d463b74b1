"""Child process of tests/test_gpu_tokens.py::test_other_compiled_forms_give_the_bits_of_the_default_forms: the forward cross-attention,
self-attention and mask pre-processing cases of tests/tokens_reference.py (fixed seeds) through whatever kernel forms the environment selects --
MG_ATTN_FWD_RG, MG_TOKEN_SA_LDS and MG_IMD_PREP_PLANES are read once per process, so every other form needs a process of its own. The parent calls
outputs() in its own process (the default forms) and requires the same bits.
usage: python tests/token_forms_worker.py <out.npz>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                  # noqa: E402
import torch                        # noqa: E402

import tokens_reference as TR       # noqa: E402


def outputs():
    from maggie_amd import functional as MF, kernels as K
    dev = torch.device('cuda:0')
    out = {}

    def put(name, t):
        out[name] = t.detach().cpu().numpy().copy()

    for ci, (B, L, NID) in enumerate(TR.ATTN_CASES):
        c = TR.attn_case(B, L, NID)
        d = {n: (v.to(dev) if torch.is_tensor(v) else v) for n, v in c.items()}
        p, ctx = K.attn_tok_fwd(d['qk'], d['btab'], d['feat'], d['ids'], c['scale'])
        put('attn%d_tok_p' % ci, p)
        put('attn%d_tok_ctx' % ci, ctx)
        for tn in (False, True):
            pad = c['pads'][(ci + tn) % 3]
            b2 = d['b2'].transpose(1, 2).contiguous() if tn else d['b2']
            o, p2 = K.attn_feat_fwd(d['feat'], d['kq'], b2, d['vp'], d['obias'], None if pad is None else pad.to(dev), d['ids'], c['scale'], tn)
            put('attn%d_feat_out_tn%d' % (ci, tn), o)
            put('attn%d_feat_p_tn%d' % (ci, tn), p2)
    for si, (B, T, D) in enumerate(TR.SA_CASES):
        c = TR.sa_case(B, T, D)
        for pi, pad in enumerate(c['pads']):
            q, k, v = (c[n].to(dev).requires_grad_(True) for n in 'qkv')
            o = MF.token_self_attention(q, k, v, None if pad is None else pad.to(dev))
            put('sa%d_out_pad%d' % (si, pi), o)
            put('sa%d_p_pad%d' % (si, pi), o.grad_fn.saved_tensors[3])
    for ii, case in enumerate(TR.IMD_CASES):
        B, NF, n_in, n_gt, n_i, h, w, s, gs = case
        mask, gt = TR.imd_case(*case, seed=ii)
        ids, guid, valid = K.imd_prep(mask.to(dev), None if gt is None else gt.to(dev), h, w, n_i)
        put('imd%d_ids' % ii, ids)
        put('imd%d_valid' % ii, valid)
        if guid is not None:
            put('imd%d_guidance' % ii, guid)
    torch.cuda.synchronize()
    return out


if __name__ == '__main__':
    np.savez(sys.argv[1], **outputs())
    print('DONE %s' % ' '.join('%s=%s' % (k, os.environ.get(k, '-')) for k in ('MG_ATTN_FWD_RG', 'MG_TOKEN_SA_LDS', 'MG_IMD_PREP_PLANES')))
