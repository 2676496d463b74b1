"""Child process of tests/test_gpu_conv_exact.py::test_large_lds_forms_on_a_second_device: a FRESH process (the library's per-device once-masks are
fresh), in which the forms named on the command line run on cuda:0 and then on cuda:1 (the test names two forms that ask for more than 64 KiB of
dynamic LDS, the one-slab form, which sizes its grid by the device's CU count, and the gather9 weight gradient, which asks for 60 KiB). The conv cases are the smallest tests/conv_exact.py case of their form and must hold their
exact-integer expectation on both devices; one mg_token_linear_multi_fwd call (66 KiB of LDS) must return the same bits on both.
usage: python tests/second_device_worker.py DEVICE,DEVICE FORM...  -> 'RESULT {...}' ("<form>@<device>": "ok" or the failure; "token_equal": bool)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                # noqa: E402

import conv_exact as X                      # noqa: E402
import test_gpu_conv_exact as T             # noqa: E402


def smallest(form):
    def work(c):
        Ho, Wo = X.out_hw(c)
        return (c.N if c.mode == 'GATHER' else c.N * Ho * Wo) * c.Cout * c.k * c.k * c.Cin
    return min(X.cases_by_form()[form], key=work)


def token(dev):
    from maggie_amd import functional as MF
    g = torch.Generator().manual_seed(9)
    x, w, b = torch.randn(11, 128, generator=g), torch.randn(128, 128, generator=g) / 11, torch.randn(128, generator=g)
    with torch.no_grad():
        a, = MF.token_linear_multi([dict(x=x.to(dev), W=w.to(dev), b=b.to(dev))])      # K = N = 128: W alone is 66 048 bytes of LDS
    return a.cpu()


def main():
    res, tok = {}, []
    try:
        for d in [int(v) for v in sys.argv[1].split(',')]:
            torch.cuda.set_device(d)
            dev = torch.device('cuda', d)
            for form in sys.argv[2:]:
                c = smallest(form)
                dtype = X.DTYPES[c.dtypes[0]]
                X.check_conditions(c, dtype)
                try:
                    (T._run_wgrad if c.kind == 'wgrad' else T._run_fprop)(c, dtype, dev)
                    res['%s@%d' % (form, d)] = 'ok'
                except AssertionError as e:
                    res['%s@%d' % (form, d)] = 'assert: %s' % str(e)[:500]
            tok.append(token(dev))
            torch.cuda.synchronize()
        res['token_equal'] = bool(torch.equal(tok[0], tok[1])) and bool(tok[0].isfinite().all())
    except Exception as e:                  # a launch or device error: nothing more goes to a device from this process
        res['error'] = repr(e)[:1000]
    print('RESULT ' + json.dumps(res))
    return 1 if 'error' in res else 0


if __name__ == '__main__':
    sys.exit(main())
