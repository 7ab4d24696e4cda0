"""Golden vectors for the smoke inference driver by RUNNING the reference's InferencePipeline (smoke/inference_2d.py:99-456).

Build-container only (needs /root/reference):   python tests/golden/make_ref_smoke_inference_golden.py
Writes tests/golden/ref_smoke_inference.npz, ref_smoke_inference_1.npz and ref_smoke_inference_manifest.json -- data only. The inputs are
regenerated on any host by tests/smoke_inference_inputs.py (an integer hash), so only outputs are stored:
  (a) the `init` and `control` conditions run_model hands to sample(), at the conditioned positions (init: the first and last frame of
      every sub-band's run; control: rows ::4 of the coefficient block), and the largest magnitude outside the block (zero);
  (b) run_base_model's fp32 pred and its fp64 difference to the exact value (the same code run on fp64 tensors) -- channel 5 in full (one
      value per frame), channels 0..4 on four frames and rows ::3, plus the reference's own error over the WHOLE tensor as numbers. The
      whole tensors (7.8 MB for the full-shape case) do not fit a committed file; the tests rebuild the exact value with oracle/dwt_ref.py
      and the stored entries pin that rebuild to the reference's fp64 run;
  (c) the five arrays of multi_evaluate in the case's mode, on a hash-generated pred. In control mode multi_evaluate_control is replaced on
      the instance by a function returning a hash-generated solver_out.

What runs is the reference's own code. The third-party routines it calls that are absent here (ptwt.waverec3 / wavedec3,
pytorch_wavelets.DWT1DInverse / DWTForward, pywt.Wavelet) are torch stand-ins, CHECKED against oracle/dwt_ref.py to 1e-12 in fp64 before
anything is generated (make_ref_guidance_golden.py does the first half of this). The model is a stub whose sample() records its keywords
and returns tests/helpers.guidance_input. multi_evaluate as written reads a local name that only its super-resolution branch assigns, so
without a super model it stops with UnboundLocalError before its first print; the generator compiles the method's own source, taken
from the reference at run time, with that name assigned after the docstring, and calls that. Two of the reference's hard-coded sizes are
met as follows: run_base_model expands the
smoke-out plane to 64 x 64 cells whatever the field size, so for the 32 x 32 cases that one expand() is given the field size; and
multi_evaluate keeps one cell in 4 of solver_out, so the stand-in solver_out has twice the field's cells per side.
"""
import inspect
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_ref_golden as M  # noqa: E402
from oracle import dwt_ref as R  # noqa: E402
from tests import smoke_inference_inputs as SI  # noqa: E402

M.STUBS['matplotlib/__init__.py'] = ''
M.STUBS['matplotlib/pyplot.py'] = ''
M.STUBS['dataset/__init__.py'] = ''
M.STUBS['dataset/evaluate_solver.py'] = ''
M.install_stubs()


# ---- differentiable stand-ins (zero-padding mode synthesis = transposed stride-2 convolution, then drop p = (2L-3)//2 at both ends)
def _synth(lo, hi, wave, axis):
    _, _, gl, gh = R.filter_bank(wave)
    lo, hi = lo.movedim(axis, -1), hi.movedim(axis, -1)
    m_, L = lo.shape[-1], len(gl)

    def up(t):
        z = torch.zeros(t.shape[:-1] + (2 * m_ - 1,), dtype=t.dtype)
        z[..., ::2] = t
        return z
    ul, uh = up(lo), up(hi)
    y = 0
    for m in range(L):
        y = y + F.pad(ul * float(gl[m]) + uh * float(gh[m]), (m, L - 1 - m))
    p = (2 * L - 3) // 2
    return y[..., p:y.shape[-1] - p].movedim(-1, axis)


class _Wavelet:
    def __init__(self, name):
        self.name = name


def _waverec3(coeffs, wavelet):
    c = dict(coeffs[1])
    c['aaa'] = coeffs[0]
    w = wavelet.name
    lvl = {th: _synth(c[th + 'a'], c[th + 'd'], w, -1) for th in ('aa', 'ad', 'da', 'dd')}
    lvl2 = {t: _synth(lvl[t + 'a'], lvl[t + 'd'], w, -2) for t in ('a', 'd')}
    return _synth(lvl2['a'], lvl2['d'], w, -3)


class _DWT1DInverse:
    def __init__(self, mode='zero', wave='db1'):
        assert mode == 'zero'
        self.wave = wave

    def to(self, device):
        return self

    def __call__(self, coeffs):
        lo, his = coeffs
        return _synth(lo, his[0], self.wave, -1)


# check the stand-ins against the pinned oracle before trusting them
_rng = np.random.default_rng(3)
_lll = _rng.standard_normal((3, 10, 18, 18))
_det = {k: _rng.standard_normal((3, 10, 18, 18)) for k in ('aad', 'ada', 'add', 'daa', 'dad', 'dda', 'ddd')}
_a = _waverec3([torch.from_numpy(_lll), {k: torch.from_numpy(v) for k, v in _det.items()}], _Wavelet('bior1.3')).numpy()
_b = R.idwt3(_lll, _det, 'bior1.3')
assert _a.shape == _b.shape and np.abs(_a - _b).max() < 1e-12, np.abs(_a - _b).max()
_lo, _hi = _rng.standard_normal((2, 1, 18)), _rng.standard_normal((2, 1, 18))
assert np.abs(_DWT1DInverse('zero', 'bior1.3')((torch.from_numpy(_lo), [torch.from_numpy(_hi)])).numpy() - R.idwt1d(_lo, _hi, 'bior1.3', 'zero')).max() < 1e-12

pw = types.ModuleType('pytorch_wavelets')
pw.DWT1DInverse = _DWT1DInverse
pw.DWTForward = pw.DWTInverse = pw.DWT1DForward = None
sys.modules['pytorch_wavelets'] = pw
pt = types.ModuleType('ptwt')
pt.waverec3 = _waverec3
sys.modules['ptwt'] = pt
py = types.ModuleType('pywt')
py.Wavelet = _Wavelet
sys.modules['pywt'] = py

with M.cuda_default_args_on_cpu():
    import inference_2d as INF                     # noqa: E402  /root/reference/smoke/inference_2d.py



def _analysis(x, h, axis):
    x = x.movedim(axis, -1)
    L, N = len(h), x.shape[-1]
    p, nk = (2 * L - 3) // 2, (N + L - 1) // 2
    xp = F.pad(x, (p, p + N % 2 + 2))
    y = 0
    for m in range(L):
        y = y + float(h[L - 1 - m]) * xp[..., m:m + 2 * nk:2]
    return y.movedim(-1, axis)


def _wavedec3(x, wavelet, mode='zero', level=1):
    assert mode == 'zero' and level == 1
    dl, dh, _, _ = R.filter_bank(wavelet.name)
    out = {}
    for key in R.BANDS3:
        y = x
        for ax, letter in zip((-3, -2, -1), key):
            y = _analysis(y, dl if letter == 'a' else dh, ax)
        out[key] = y
    return [out.pop('aaa'), out]


class _DWTForward:
    def __init__(self, J=1, mode='zero', wave='db1'):
        assert J == 1 and mode == 'zero'
        self.wave = wave

    def to(self, device):
        return self

    def __call__(self, x):
        dl, dh, _, _ = R.filter_bank(self.wave)
        lo_w, hi_w = _analysis(x, dl, -1), _analysis(x, dh, -1)
        return _analysis(lo_w, dl, -2), [torch.stack([_analysis(lo_w, dh, -2), _analysis(hi_w, dl, -2), _analysis(hi_w, dh, -2)], dim=2)]


_rng = np.random.default_rng(5)
_x = _rng.standard_normal((2, 16, 32, 30))
_l, _d = _wavedec3(torch.from_numpy(_x), _Wavelet('bior1.3'))
_rl, _rd = R.dwt3(_x, 'bior1.3', 'zero')
assert list(_d) == list(R.BANDS3[1:]) and np.abs(_l.numpy() - _rl).max() < 1e-12 and all(np.abs(_d[k].numpy() - _rd[k]).max() < 1e-12 for k in _rd)
_x = _rng.standard_normal((2, 1, 32, 31))
_yl, _yh = _DWTForward(1, 'zero', 'bior1.3')(torch.from_numpy(_x))
_ryl, _ryh = R.dwt2(_x, 'bior1.3', 'zero')
assert np.abs(_yl.numpy() - _ryl).max() < 1e-12 and np.abs(_yh[0].numpy() - _ryh).max() < 1e-12
INF.ptwt.wavedec3 = _wavedec3
INF.DWTForward = _DWTForward


class _Model:
    wave_type, pad_mode = 'bior1.3', 'zero'

    def __init__(self, x, shape, ori):
        self.x, self.padded_shape, self.ori_shape, self.kw = x, list(shape), list(ori), None

    def sample(self, **kw):
        self.kw = kw
        return self.x.clone()


def _pipeline(name, dtype, tmp):
    tshape, shape, ori, cc, _ = SI.CASES[name]
    x, resc = SI.sample_output(name)
    model = _Model(x.to(dtype), shape, ori)
    args = types.SimpleNamespace(is_wavelet=True, is_condition_control=cc, image_size=64, device='cpu', upsample=0, is_super_model=False,
                                 w_energy=SI.W_ENERGY)
    ppl = INF.InferencePipeline([model], {'design_fn': None, 'design_guidance': 'standard'}, resc.to(dtype), results_path=tmp, args_general=args)
    return ppl, model


def _run_model(ppl, state, ori):
    """run_model with the 64 x 64 of run_base_model's smoke-out expand() replaced by the field size."""
    orig = torch.Tensor.expand

    def expand(self, *sizes):
        if len(sizes) == 5 and tuple(sizes[-2:]) == (64, 64) and tuple(self.shape[-3:]) == (1, 1, 1):
            sizes = tuple(sizes[:-2]) + (ori[1], ori[2])
        return orig(self, *sizes)
    torch.Tensor.expand = expand
    try:
        return ppl.run_model(state)
    finally:
        torch.Tensor.expand = orig


def _multi_evaluate():
    """InferencePipeline.multi_evaluate with the label list its prints read assigned at the top of the body (see the module docstring)."""
    import textwrap
    src = textwrap.dedent(inspect.getsource(INF.InferencePipeline.multi_evaluate))
    q = src.index("'''", src.index("'''") + 3) + 3           # the end of the docstring
    src = src[:q] + "\n    message = ['as sampled']" + src[q:]
    ns = {}
    exec(compile(src, 'multi_evaluate', 'exec'), INF.__dict__, ns)
    return ns['multi_evaluate']


def _solver_out(name):
    v = SI.score_data_control(name)                                  # [B, to, 6, ho, wo]
    b, to, _, ho, wo = v.shape
    ti = 256 // to
    view = np.broadcast_to(v[:, :, None, :, :, None, :, None], (b, to, ti, 6, ho, 2, wo, 2))
    return view.reshape(b, 256, 6, 2 * ho, 2 * wo)


def main():
    files, manifest = {}, {'w_energy': SI.W_ENERGY, 'cases': {}}
    tmp = tempfile.mkdtemp(prefix='wdno_inf_')
    for name, (tshape, shape, ori, cc, seed) in SI.CASES.items():
        d = files.setdefault(SI.FILE_OF[name], {})
        (tc, hc, wc), (to, ho, wo) = shape, ori
        state = SI.batch_state(name)
        ppl, model = _pipeline(name, torch.float32, tmp)
        pred = _run_model(ppl, state, ori).detach()
        init, control = model.kw['init'], model.kw['control']
        assert tuple(init.shape) == (tshape[0], 24, 40, 40) and tuple(control.shape) == (tshape[0], 24, 16, 40, 40)
        assert torch.equal(model.kw['init_u'], SI.base_state(name)[:, 0, 0])
        d[f'{name}::init'] = init[:, list(SI.INIT_FRAMES), :hc, :wc].numpy().copy()
        d[f'{name}::control'] = control[:, :tc, :, :hc:SI.CONTROL_ROWS, :wc].numpy().copy()
        io, co = init.clone(), control.clone()
        io[:, :, :hc, :wc] = 0
        co[:, :tc, :, :hc, :wc] = 0
        d[f'{name}::cond_rest_absmax'] = np.array([float(io.abs().max()), float(co.abs().max())])
        ppl64, _ = _pipeline(name, torch.float64, tmp)
        exact = _run_model(ppl64, state.double(), ori).detach().numpy()
        assert pred.dtype == torch.float32 and tuple(pred.shape) == (tshape[0], to, 6, ho, wo) and exact.dtype == np.float64
        diff = pred.double().numpy() - exact
        fr = SI.PRED_FRAMES(to)
        d[f'{name}::pred04'] = pred[:, fr, :5, ::SI.PRED_ROWS].numpy().copy()
        d[f'{name}::diff04'] = diff[:, fr, :5, ::SI.PRED_ROWS].copy()
        assert float(np.abs(exact[:, :, 5] - exact[:, :, 5, :1, :1]).max()) == 0.0
        d[f'{name}::pred5'] = pred[:, :, 5, 0, 0].numpy().copy()
        d[f'{name}::diff5'] = diff[:, :, 5, 0, 0].copy()
        # the reference's own fp32 error over the whole tensor: [max|err| over channels 0..4, max|exact| there, the same for channel 5]
        d[f'{name}::ref_err'] = np.array([np.abs(diff[:, :, :5]).max(), np.abs(exact[:, :, :5]).max(), np.abs(diff[:, :, 5]).max(), np.abs(exact[:, :, 5]).max()])
        mine = SI.exact_pred(*SI.sample_output(name), shape, ori, 20)
        assert np.abs(mine - exact).max() < 1e-12 * max(1.0, np.abs(exact).max()), np.abs(mine - exact).max()      # the tests' rebuild
        # (c) metrics
        sp = SI.score_pred(name)
        if cc:
            data = SI.score_data_sim(name)
        else:
            data = state
            so = _solver_out(name)
            ppl.multi_evaluate_control = lambda pred, data, plot=False: so
        out = _multi_evaluate()(ppl, sp.clone(), data, plot=False)
        for key, arr in zip(('J_total', 'J_target', 'J_energy', 'mse', 'n_l2'), out):
            assert arr.shape == (1,)
            d[f'{name}::{key}'] = np.asarray(arr)
        manifest['cases'][name] = dict(state=list(tshape), shape=list(shape), ori_shape=list(ori), is_condition_control=cc, file=SI.FILE_OF[name],
                                       metric_dtype=str(np.asarray(out[3]).dtype))
        print(name, 'ref err 0..4', d[f'{name}::ref_err'][0] / d[f'{name}::ref_err'][1], 'ch5', d[f'{name}::ref_err'][2] / d[f'{name}::ref_err'][3],
              {k: float(d[f'{name}::{k}'][0]) for k in ('J_total', 'J_target', 'J_energy', 'mse', 'n_l2')})
    P = INF.InferencePipeline
    manifest['signatures'] = {n: list(inspect.signature(f).parameters) for n, f in (
        ('guidance_fn', INF.guidance_fn), ('load_model', INF.load_model), ('inference', INF.inference), ('main', INF.main),
        ('InferencePipeline.__init__', P.__init__), ('InferencePipeline.run_base_model', P.run_base_model),
        ('InferencePipeline.run_super_model', P.run_super_model), ('InferencePipeline.run_model', P.run_model), ('InferencePipeline.run', P.run),
        ('InferencePipeline.save_results', P.save_results), ('InferencePipeline.per_evaluate', P.per_evaluate),
        ('InferencePipeline.multi_evaluate_control', P.multi_evaluate_control), ('InferencePipeline.multi_evaluate', P.multi_evaluate))}
    for fname, d in files.items():
        out = os.path.join(HERE, fname)
        np.savez_compressed(out, **d)
        print('wrote', out, os.path.getsize(out))
        assert os.path.getsize(out) < 2 ** 20
    with open(os.path.join(HERE, 'ref_smoke_inference_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
