"""Host-side checks of the Burgers evaluation driver (wdno_amd/burgers/eval_ddpm_burgers.py, reconstruct.py: plan, score.py: formulas,
result_io.py, ddpm_burgers/test_util.py) against what the reference's own run recorded (tests/golden/ref_burgers_eval.npz and its
manifest). No GPU and no built library needed."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import burgers_eval_inputs as EI, burgers_eval_ref as ER
from tests.helpers import GOLDEN, load_npz

with open(os.path.join(GOLDEN, 'ref_burgers_eval_manifest.json')) as _f:
    MAN = json.load(_f)
OUT = ('ddpm_mse', 'J_diffused', 'J_actual', 'energy', 'total_J')


@pytest.fixture(scope='module')
def trees():
    from wdno_amd import tree_path
    for t in ('third_party', 'burgers'):
        p = tree_path(t)
        if p not in sys.path:
            sys.path.insert(0, p)
    import eval_ddpm_burgers as E
    import result_io as IO
    from ddpm_burgers import test_util as TU
    from wdno_amd.burgers import reconstruct as Rc, score as Sc
    assert os.path.abspath(E.__file__).startswith(os.path.abspath(os.path.join(os.path.dirname(__file__), '..', 'wdno_amd', 'burgers')))
    return dict(E=E, IO=IO, TU=TU, Rc=Rc, Sc=Sc)


@pytest.fixture(scope='module')
def gold():
    return load_npz('ref_burgers_eval.npz')


# ------------------------------------------------------------------------------------------------ plan()
def test_plan_integers_tile_rule_and_lds(trees):
    Rc = trees['Rc']
    pl = Rc.plan((50, 9, 64, 64), (41, 60), (81, 120))
    assert (pl['B'], pl['C'], pl['H'], pl['W'], pl['h'], pl['w'], pl['n_t'], pl['n_x'], pl['L'], pl['mode']) == (50, 9, 64, 64, 41, 60, 81, 120, 10, 0)
    assert (pl['sample_stride'], pl['chan_stride'], pl['row_stride']) == (9 * 64 * 64, 64 * 64, 64)
    assert (pl['tn'], pl['ntile'], pl['lds_bytes']) == (28, 3, 8 * 28 * 60) and pl['lds_bytes'] <= 64 * 1024
    for (xs, sh, ori) in (((3, 8, 16, 24), (9, 12), (17, 24)), ((1, 8, 12, 20), (7, 9), (13, 17)), ((2, 8, 64, 64), (32, 60), (64, 120)),
                          ((1, 8, 40, 40), (17, 20), (33, 40))):
        p = Rc.plan(xs, sh, ori)
        assert p['tn'] % 2 == 0 and 2 <= p['tn'] <= Rc.TILE_MAX and (p['ntile'] - 1) * p['tn'] < p['n_t'] <= p['ntile'] * p['tn']
        assert p['lds_bytes'] == Rc.lds_bytes(p['w'], p['tn']) <= 64 * 1024
    # a strided view: channel stride 2 planes, rows of a wider tensor
    p = Rc.plan((2, 8, 16, 24), (9, 12), (17, 24), strides=(16 * 16 * 30, 2 * 16 * 30, 30, 1))
    assert (p['sample_stride'], p['chan_stride'], p['row_stride']) == (16 * 16 * 30, 2 * 16 * 30, 30)
    # a block so wide that 32 rows do not fit: the tile shrinks
    p = Rc.plan((1, 8, 64, 600), (40, 512), (80, 1024))
    assert p['lds_bytes'] <= 64 * 1024 and p['tn'] == 16


@pytest.mark.parametrize('kw', [
    dict(wave_type='bior1.3'), dict(pad_mode='zero'), dict(x_shape=(2, 7, 64, 64)), dict(shape=(65, 60)), dict(shape=(41, 65)),
    dict(ori_shape=(83, 120)), dict(ori_shape=(81, 121)), dict(ori_shape=(1, 120)), dict(shape=(4, 60), ori_shape=(8, 120)),
    dict(strides=(9 * 64 * 64, 64 * 64, 63, 1)), dict(strides=(9 * 64 * 64, 64 * 64, 64, 2)), dict(strides=(8 * 64 * 64, 64 * 64, 64, 1)),
    dict(x_shape=(70000, 9, 64, 64))])
def test_plan_refuses(trees, kw):
    base = dict(x_shape=(2, 9, 64, 64), shape=(41, 60), ori_shape=(81, 120))
    base.update(kw)
    with pytest.raises(ValueError):
        trees['Rc'].plan(**base)


def test_solver_downsampling_identity():
    """The evaluation's solver call with output_space_downsample=True keeps every 16th of the 1920 grid points: the reference's [:, :, ::16]."""
    from wdno_amd import burgers_solver
    pl = burgers_solver.plan((50, 120), (50, 80, 120), 8.0, num_t=80, output_space_downsample=True)
    assert pl['sub_s'] == 16 == 2 ** 4 and pl['out_cols'] == 120 and pl['steps'] == 614400


# ------------------------------------------------------------------------------------------------ the fp64 evaluation against the reference's fp64 run
@pytest.mark.parametrize('name', ['full', 'small'])
def test_eval_ref_is_pinned_to_the_reference_fp64_run(gold, name):
    c = MAN['cases'][name]
    x, resc, ut = EI.case_input(name)
    u, f = ER.reconstruct(x, resc, c['shape'], c['ori'])
    assert u.shape == (x.shape[0], c['ori'][0], c['ori'][1]) and f.shape == (x.shape[0], c['ori'][0] - 1, c['ori'][1])
    assert np.abs(u[:, ::5, ::7] - gold[f'{name}::u64_sub']).max() < 1e-12 and np.abs(f[:, ::5, ::7] - gold[f'{name}::f64_sub']).max() < 1e-12
    assert abs(np.abs(u).max() - c['max_u']) < 1e-12 and abs(np.abs(f).max() - c['max_f']) < 1e-12
    # the reference's fp32 fields are within their recorded error of it, and that error is fp32 rounding
    assert abs(np.abs(gold[f'{name}::u'] - u).max() - c['err_u']) < 1e-12 and c['err_u'] < 1e-6 * max(1.0, c['max_u'])
    assert abs(np.abs(gold[f'{name}::f'] - f).max() - c['err_f']) < 1e-12 and c['err_f'] < 1e-6 * max(1.0, c['max_f'])
    got = ER.evaluate(gold[f'{name}::u'], gold[f'{name}::f'], gold[f'{name}::x_gt'], ut, MAN['wf'])
    for k, v in zip(OUT, got):
        assert v.shape == gold[f'{name}::{k}64'].shape and np.abs(v - gold[f'{name}::{k}64']).max() <= 1e-12 * max(1.0, np.abs(v).max()), k


def test_eval_ref_sub2_is_pinned(gold):
    u, f, x_gt, ut = EI.sub2_input()
    for k, v in zip(OUT, ER.evaluate(u, f, x_gt, ut, MAN['wf'])):
        assert np.abs(v - gold[f'sub2::{k}64']).max() <= 1e-12 * max(1.0, np.abs(v).max()), k
        assert np.abs(gold[f'sub2::{k}'] - gold[f'sub2::{k}64']).max() <= 1e-5 * np.abs(v).max(), k      # the fp32 run is the same quantity


# ------------------------------------------------------------------------------------------------ score's host formulas
def test_score_formulas_on_hand_made_sums(trees):
    Sc = trees['Sc']
    n_t, n_x, sub, wf = 5, 4, 2, 0.25
    s = np.array([[32.0, 8.0, 18.0, 12.0, 2.25, 1.5, 4.0, 8.0, 4.0, 1.0, 1.0, 6.0, 32.0, 16.0],
                  [16.0, 4.0, 2.0, 4.0, 0.25, 0.5, 16.0, 32.0, 8.0, 4.0, 2.0, 10.0, 32.0, 16.0]])
    ddpm, jd, ja, en, tj = Sc.formulas(s, n_t, n_x, sub, wf, upsample_t=1)
    assert np.array_equal(ddpm, [2.0, 1.0])
    nm, na = np.sqrt(64.0 / 16) + 1e-5, np.sqrt(32.0 / 16) + 1e-5          # the batch-wide normalisers: sqrt(mean t^2), sqrt(mean |t|)
    assert np.allclose(jd, [[2.0, 1.0], [2.25, 0.25], [1.5, 0.5], [1.5, 0.5], [1.5 / nm, 0.5 / nm], [np.sqrt(1.5) / na, np.sqrt(0.5) / na]], rtol=1e-15)
    assert np.allclose(ja, [[1.0, 4.0], [1.0, 4.0], [0.5, 1.0], [1.0, 2.0], [1.0 / nm, 2.0 / nm], [np.sqrt(0.5) / na, 1.0 / na]], rtol=1e-15)
    assert np.array_equal(en, [1.5, 2.5]) and np.array_equal(tj, [1.0 + 0.25 * 1.5, 4.0 + 0.25 * 2.5])
    assert jd.dtype == ja.dtype == en.dtype == np.float64 and jd.shape == (6, 2)
    # report_all=False: mse only; is_condition_f: J_actual is J_diffused
    _, jd1, ja1, _, tj1 = Sc.formulas(s, n_t, n_x, sub, wf, report_all=False)
    assert np.array_equal(jd1, [2.0, 1.0]) and np.array_equal(ja1, [1.0, 4.0]) and np.array_equal(tj1, [1.0 + 0.25 * 6, 4.0 + 0.25 * 10])
    _, jd2, ja2, _, tj2 = Sc.formulas(s, n_t, n_x, sub, wf, actual_is_diffused=True)
    assert np.array_equal(jd2, ja2) and np.array_equal(tj2, [2.0 + 0.25 * 6, 1.0 + 0.25 * 10])
    # a sample's nmse depends on its batch by definition: alone, sample 0 is normalised by its own t
    s2 = s.copy()
    s2[1, 12] = 96.0
    assert Sc.formulas(s2, n_t, n_x, sub, wf)[1][4, 0] != jd[4, 0] and Sc.formulas(s2[:1], n_t, n_x, sub, wf)[1][4, 0] == jd[4, 0]
    assert Sc.COLUMNS == ER.COLUMNS and len(Sc.COLUMNS) == 14


def test_formulas_reproduce_the_reference_from_exact_sums(trees, gold):
    """formulas(sums) is the reference's metric: on the fixture's fp32 fields it meets the reference's fp64 run."""
    for name in ('full', 'small'):
        _, _, ut = EI.case_input(name)
        u, f, x_gt = (gold[f'{name}::{k}'] for k in ('u', 'f', 'x_gt'))
        got = trees['Sc'].formulas(ER.sums(u, f, x_gt, ut), u.shape[1], u.shape[2], 1, MAN['wf'])
        for k, v in zip(OUT, got):
            assert np.abs(v - gold[f'{name}::{k}64']).max() <= 1e-12 * max(1.0, np.abs(v).max()), (name, k)
    u, f, x_gt, ut = EI.sub2_input()
    for k, v in zip(OUT, trees['Sc'].formulas(ER.sums(u, f, x_gt, ut), 17, 24, 2, MAN['wf'])):
        assert np.abs(v - gold[f'sub2::{k}64']).max() <= 1e-12 * max(1.0, np.abs(v).max()), k


def test_lower_median_rule(trees):
    """torch.median returns the element of rank (n - 1) // 2: the lower middle of an even row, the middle of an odd one."""
    Sc = trees['Sc']
    even, odd = torch.tensor([4.0, 1.0, 3.0, 2.0]), torch.tensor([5.0, 1.0, 4.0, 2.0, 3.0])
    for row, want in ((even, 2.0), (odd, 3.0)):
        assert row.median(-1)[0].item() == want == row.sort()[0][Sc.lower_median_rank(row.numel())].item()
        assert ER.lower_median(row.numpy()) == want


# ------------------------------------------------------------------------------------------------ the drop-in modules
def test_parser_has_the_reference_options_and_defaults(trees):
    E = trees['E']
    ours = {a.option_strings[0]: a for a in E.build_parser()._actions if a.option_strings and a.option_strings[0] != '-h'}
    assert list(ours) == [o['option'] for o in MAN['parser']] and len(ours) == 35
    for o in MAN['parser']:
        a = ours[o['option']]
        assert a.default == o['default'] and a.nargs == o['nargs'] and getattr(a.type, '__name__', None) == o['type'], o['option']
    ns = E.build_parser().parse_args(['--exp_id', 'm', '--wus', '0.5', '1', '--is_condition_u0', 'True'])
    assert ns.wus == [0.5, 1.0] and ns.is_condition_u0 is True and ns.wfs == [0] and ns.batch_size == 50
    assert E.rescaler_table(ns).flatten().tolist() == [10, 3, 3, 1, 21, 5, 5, 1, 10]
    with pytest.raises(ValueError):
        E.rescaler_table(types.SimpleNamespace(is_wavelet=True, pad_mode='zero', wave_type='bior2.4', is_super_model=False))


def test_result_io_round_trip(trees, tmp_path):
    yaml = pytest.importorskip('yaml')
    IO = trees['IO']
    assert IO.data_merge(None, {'a': 1}) == {'a': 1} and IO.data_merge(3, 4) == 4 and IO.data_merge([1], [2, 3]) == [1, 2, 3] and IO.data_merge([1], 2) == [1, 2]
    assert IO.data_merge({'a': {'b': 1}, 'l': [1]}, {'a': {'c': 2}, 'l': [2], 'd': 5}) == {'a': {'b': 1, 'c': 2}, 'l': [1, 2], 'd': 5}
    with pytest.raises(IO.YamlReaderError):
        IO.data_merge({'a': 1}, 3)
    fname = str(tmp_path / 'deep' / 'er' / 'result.yaml')                  # neither the file nor its directory exists yet
    IO.save_acc(np.array([1.0, 2.0, 3.0], dtype=np.float32), fname, model_name='m')
    IO.save_acc(np.array([2.0, 4.0]), fname, make_dict_path=lambda acc, a: {a['model_name']: {a['g']: {'J': acc}}}, model_name='m', g='wu=1.0, wf=0.0')
    with open(fname) as fh:
        text = fh.read()
    res = yaml.safe_load(text)
    assert res == {'m': {'result': {'mean': 2.0, 'std': float(np.std(np.array([1.0, 2.0, 3.0], dtype=np.float32)))}, 'wu=1.0, wf=0.0': {'J': {'mean': 3.0, 'std': 1.0}}}}
    assert type(res['m']['result']['mean']) is float and 'numpy' not in text
    # save_eval_results: the 15 names of a resolution
    E = trees['E']
    fname2 = str(tmp_path / 'table.yaml')
    E.save_eval_results([[np.full(3, float(i)) for i in range(15)]], 'model', fname2, model_str='d', wu=0.5, wf=1.5)
    with open(fname2) as fh:
        table = yaml.safe_load(fh)['model']
    assert sorted(table) == ['model_description', 'wu=0.5, wf=1.5'] and table['model_description'] == 'd'
    entries = table['wu=0.5, wf=1.5']
    assert sorted(entries) == sorted(E.result_names(0)) and len(entries) == 15 and entries['totalJ_0_'] == {'mean': 14.0, 'std': 0.0}


def test_out_of_scope_raises_not_implemented(trees):
    E, TU = trees['E'], trees['TU']
    args = types.SimpleNamespace(is_wavelet=True, is_super_model=False, wave_type='bior2.4', pad_mode='periodization', upsample_x=0, is_condition_f=False)
    ddpm = types.SimpleNamespace(is_wavelet=True, padded_shape=[41, 60], ori_shape=[81, 120], is_condition_f=False)
    cases = [
        lambda: E.evaluate('m', '', types.SimpleNamespace(**{**vars(args), 'is_super_model': True})),
        lambda: E.evaluate('m', '', types.SimpleNamespace(**{**vars(args), 'is_wavelet': False})),
        lambda: E.diffuse_2dconv(ddpm, args, None, N_upsample=1, low=None),
        lambda: E.diffuse_2dconv(ddpm, types.SimpleNamespace(**{**vars(args), 'is_super_model': True, 'is_condition_f': True}), None),
        lambda: E.diffuse_2dconv(types.SimpleNamespace(**{**vars(ddpm), 'is_wavelet': False}), args, None),
        lambda: E.get_loss_fn_2dconv(types.SimpleNamespace(**{**vars(args), 'is_wavelet': False}), [41, 60], [81, 120], 1),
        lambda: E.get_nablaJ_2dconv(args=types.SimpleNamespace(**{**vars(args), 'is_wavelet': False}), shape=[41, 60], ori_shape=[81, 120], RESCALER=1),
        lambda: TU.load_2dconv_super_model('m', args, 1),
    ]
    for fn in cases:
        with pytest.raises(NotImplementedError, match=r'reference burgers/'):
            fn()


def test_generic_metric_is_the_reference_metric(trees, gold):
    """test_util.metric / mse_deviation (plain torch, CPU here) on the fixture's fields give the reference's fp32 arrays (to fp32 summation order; the medians exactly)."""
    TU = trees['TU']
    for name in ('full', 'small'):
        _, _, ut = EI.case_input(name)
        u, f, x_gt = (torch.from_numpy(gold[f'{name}::{k}']) for k in ('u', 'f', 'x_gt'))
        jd, _, _ = TU.metric(ut, f, 0, wf=MAN['wf'], report_all=True, u=u, evaluate=True)
        ja, en, tj = TU.metric(ut, f, 0, wf=MAN['wf'], report_all=True, u=x_gt, evaluate=True)
        assert isinstance(ja, tuple) and len(ja) == 6 and all(v.dtype == torch.float32 and v.shape == (u.shape[0],) for v in ja)
        got = (TU.mse_deviation(u[:, 1:], x_gt[:, 1:]).numpy(), np.array([v.numpy() for v in jd]), np.array([v.numpy() for v in ja]), en.numpy(), tj.numpy())
        for k, v in zip(OUT, got):                 # fp32 sums of up to 9 600 terms: the order of a CPU's reduction may differ from the fixture's
            assert v.dtype == np.float32 and np.abs(v - gold[f'{name}::{k}']).max() <= 1e-5 * np.abs(gold[f'{name}::{k}']).max(), (name, k)
        for j in (1, 2):                           # the medians are single roundings, no sum: equal bits
            assert np.array_equal(got[j][[1, 3]], gold[f'{name}::{OUT[j]}'][[1, 3]]), (name, j)
    assert TU.metric(ut, f, 0, wf=0.5, u=x_gt, evaluate=True)[0].shape == (u.shape[0],)          # report_all=False: the mse alone
    assert TU.SOLVER_N_UPSAMPLE == 4
