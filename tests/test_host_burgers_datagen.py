"""Host side of the Burgers data-set generator (wdno_amd.burgers_datagen): the draws and the separable forcing against the reference's
make_data_varying_f (bit for bit, on the CPU), plan(), the shuffle and the files, the command line. No GPU, no library."""
import json
import os
import random

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN

with open(os.path.join(GOLDEN, 'ref_burgers_datagen_manifest.json')) as _f:
    M = json.load(_f)
_G = None


def _golden(key):
    global _G
    if _G is None:
        _G = np.load(os.path.join(GOLDEN, 'ref_burgers_datagen.npz'))
    return torch.from_numpy(_G[key])


@pytest.mark.parametrize('tag', ['a', 'c'])
def test_draws_reproduce_reference_two_batches(tag):
    """After torch.manual_seed(S), two consecutive draw(4, 120, 80, 'cpu') give the u0 and (through dense_forcing) the f of two consecutive
    make_data_varying_f calls, bit for bit; 'c' with the alpha at which the clamp is active."""
    from wdno_amd.burgers_datagen import dense_forcing, draw
    alpha = 1. if tag == 'a' else M['alpha']
    N, s, t = M['sizes'][tag]
    torch.manual_seed(M['seed'])
    for i in range(2):
        u0, AX, TT = draw(N, s, t, 'cpu')
        assert AX.shape == (N, 8, s) and TT.shape == (N, t, 8) and AX.dtype == TT.dtype == u0.dtype == torch.float32
        assert torch.equal(u0, _golden(f'{tag}{i}/u0')), (tag, i)
        f = dense_forcing(AX, TT, alpha)
        assert f.shape == (N, t, s) and torch.equal(f, _golden(f'{tag}{i}/f')), (tag, i)
    if tag == 'c':
        assert (f.abs() == 10.).any()


def test_draws_reproduce_reference_odd_size():
    from wdno_amd.burgers_datagen import dense_forcing, draw
    N, s, t = M['sizes']['odd']
    torch.manual_seed(M['odd_seed'])
    u0, AX, TT = draw(N, s, t, 'cpu')
    assert torch.equal(u0, _golden('odd/u0')) and torch.equal(dense_forcing(AX, TT), _golden('odd/f'))


@pytest.mark.parametrize('s, t, nx, nt, T, want', [
    (1920, 1280, 120, 80, 8, dict(sx=16, st=16, u_shape=(5, 81, 120), f_shape=(5, 80, 120))),
    (1920, 1280, 128, 10, 1., dict(sx=15, st=128, u_shape=(5, 11, 128), f_shape=(5, 10, 128))),      # the parser's defaults
    (333, 6, 100, 3, 0.01, dict(sx=3, st=2, u_shape=(5, 4, 111), f_shape=(5, 3, 111))),
])
def test_plan_strides_and_record_shapes(s, t, nx, nt, T, want):
    from wdno_amd import burgers_datagen as D, burgers_solver as B
    p = D.plan(5, s, t, T, nt, nx, nt)
    assert {k: p[k] for k in want} == want
    steps = round(T * 76800)
    assert p['steps'] == steps and p['f_time'] == steps // t and p['record_time'] == steps // nt
    assert (p['waves'], p['points']) in B.configs(s)
    q = B.plan((5, s), (5, t, s), T, num_t=nt, s=s)                   # the solver's integers and constants, unchanged
    assert all(p[k] == q[k] for k in ('steps', 'record_time', 'f_time', 'c', 'd', 'dm', 'dt', 'sub_s'))


def test_plan_data_set_shape_and_configuration():
    from wdno_amd import burgers_datagen as D
    p = D.plan(800, 1920, 1280, 8, 80, 120, 80)
    assert (p['steps'], p['f_time'], p['record_time']) == (614400, 480, 7680)
    assert (p['waves'], p['points']) == D.choose_config(800, 1920) and 64 * p['waves'] * p['points'] >= 1920
    assert D.plan(8, 1920, 1280, 8, 80, 120, 80, config=(8, 4))['waves'] == 8
    with pytest.raises(ValueError):
        D.plan(8, 1920, 1280, 8, 80, 120, 80, config=(1, 4))


def test_plan_raises_reference_errors():
    from wdno_amd.burgers_datagen import plan
    with pytest.raises(ValueError, match='slice step cannot be zero'):
        plan(4, 120, 24, 0.01, 4, 50, 48)                                 # nt > t: f[:, ::0]
    with pytest.raises(ValueError, match='slice step cannot be zero'):
        plan(4, 120, 24, 0.01, 4, 121, 4)                                 # nx > s
    with pytest.raises(IndexError):
        plan(4, 120, 7, 0.01, 4, 50, 4)                                   # 768 steps, t = 7: f index 7 of 7
    with pytest.raises(ZeroDivisionError):
        plan(4, 120, 1000, 0.01, 4, 50, 4)                                # f_time = 0
    with pytest.raises(ZeroDivisionError):
        plan(4, 120, 24, 0.01, 0, 50, 4)                                  # num_t = 0


def test_shuffle_split_is_the_reference_shuffle():
    from wdno_amd.burgers_datagen import shuffle_split
    random.seed(M['seed'])
    train, test = shuffle_split(40, 30)
    assert train + test == _golden('shuffle40').tolist() and len(train) == 30


def test_write_dataset_files(tmp_path, monkeypatch):
    """With generate() replaced by a CPU stub: two files of fp32 'u' [n, nt + 1, nx] and 'f' [n, nt, nx] with the counts asked for, the
    reference's shuffle applied to the batches in order, and FileExistsError on a second call."""
    from wdno_amd import burgers_datagen as D
    calls = []

    def stub(u0, AX, TT, T, num_t, nx, nt, alpha=1., visc=0.01, dt=D.DT, config=None):
        p = D.plan(u0.shape[0], u0.shape[1], TT.shape[1], T, num_t, nx, nt)
        f = D.dense_forcing(AX, TT, alpha)[:, ::p['st'], ::p['sx']]
        u = torch.zeros(p['u_shape'])
        u[:, 0] = u0[:, ::p['sx']]
        u[:, 1:] = len(calls) + 1
        calls.append((u.clone(), f.clone()))
        return u, f
    monkeypatch.setattr(D, 'generate', stub)
    save = str(tmp_path / 'd') + os.sep
    n = D.write_dataset(save, 30, 10, batch_size=8, end_time=0.01, nt=4, nx=10, alpha=1., seed=M['seed'], s=40, t=8, device='cpu')
    assert n == (30, 10) and len(calls) == 5
    tr, te = torch.load(save + 'train'), torch.load(save + 'test')
    for d, cnt in ((tr, 30), (te, 10)):
        assert sorted(d) == ['f', 'u']
        assert d['u'].shape == (cnt, 5, 10) and d['f'].shape == (cnt, 4, 10)
        assert d['u'].dtype == d['f'].dtype == torch.float32 and d['u'].device.type == 'cpu'
    order = _golden('shuffle40')
    u_all, f_all = torch.cat([c[0] for c in calls]), torch.cat([c[1] for c in calls])
    assert torch.equal(torch.cat([tr['u'], te['u']]), u_all[order]) and torch.equal(torch.cat([tr['f'], te['f']]), f_all[order])
    torch.manual_seed(M['seed'])                                           # the first batch is the first draw after the seed
    assert torch.equal(calls[0][0][:, 0], D.draw(8, 40, 8, 'cpu')[0][:, ::4])
    with pytest.raises(FileExistsError):
        D.write_dataset(save, 30, 10, batch_size=8, end_time=0.01, nt=4, nx=10, alpha=1., seed=M['seed'], s=40, t=8, device='cpu')
    assert len(calls) == 5                                                 # refused before anything was generated


def test_parser_matches_reference():
    from wdno_amd.burgers_datagen import main, parser
    ap = parser()
    got = {a.option_strings[0]: a for a in ap._actions if a.option_strings and a.dest != 'help'}
    assert list(got) == list(M['parser'])
    for name, ref in M['parser'].items():
        assert repr(got[name].default) == ref['default'], name
        assert (got[name].type.__name__ if got[name].type else None) == ref['type'], name
    with pytest.raises(NotImplementedError):
        main(['--uniform_u_f', 'True'])


def test_dropin_script_block_leaves_namespace_alone():
    """The drop-in gained a __main__ block only: the names the reference's module defines still fall through to it."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, 'wdno_amd', 'burgers', 'ddpm_burgers', 'generate_burgers.py')
    spec = importlib.util.spec_from_file_location('_dropin_generate_burgers_dg', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    public = {k for k in vars(mod) if not k.startswith('_')}
    assert public == {'wdno_amd', 'burgers_numeric_solve_free'}
    with open(path) as f:
        assert "if __name__ == '__main__':" in f.read()
