"""Golden vectors for the Burgers data-set generator: make_data_varying_f (burgers/ddpm_burgers/generate_burgers.py:207-275), the shuffle of
generate_data_burgers_equation (l.355-356) and the script's argument parser (l.409-450), by importing / reading the reference.

Build-container only (needs /root/reference):   python tests/golden/make_ref_burgers_datagen_golden.py
Writes tests/golden/ref_burgers_datagen.npz and ref_burgers_datagen_manifest.json -- data only:
  a{0,1}/u0, a{0,1}/f    two consecutive make_data_varying_f(4, 4, s=120, t=80, 'cpu') calls after torch.manual_seed(SEED)
  c{0,1}/u0, c{0,1}/f    the same two calls with alpha = ALPHA, at which the clamp at +-10 is active in the stored f (asserted here)
  odd/u0, odd/f          one call at an odd size, make_data_varying_f(3, 3, s=37, t=13, 'cpu'), after torch.manual_seed(SEED + 1)
  shuffle40              random.sample(range(40), 40) after random.seed(SEED)
The manifest holds the seed, alpha, the sizes and the reference parser's argument names and defaults (read from the script's text with
`ast`: the parser lives under `if __name__ == "__main__"` and cannot be imported).
"""
import ast
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_golden as M  # noqa: E402

M.install_stubs()
from ddpm_burgers import generate_burgers as G  # noqa: E402

SEED = 20260
ALPHA = 4.0


def parser_defaults():
    """{'--name': repr(default)} of every parser.add_argument(...) of the reference script, in its order."""
    with open(G.__file__) as f:
        tree = ast.parse(f.read())
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'add_argument':
            name = ast.literal_eval(node.args[0])
            default = [ast.literal_eval(k.value) for k in node.keywords if k.arg == 'default']
            typ = [ast.unparse(k.value) for k in node.keywords if k.arg == 'type']
            out[name] = dict(default=repr(default[0]) if default else None, type=typ[0] if typ else None)
    return out


def main():
    g = {}
    for tag, alpha in (('a', 1.), ('c', ALPHA)):
        torch.manual_seed(SEED)
        for i in range(2):
            u0, f = G.make_data_varying_f(4, 4, s=120, t=80, device='cpu', alpha=alpha)
            assert u0.dtype == torch.float32 and f.dtype == torch.float32 and tuple(f.shape) == (4, 80, 120)
            g[f'{tag}{i}/u0'], g[f'{tag}{i}/f'] = u0.numpy(), f.numpy()
            if tag == 'c':
                hit = int((f.abs() == 10.).sum())
                assert hit > 0 and f.abs().max() == 10., (i, hit)
                assert hit < f.numel() // 2                      # and it is not all clamp
                print(f'c{i}: {hit} of {f.numel()} values at the clamp', flush=True)
    assert np.array_equal(g['a0/u0'], g['c0/u0']) and not np.array_equal(g['a0/f'], g['c0/f'])
    torch.manual_seed(SEED + 1)
    u0, f = G.make_data_varying_f(3, 3, s=37, t=13, device='cpu')
    g['odd/u0'], g['odd/f'] = u0.numpy(), f.numpy()
    random.seed(SEED)
    g['shuffle40'] = np.array(random.sample(range(40), 40), np.int64)
    np.savez_compressed(os.path.join(HERE, 'ref_burgers_datagen.npz'), **g)
    manifest = dict(seed=SEED, alpha=ALPHA, sizes=dict(a=[4, 120, 80], c=[4, 120, 80], odd=[3, 37, 13]), odd_seed=SEED + 1,
                    parser=parser_defaults())
    with open(os.path.join(HERE, 'ref_burgers_datagen_manifest.json'), 'w') as fh:
        json.dump(manifest, fh, indent=1)
    for fn in ('ref_burgers_datagen.npz', 'ref_burgers_datagen_manifest.json'):
        print(fn, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == '__main__':
    main()
