"""Inputs of the Burgers control-objective fixtures (tests/golden/ref_burgers_guidance.npz), regenerated identically by the fixture generator
and by the tests from an integer hash (tests/helpers._hash_values: no random generator, no libm), so only outputs are stored. No product
code here."""
import numpy as np
import torch

from tests.helpers import _hash_values

RESCALER = [10, 3, 3, 1, 21, 5, 5, 1, 10]                    # train_ddpm_burgers.py:234-249 (bior2.4 / periodization, conditioned on u0)
RESCALER_SUPER = RESCALER[:8] * 2 + [10]                     # (is_super_model: the eight values repeated)

# name: tensor shape, coefficient shape (padded_shape), field shape (ori_shape), RESCALER, wu, wf, condition_f, is_super_model
CASES = {
    'full_u': dict(xshape=(2, 9, 64, 64), shape=(41, 60), ori=(81, 120), resc=RESCALER, wu=1.0, wf=0.0, condition_f=False, is_super=False),
    'full_uf': dict(xshape=(2, 9, 64, 64), shape=(41, 60), ori=(81, 120), resc=RESCALER, wu=0.7, wf=0.03, condition_f=False, is_super=False),
    'full_u_cf': dict(xshape=(2, 9, 64, 64), shape=(41, 60), ori=(81, 120), resc=RESCALER, wu=1.0, wf=0.0, condition_f=True, is_super=False),
    'full_uf_cf': dict(xshape=(2, 9, 64, 64), shape=(41, 60), ori=(81, 120), resc=RESCALER, wu=0.7, wf=0.03, condition_f=True, is_super=False),
    'small': dict(xshape=(2, 9, 16, 16), shape=(9, 12), ori=(17, 24), resc=RESCALER, wu=0.7, wf=0.03, condition_f=False, is_super=False),
    'super': dict(xshape=(2, 17, 32, 32), shape=(21, 28), ori=(41, 56), resc=RESCALER_SUPER, wu=0.7, wf=0.03, condition_f=False, is_super=True),
}


def seed_of(name):
    return sum(name.encode())


def burgers_guidance_input(xshape, shape, ori, resc, seed):
    """x [B, C, H, W] in network units (values of fp32, non-zero everywhere: the gradient must ignore what lies outside the coefficient
    block by itself), RESCALER [1, C, 1, 1] and u_target [B, n_t, n_x] in field units, all float32 tensors."""
    b, c, h, w = xshape
    x = 0.6 * _hash_values(b * c * h * w, seed).reshape(b, c, h, w)
    u_target = 2.0 * _hash_values(b * ori[0] * ori[1], seed + 1).reshape(b, ori[0], ori[1])
    r = np.asarray(resc, dtype=np.float64).reshape(1, c, 1, 1)
    return torch.from_numpy(x).float(), torch.from_numpy(r).float(), torch.from_numpy(u_target).float()


def case_input(name):
    c = CASES[name]
    return burgers_guidance_input(c['xshape'], c['shape'], c['ori'], c['resc'], seed_of(name))


# the guided chains (fixture keys 'chain::*'): the tiny U-Net and diffusion settings of the 'gb' chains of ref_round2.npz, whose weights they reuse
CHAIN = dict(shape=(11, 14), ori=(20, 28), xshape=(2, 9, 16, 16), wu=0.5, wf=0.05, condition_f=False, ddpm6_s=0.2)


def chain_input():
    """u_target [2, 20, 28] and u_init [2, 8, 16] (network units) of the guided chains."""
    u_target = torch.from_numpy(2.0 * _hash_values(2 * 20 * 28, 977).reshape(2, 20, 28)).float()
    u_init = torch.from_numpy(0.8 * _hash_values(2 * 8 * 16, 978).reshape(2, 8, 16)).float()
    r = torch.tensor(RESCALER, dtype=torch.float32).reshape(1, 9, 1, 1)
    return u_target, u_init, r
