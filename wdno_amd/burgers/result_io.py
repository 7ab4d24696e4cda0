"""MI355X restatement of burgers/ddpm_burgers/result_io.py: the YAML result table of the evaluation drivers.

It is the top-level module `result_io` of this tree -- the name the reference's test_util imports it by (test_util.py:18) -- and what
eval_ddpm_burgers.py here imports. `ddpm_burgers.result_io` itself is left to the reference's package when that is on sys.path behind this
tree (tests/test_host.py pins that fall-through), so nothing that resolved there before resolves differently now.

data_merge, merge_save_dict and save_acc keep the reference's contract: nested dictionaries are merged key by key, lists are extended or
appended to, a primitive (or nothing) is replaced; the file and its directory are created when missing; save_acc stores the mean and the
standard deviation of an array as python floats under the path make_dict_path builds. yaml is imported inside the functions, so the
module loads without it. Every other name of the reference module comes from there when the reference is on sys.path behind this tree."""
import os
from pathlib import Path

import numpy as np

import wdno_amd

_reference_getattr = wdno_amd.reference_fallthrough('ddpm_burgers.result_io', __file__)


class YamlReaderError(Exception):
    pass


def data_merge(a, b):
    """Merge b into a and return the result; a is modified when it is a list or a dictionary."""
    if a is None or isinstance(a, (str, int, float)):
        return b
    if isinstance(a, list):
        if isinstance(b, list):
            a.extend(b)
        else:
            a.append(b)
        return a
    if isinstance(a, dict):
        if not isinstance(b, dict):
            raise YamlReaderError(f'Cannot merge non-dict "{b}" into dict "{a}"')
        for key in b:
            a[key] = data_merge(a[key], b[key]) if key in a else b[key]
        return a
    raise YamlReaderError(f'NOT IMPLEMENTED "{b}" into "{a}"')


def merge_save_dict(fname, new_res):
    """Merge new_res into the YAML file fname (created, with its directory, when it does not exist)."""
    import yaml
    directory = os.path.dirname(fname)
    if directory:
        Path(directory).mkdir(parents=True, exist_ok=True)
    res = None
    if os.path.exists(fname):
        with open(fname, 'r') as fh:
            res = yaml.safe_load(fh)
    res = data_merge(res, new_res)
    with open(fname, 'w') as fh:
        yaml.dump(res, fh)


def save_acc(acc, fname, make_dict_path=lambda acc_dict, dict_args: {dict_args['model_name']: {'result': acc_dict}}, **dict_path_args):
    """{'mean', 'std'} of acc as python floats, placed by make_dict_path(acc_dict, dict_path_args) and merged into fname."""
    merge_save_dict(fname, make_dict_path({'mean': float(np.mean(acc)), 'std': float(np.std(acc))}, dict_path_args))


def __getattr__(name):          # save_edge_flip, rep_save_model, ... of the reference module
    return _reference_getattr(name)
