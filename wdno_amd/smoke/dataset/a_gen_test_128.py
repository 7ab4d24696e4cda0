"""MI355X drop-in for smoke/dataset/a_gen_test_128.py: `exp2_same_side_128` generates its scenes on the GPU (wdno_amd.smoke_datagen,
csrc/smoke_datagen.hip) and writes the reference's files. Same signature, same scene numbers per branch, same command line
(--test_or_train --data_savepath --branch_begin --branch_end), in one process without a multiprocessing.Pool. The data-set seed comes
from `seed=` / --seed (default 0) instead of the process id, so a data set can be generated again. Every other name comes from the
reference's module when that is on sys.path behind this tree."""
import wdno_amd
from wdno_amd import smoke_datagen as _gen

SPLIT = 'test_128'

_reference_getattr = wdno_amd.reference_fallthrough('dataset.a_gen_test_128', __file__)


def exp2_same_side_128(is_train_, fix_velocity_, Test_, branch_num, data_savepath, seed=0):
    return _gen.exp2_same_side_128(SPLIT, is_train_, fix_velocity_, Test_, branch_num, data_savepath, seed=seed)


def __getattr__(name):          # anything else of the reference module
    return _reference_getattr(name)


if __name__ == '__main__':
    _gen.script_main(SPLIT)
