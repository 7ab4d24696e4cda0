"""MI355X drop-in for burgers/ddpm_burgers (unet, diffusion_1d, train_diffusion, model_utils, wavelet_utils, test_util, and the
control-evaluation solver `burgers_numeric_solve_free` of generate_burgers).

Modules this package does not provide (result I/O -- this tree's own is the top-level module result_io --, ...) fall through to the reference's package of the same name when
that is also on sys.path, and so do the names generate_burgers does not define (the data-generation routines): put wdno_amd's tree
*before* the reference directory and the drivers run unchanged, with the hot-path modules resolved here."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
