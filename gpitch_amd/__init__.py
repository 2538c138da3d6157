"""gpitch_amd — MI355X-native engine behind the gpitch pdgp / sgpr_ss ELBO path.

Importing the package loads libgpitch_hip.so (the hand-written HIP kernels behind a C-ABI,
include/gpitch_abi.h).  There is no CPU fallback: a missing library raises ImportError here and a
missing gfx950 device raises when the first handle is created.
"""
from . import _lib

_lib.load_library()

from .methods import (logistic, ilogistic, softplus, isoftplus, gaussfun, logistic_tf, softplus_tf,  # noqa: E402
                      gaussfun_tf, midi2freq, freq2midi, norm, find_ideal_f0, readaudio, init_cparam)
from . import param, kernels, matern12_spectral_mixture, likelihoods, conditionals, pdgp, sgpr_ss, synth, train  # noqa: E402,F401
from . import samplecov, kernelfit, pdgp_batch  # noqa: E402,F401
from .pdgp_batch import optimize_many, predict_many, predict_sources_many, PdgpBatch  # noqa: E402,F401
from .pdgp_batch import sample_sources_many, check_sampleable  # noqa: E402,F401
from .pdgp_batch import tie_groups, check_tied  # noqa: E402,F401
from .sgpr_ss import merged_order, sample_eps_shapes, sample_components  # noqa: E402,F401
from .sgpr_ss import ssm_timeline, ssm_state_dim, ssm_sample_eps_shapes  # noqa: E402,F401
from . import checkpoint  # noqa: E402,F401  (binds state_dict / load_state_dict to Pdgp, SGPRSS and Kern)
from .checkpoint import save, load  # noqa: E402,F401
from .init_models import init_liv, init_iv  # noqa: E402,F401
from .window_overlap import segmented, windowed, merged_mean, merged_variance  # noqa: E402,F401
from .init_kernels import init_kern_act, init_kern_com, init_kern  # noqa: E402,F401
