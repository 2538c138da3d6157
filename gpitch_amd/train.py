"""Optimiser tokens.  `AdamOptimizer` plays the role of tf.train.AdamOptimizer as passed to
Model.optimize(method=...) in demos/scripts/demo-modgp.py:44-45; the update itself runs on the GPU
(gp_adam_step, csrc/opt.hip).  `NatGradAdam` moves the variational posteriors of a Pdgp by natural-gradient steps
(gp_pdgp_natgrad_step, csrc/natgrad.hip) and everything else by Adam; with `gamma_com` or `halvings` it gives the component
GPs a step length of their own and halves, per latent GP and on the device, a step that would be refused
(gp_pdgp_natgrad_step_adaptive)."""
import math


class AdamOptimizer(object):
    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.learning_rate = float(learning_rate)
        self.beta1 = float(beta1)
        self.beta2 = float(beta2)
        self.epsilon = float(epsilon)


class NatGradAdam(object):
    """Pdgp.optimize(method=NatGradAdam(gamma, learning_rate, ...)): per iteration one natural-gradient step of length
    `gamma` on q(u) of every latent GP whose q_mu and q_sqrt are both free, then Adam (the remaining arguments, as
    AdamOptimizer's) on the noise variance, the kernels' Params and the inducing inputs, from the same ELBO evaluation.
    With everything else fixed, gamma = 1 puts q(u) of a component GP on its optimum in one step (the data term is
    linear in its expectation parameters); the activations' likelihood is not conjugate, and a step whose I - 2 gamma P
    is not positive definite is refused with NotPositiveDefiniteError: take a smaller gamma.  optimize_many /
    PdgpBatch.optimize take the token too (gp_pdgpb_natgrad, csrc/pdgp_batch.hip) and refuse such a step per model: the
    refused model is left as it was, the others go on.  Not an AdamOptimizer: check_batchable (the Adam path's scope
    check) and sharded models do not take it.

    Keyword-only: `gamma_com` (None, or a number in (0, 1]) is the component GPs' step length, `gamma` then being the
    activation GPs' (gamma_com = 1 is exact for the conjugate component GPs while the activations stay damped);
    `halvings` (an int in 0..10) lets every latent GP, each iteration and independently of the others, take the first of
    gamma, gamma / 2, ..., gamma / 2^halvings whose I - 2 gamma P is positive definite, and only a GP for which none is
    refuses the step.  Each iteration starts from the full length again.  The result of optimize() then carries
    natgrad = {"halvings": [...], "shortest_gamma": [...]}, per latent GP in the rows [g_0..g_{P-1}, f_0..f_{P-1}]: the
    halvings summed over the iterations and the shortest length taken.  A token with neither argument follows the
    one-length code path unchanged."""

    def __init__(self, gamma=0.1, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, *, gamma_com=None, halvings=0):
        self.gamma = self.check_gamma("gamma", gamma)
        self.gamma_com = None if gamma_com is None else self.check_gamma("gamma_com", gamma_com)
        self.halvings = self.check_halvings(halvings)
        self.learning_rate = float(learning_rate)
        self.beta1 = float(beta1)
        self.beta2 = float(beta2)
        self.epsilon = float(epsilon)

    @staticmethod
    def check_gamma(name, gamma):
        if (isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma)
                or not (0.0 < float(gamma) <= 1.0)):
            raise ValueError("NatGradAdam: %s must be a number in (0, 1], not %r" % (name, gamma))
        return float(gamma)

    @staticmethod
    def check_halvings(halvings):
        if isinstance(halvings, bool) or not isinstance(halvings, int) or not (0 <= halvings <= 10):
            raise ValueError("NatGradAdam: halvings must be an int in 0..10, not %r" % (halvings,))
        return halvings

    def adaptive(self):
        """does the token take the per-role / halving entries (gp_pdgp_natgrad_step_adaptive, gp_pdgpb_natgrad_adaptive)?"""
        return getattr(self, "gamma_com", None) is not None or getattr(self, "halvings", 0) != 0

    def role_gammas(self, num_sources):
        """the step length of every latent GP in the rows [g_0..g_{P-1}, f_0..f_{P-1}]"""
        com = self.gamma if self.gamma_com is None else self.gamma_com
        return [self.gamma] * num_sources + [com] * num_sources


class OptimizeResult(dict):
    """scipy-style result as GPflow returns it (demo_modgp.ipynb:140-146)."""
    __getattr__ = dict.get
