"""Optimiser tokens.  `AdamOptimizer` plays the role of tf.train.AdamOptimizer as passed to
Model.optimize(method=...) in demos/scripts/demo-modgp.py:44-45; the update itself runs on the GPU
(gp_adam_step, csrc/opt.hip).  `NatGradAdam` moves the variational posteriors of a Pdgp by natural-gradient steps
(gp_pdgp_natgrad_step, csrc/natgrad.hip) and everything else by Adam."""


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
    check) and sharded models do not take it."""

    def __init__(self, gamma=0.1, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not (0.0 < float(gamma) <= 1.0):
            raise ValueError("NatGradAdam: gamma must be a number in (0, 1], not %r" % (gamma,))
        self.gamma = float(gamma)
        self.learning_rate = float(learning_rate)
        self.beta1 = float(beta1)
        self.beta2 = float(beta2)
        self.epsilon = float(epsilon)


class OptimizeResult(dict):
    """scipy-style result as GPflow returns it (demo_modgp.ipynb:140-146)."""
    __getattr__ = dict.get
