#!/usr/bin/env python
"""Climbing one Thompson sample by gradient ascent: a 1-D model with one Gaussian task, one posterior sample path drawn as a
function (`SVMOGP.sample_paths`), and a few starts that follow `PosteriorPaths.value_and_grad` uphill inside [0, 1].  A demonstration of the
interface, not a tested optimiser.  Run on an MI355X:
    python examples/thompson_ascent.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hetmogp_amd import SVMOGP, HetLikelihood, Gaussian, util  # noqa: E402


def main(seed=0, starts=5, steps=60, verbose=True):
    rng = np.random.RandomState(seed)
    X = np.sort(rng.rand(200))[:, None]
    Y = np.sin(6.0 * X) + 0.5 * np.cos(17.0 * X) + 0.1 * rng.randn(200, 1)
    likelihood = HetLikelihood([Gaussian(sigma=0.1)])
    kern_list = util.latent_functions_prior(1, lenghtscale=np.array([0.1]), variance=np.array([1.0]), input_dim=1)
    model = SVMOGP(X=[X], Y=[Y], Z=np.linspace(0, 1, 20)[:, None], kern_list=kern_list, likelihood=likelihood,
                   Y_metadata=likelihood.generate_metadata())
    model = util.vem_algorithm(model, stochastic=False, vem_iters=3, optZ=False, verbose=False, verbose_plot=False, non_chained=True)
    with model.sample_paths(size=1, functions=[0], num_features=512, seed=seed) as path:      # one Thompson sample, a function of x
        x = np.linspace(0.1, 0.9, starts)[:, None]
        f0 = path(x)[0, :, 0]
        for _ in range(steps):                                                              # all starts climb in one call per step
            f, g = path.value_and_grad(x)
            x = np.clip(x + 0.002 * g[0, :, 0, :], 0.0, 1.0)
        f1 = path(x)[0, :, 0]
    best = int(np.argmax(f1))
    if verbose:
        for a, b, c in zip(f0, f1, x[:, 0]):
            print("start value %8.4f -> %8.4f at x = %.4f" % (a, b, c))
        print("next query of the Thompson sample: x = %.4f (value %.4f)" % (x[best, 0], f1[best]))
    return x[best, 0], f0, f1


if __name__ == "__main__":
    main()
