"""TEST HELPER - the exact transient distribution of synth.birth_death.

The species do not interact: species i has immigration k_i and death g_i x_i.  Started from x0, species i at time t is
distributed as Binomial(x0_i, e^{-g_i t}) (the survivors of the start population) convolved with
Poisson(k_i / g_i (1 - e^{-g_i t})) (the immigrants still alive), and the species are independent, so the distribution
on the box is the outer product of the per-species pmfs with the index sum_i x_i stride_i, species 0 fastest.

The FSP solution R on the box is a lower bound of the truth restricted to the box, and the mass it lost is exactly
the gap between the two (Munsky & Khammash 2006, Theorem 2.2):  truth|box - R >= 0 and
sum(truth|box - R) = 1 - sum(R) - (the truth's mass outside the box).
"""
import numpy as np
from scipy import stats


def species_pmf(x0, k, g, t, size):
    """pmf of one species on 0..size-1"""
    p = np.exp(-g * t)
    lam = k / g * -np.expm1(-g * t)
    x = np.arange(size)
    surv = stats.binom.pmf(x, int(x0), p)
    immi = stats.poisson.pmf(x, lam)
    return np.convolve(surv, immi)[:size]


def box_pmf(dims, k, g, x0, t):
    """-> (the truth restricted to the box as a flat vector, species 0 fastest; the truth's mass outside the box)"""
    vs = [species_pmf(x0[i], k[i], g[i], t, dims[i]) for i in range(len(dims))]
    p = vs[0]
    for v in vs[1:]:
        p = (v[:, None] * p[None, :]).reshape(-1)
    inside = 1.0
    for v in vs:
        inside *= v.sum()
    return p, max(0.0, 1.0 - inside)


def default_rates(d):
    """synth.birth_death's default k and g"""
    return np.linspace(5.0, 9.0, d), np.linspace(0.6, 1.4, d)
