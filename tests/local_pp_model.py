"""The local posterior of a branch (qs_branch_frequencies, engine.local_pp, csrc/host/local_pp.hpp) without a GPU and
without doubles.

frequencies: (n_nodes, 4) Python integers (en, Z1, Z2, Z3) from rows (m, n_nodes, 4) of per-tree words (present, q1, q2, q3): en = the
trees with S = q1 + q2 + q3 > 0, Z_i = the sum over them of floor(q_i * 2^40 / S), in big integers.
posterior: (pp1, pp2, pp3, length, polytomy_p) from en and z = (z1, z2, z3) with mpmath at 50 digits, straight from the definition:
h(x) = the unregularised incomplete beta integral from 1/3 to 1 with a = x + 1, b = en - x + 2 lam; no log space is needed there.
beta_tail: that integral as a series of positive terms (mpmath.betainc subtracts two large numbers and gives up at en = 10^4):
  int_0^x u^(p-1) (1-u)^(q-1) du = x^p (1-x)^q / p * sum_k prod_{j<k} (p + q + j) / (p + 1 + j) * x
(Euler's transformation of the hypergeometric form of the integral), taken with p = b, q = a, x = 2/3 after u = 1 - t. The two tails
of a case add up to B(a, b), which tests/test_local_pp_model.py checks."""
import math

import mpmath

ONE = 1 << 40


def frequencies(rows):
    rows = [[[int(w) for w in node] for node in tree] for tree in rows]
    n_nodes = len(rows[0]) if rows else 0
    out = [[0, 0, 0, 0] for _ in range(n_nodes)]
    for tree in rows:
        for v, (_, q1, q2, q3) in enumerate(tree):
            s = q1 + q2 + q3
            if s > 0:
                out[v][0] += 1
                for i, q in enumerate((q1, q2, q3)):
                    out[v][1 + i] += q * ONE // s
    return out


def beta_tail(p, q, x):
    """int_0^x u^(p-1) (1-u)^(q-1) du at the working precision"""
    p, q, x = mpmath.mpf(p), mpmath.mpf(q), mpmath.mpf(x)
    term = total = mpmath.mpf(1)
    k = 0
    small = mpmath.mpf(10) ** -(mpmath.mp.dps + 10)
    while term > total * small:
        term *= (p + q + k) / (p + 1 + k) * x
        total += term
        k += 1
    return mpmath.power(x, p) * mpmath.power(1 - x, q) / p * total


def posterior(en, z, lam=0.5):
    if en <= 0:
        return (math.nan,) * 5
    with mpmath.workdps(50):
        z = [mpmath.mpf(x) for x in z]
        lam, n = mpmath.mpf(lam), mpmath.mpf(en)
        third = mpmath.mpf(1) / 3
        w = [mpmath.power(2, x) * beta_tail(n - x + 2 * lam, x + 1, 2 * third) for x in z]
        total = w[0] + w[1] + w[2]
        pp = [float(x / total) for x in w]
        theta = z[0] / (n + 2 * lam - 1)
        if theta <= third:
            length = 0.0
        elif theta >= 1:
            length = math.inf
        else:
            length = float(-mpmath.log(mpmath.mpf(3) / 2 * (1 - theta)))
        chi2 = sum((x - n / 3) ** 2 / (n / 3) for x in z)
        return pp[0], pp[1], pp[2], length, float(mpmath.exp(-chi2 / 2))
