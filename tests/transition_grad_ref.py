"""NumPy restatement of the linearised transition ("Linearisation"): test infrastructure, no product path imports
it.  Mean and variance of the SE-ARD conditional (white=True, full_cov=False) written with beta and Gamma of
moment_ref.posterior_terms, and their gradients with respect to the input rows, in a floating-point type of the caller's choice:
np.float64 is the reference the device is compared with, np.longdouble measures that reference's own error (e_ref).  Kernels are the
oracle's SquaredExponential objects (logvariance, loglengthscales)."""
import numpy as np


def linearize(Xnew, Z, kern, beta, Gam, dtype=np.float64):
    """mean, var (N, D) and dmean, dvar (N, D, P) of one group:
         k_j = s2 exp(-sum_p (x_p - z_jp)^2 / (2 l_p^2)),  nu_jp = z_jp - x_p,  t = Gamma k
         mean = sum_j k_j beta_j                       var = s2 - sum_j k_j t_j
         dmean_p = (1 / l_p^2) sum_j k_j beta_j nu_jp  dvar_p = -(2 / l_p^2) sum_j k_j t_j nu_jp"""
    t = dtype
    X, Z = np.asarray(Xnew, dtype=t), np.asarray(Z, dtype=t)
    (N, P), D = X.shape, len(kern)
    mean, var = np.zeros((N, D), dtype=t), np.zeros((N, D), dtype=t)
    dmean, dvar = np.zeros((N, D, P), dtype=t), np.zeros((N, D, P), dtype=t)
    nu = Z[None, :, :] - X[:, None, :]                                           # (N, M, P)
    for a in range(D):
        s2 = np.exp(t(kern[a].logvariance))
        il2 = np.exp(-2 * np.asarray(kern[a].loglengthscales, dtype=t))          # 1 / l^2, (P,)
        K = s2 * np.exp(-0.5 * np.sum(nu * nu * il2[None, None, :], axis=2))     # (N, M)
        b, G = np.asarray(beta[a], dtype=t), np.asarray(Gam[a], dtype=t)
        T = K @ G
        mean[:, a] = K @ b
        var[:, a] = s2 - np.sum(K * T, axis=1)
        dmean[:, a] = np.einsum("nm,nmp->np", K * b[None, :], nu) * il2[None, :]
        dvar[:, a] = -2 * np.einsum("nm,nmp->np", K * T, nu) * il2[None, :]
    return mean, var, dmean, dvar


def mixture(groups):
    """The equal-weight mixture over the groups and its gradients, from a list of (mean, var, dmean, dvar): mix_mean, mix_var,
    mix_dmean, mix_dvar; the variance gradient in centred form, mean_g(dvar_g + 2 (mean_g - mix_mean) dmean_g)."""
    m, v = np.stack([g[0] for g in groups]), np.stack([g[1] for g in groups])
    dm, dv = np.stack([g[2] for g in groups]), np.stack([g[3] for g in groups])
    G = len(groups)
    mm = m.sum(axis=0) / G
    mv = (v + m * m).sum(axis=0) / G - mm * mm
    mdm = dm.sum(axis=0) / G
    mdv = (dv + 2 * (m - mm[None])[..., None] * dm).sum(axis=0) / G
    return mm, mv, mdm, mdv


def central_differences(fn, Xnew, h, dtype=np.float64):
    """(fn(X + h e_p) - fn(X - h e_p)) / 2h for every input column p, stacked on a trailing axis; fn returns a tuple of arrays of
    which each gets its own stack."""
    X = np.asarray(Xnew, dtype=dtype)
    P = X.shape[1]
    cols = []
    for p in range(P):
        e = np.zeros(P, dtype=dtype)
        e[p] = h
        up, dn = fn(X + e[None, :]), fn(X - e[None, :])
        cols.append([(np.asarray(u, dtype=dtype) - np.asarray(d, dtype=dtype)) / (2 * dtype(h)) for u, d in zip(up, dn)])
    return tuple(np.stack([c[i] for c in cols], axis=-1) for i in range(len(cols[0])))
