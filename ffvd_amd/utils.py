"""Counterpart of vfegpssm/utils.py: the reparameterised Monte-Carlo draw, with the N(0,1) sample injected
(TensorFlow's random stream is not reproducible outside TensorFlow, SURVEY 7 'RNG parity')."""
from __future__ import annotations

import numpy as np

from . import _lib


def get_rand(x, eps, full_cov=False, jitter=1e-7):
    """Reparameterised draw for x = (mean, var) (utils.py:4-11); eps (N(0,1)) has the shape of mean.

    full_cov=False: mean + eps * sqrt(var), elementwise (utils.py:11).
    full_cov=True:  mean is N x D, var is D x N x N (conditional(..., full_cov=True)); the joint draw
                    out[:, d] = mean[:, d] + chol(var[d] + jitter I) eps[:, d].  jitter = 1e-7 is the value of the DGP code the
                    reference's get_rand derives from (that file is not part of the reference); a var[d] + jitter I that is not
                    positive definite raises numpy.linalg.LinAlgError naming the dim and the pivot."""
    lib = _lib.load()
    mean = _lib.as_f64(x[0])
    if full_cov:
        if mean.ndim != 2:
            raise ValueError(f"get_rand: mean: expected (N, D), got {mean.shape}")
        N, D = mean.shape
        var = _lib.as_f64(x[1], (D, N, N), "var")
        eps = _lib.as_f64(eps, mean.shape, "eps")
        out = np.empty_like(mean)
        _lib.check(lib.ffvd_op_get_rand_full_cov(_lib.dptr(mean), _lib.dptr(var), _lib.dptr(eps), N, D, float(jitter),
                                                 _lib.dptr(out)), None, "get_rand")
        return out
    var = _lib.as_f64(x[1], mean.shape, "var")
    eps = _lib.as_f64(eps, mean.shape, "eps")
    out = np.empty_like(mean)
    _lib.check(lib.ffvd_op_get_rand(_lib.dptr(mean), _lib.dptr(var), _lib.dptr(eps), mean.size, _lib.dptr(out)), None,
               "get_rand")
    return out
