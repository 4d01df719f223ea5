"""NumPy restatement of moment-matched prediction (Girard et al. 2003): test infrastructure, no product path
imports it.  The formulas are written as the design states them -- direct solves with Sigma + Lambda, the pair exponent in one piece,
the centred form of Cov(f) -- in a floating-point type of the caller's choice: np.float64 is the reference the device is compared
with, np.longdouble measures that reference's own error (e_ref).  np.linalg does not take np.longdouble, so the D x D elimination is
written out here.  Kernels are the oracle's SquaredExponential objects (logvariance, loglengthscales)."""
import numpy as np


def ge_solve(A, B):
    """X = A^-1 B and |A| by Gaussian elimination with partial pivoting, in A's dtype (A need not be positive definite)."""
    A, B = np.array(A, copy=True), np.array(B, copy=True)
    n = A.shape[0]
    det = A.dtype.type(1)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]], B[[k, piv]] = A[[piv, k]], B[[piv, k]]
            det = -det
        det = det * A[k, k]
        for r in range(k + 1, n):
            f = A[r, k] / A[k, k]
            A[r, k:] = A[r, k:] - f * A[k, k:]
            B[r] = B[r] - f * B[k]
    X = np.zeros_like(B)
    for r in range(n - 1, -1, -1):
        X[r] = (B[r] - A[r, r + 1:] @ X[r + 1:]) / A[r, r]
    return X, det


def posterior_terms(W_seq, U, q_sqrt=None, q_mode="reference", dtype=np.float64):
    """beta (D, M) = W_a u_a and Gamma (D, M, M) = W_a (I - q_a q_a^T) W_a^T; q_a = slice 0 ("reference") or slice a ("intent")."""
    D = len(W_seq)
    U = np.asarray(U, dtype=dtype)
    beta, Gam = [], []
    for a in range(D):
        W = np.asarray(W_seq[a], dtype=dtype)
        beta.append(W @ U[:, a])
        G = W @ W.T
        if q_sqrt is not None:
            B = W @ np.asarray(q_sqrt[0 if q_mode == "reference" else a], dtype=dtype)
            G = G - B @ B.T
        Gam.append(G)
    return np.stack(beta), np.stack(Gam)


def step_parts(mu, S, c, Z, kern, beta, Gam, dtype=np.float64):
    """E[f] (D,), Cov(f) (D, D) and V (D, D; column a = Cov(x, f_a)) of f at x ~ N(mu, S), control row c."""
    t = dtype
    mu, S, Z = np.asarray(mu, dtype=t), np.asarray(S, dtype=t), np.asarray(Z, dtype=t)
    D, (M, P) = mu.shape[0], Z.shape
    xin = np.concatenate((mu, np.asarray(c, dtype=t).reshape(-1)))
    nu = Z - xin[None, :]                                                        # (M, P)
    var = [np.exp(t(k.logvariance)) for k in kern]
    il2 = [np.exp(-2 * np.asarray(k.loglengthscales, dtype=t)) for k in kern]    # 1 / l^2, (P,)
    I = np.eye(D, dtype=t)
    q, Ef, V = [], np.zeros(D, dtype=t), np.zeros((D, D), dtype=t)
    for a in range(D):
        lam = il2[a][:D]
        _, detR = ge_solve(S * lam[None, :] + I, I)
        sol, _ = ge_solve(S + np.diag(1 / lam), nu[:, :D].T)                     # (Sigma + Lambda)^-1 nu^x, (D, M)
        ex = -0.5 * np.sum(nu[:, :D] * sol.T, axis=1) - 0.5 * np.sum(nu[:, D:] ** 2 * il2[a][None, D:], axis=1)
        qa = var[a] / np.sqrt(detR) * np.exp(ex)
        q.append(qa)
        Ef[a] = qa @ beta[a]
        r = (beta[a] * qa) @ nu[:, :D]
        w, _ = ge_solve(S + np.diag(1 / lam), r[:, None])
        V[:, a] = S @ w[:, 0]
    Cf = np.zeros((D, D), dtype=t)
    for a in range(D):
        for b in range(a, D):
            la, lb = il2[a][:D], il2[b][:D]
            T, detR = ge_solve(S * (la + lb)[None, :] + I, S)
            ai, bj = nu[:, :D] * la[None, :], nu[:, :D] * lb[None, :]
            ei = -0.5 * np.sum(nu ** 2 * il2[a][None, :], axis=1)
            gj = -0.5 * np.sum(nu ** 2 * il2[b][None, :], axis=1)
            s = ai[:, None, :] + bj[None, :, :]                                  # (M, M, D)
            quad = np.einsum("ijk,kl,ijl->ij", s, T, s)
            Q = var[a] * var[b] / np.sqrt(detR) * np.exp(ei[:, None] + gj[None, :] + 0.5 * quad)
            v = np.sum((beta[a][:, None] * beta[b][None, :]) * (Q - q[a][:, None] * q[b][None, :]))
            if a == b:
                v = v + var[a] - np.sum(Gam[a] * Q)
            Cf[a, b] = Cf[b, a] = v
    return Ef, Cf, V


def propagate(mu0, S0, ctrl, Z, kern, beta, Gam, Q, steps, dtype=np.float64):
    """m_x (steps, D), S_x (steps, D, D): the state after each step; ctrl (>= steps, C) or None."""
    t = dtype
    mu, S = np.asarray(mu0, dtype=t), np.asarray(S0, dtype=t)
    D = mu.shape[0]
    Qd = np.diag(np.asarray(Q, dtype=t))
    ms, Ss = np.zeros((steps, D), dtype=t), np.zeros((steps, D, D), dtype=t)
    for i in range(steps):
        c = np.zeros(0, dtype=t) if ctrl is None else ctrl[i]
        Ef, Cf, V = step_parts(mu, S, c, Z, kern, beta, Gam, dtype=t)
        mu = mu + Ef
        S = S + Cf + V + V.T + Qd
        S = np.triu(S) + np.triu(S, 1).T
        ms[i], Ss[i] = mu, S
    return ms, Ss


def summary(m_x, S_x, CC, DD, sd, Y=None):
    """The held-out summary over the G groups (equal weights): m_x (G, steps, D), S_x (G, steps, D, D), CC (D, J), DD, sd (J,)."""
    m = np.einsum("gtk,kj->gtj", m_x, CC) + DD[None, None, :]
    s2 = np.einsum("kj,gtkl,lj->gtj", CC, S_x, CC) + (sd ** 2)[None, None, :]
    ym = m.mean(axis=0)
    vt = (s2 + m * m).mean(axis=0) - ym * ym
    out = dict(y_mean=ym, y_var_total=vt)
    if Y is not None:
        n = Y.shape[0]
        ex = -0.5 * (np.log(2 * np.pi) + np.log(s2[:, :n])) - 0.5 * (Y[None] - m[:, :n]) ** 2 / s2[:, :n]
        mx = ex.max(axis=0)
        out["lpd"] = mx + np.log(np.exp(ex - mx[None]).sum(axis=0)) - np.log(m.shape[0])
        out["lpd_gauss"] = -0.5 * (np.log(2 * np.pi) + np.log(vt[:n])) - 0.5 * (Y - ym[:n]) ** 2 / vt[:n]
    return out
