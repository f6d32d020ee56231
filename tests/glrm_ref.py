"""np.longdouble oracle of the masked GLRM kernels (tests/test_glrm_kernels_gpu.py)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def x_ref(A, mask, Y, lam):
    """Per row: G_i = Ym Ym^T + lam I and r_i = Ym a_i over the observed columns in
    np.longdouble, solved in float64.  Returns X [k][n] and the condition numbers [n]."""
    k, n = Y.shape[0], A.shape[1]
    X, kappa = np.zeros((k, n)), np.zeros(n)
    for i in range(n):
        m = mask[:, i]
        Ym = Y[:, m].astype(LD)
        G = (Ym @ Ym.T + LD(lam) * np.eye(k, dtype=LD)).astype(np.float64)
        X[:, i] = np.linalg.solve(G, (Ym @ A[m, i].astype(LD)).astype(np.float64))
        kappa[i] = np.linalg.cond(G)
    return X, kappa


def y_terms_ref(A, mask, X):
    """Per data column: [Xm Xm^T | Xm a_j] over the observed rows, and the same with
    absolute values, both [p][k][k + 1] in np.longdouble."""
    k, p = X.shape[0], A.shape[0]
    S, mag = np.zeros((p, k, k + 1), dtype=LD), np.zeros((p, k, k + 1), dtype=LD)
    for j in range(p):
        m = mask[j]
        Xm, a = X[:, m].astype(LD), A[j, m].astype(LD)
        S[j] = np.concatenate([Xm @ Xm.T, (Xm @ a)[:, None]], 1)
        mag[j] = np.concatenate([np.abs(Xm) @ np.abs(Xm).T, (np.abs(Xm) @ np.abs(a))[:, None]], 1)
    return S, mag
