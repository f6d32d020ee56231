"""np.longdouble oracle of the PSVM kernels (tests/test_psvm_kernels_gpu.py)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def icf_ref(X, gamma, p, thresh):
    """The recurrence of ``models.psvm.icf`` in np.longdouble; the pivot is the
    largest residual diagonal, the lowest row index among equals.

    Returns H [n][k_used], the pivot rows, and per accepted step after the first
    the distance from the largest residual diagonal to the second largest among
    the rows that are not bitwise copies of the pivot row; then the margin by
    which every pivot cleared ``thresh`` (and the stopping value missed it)."""
    X = np.asarray(X, dtype=LD)
    n = X.shape[0]
    xsq = (X * X).sum(1)
    diag = np.ones(n, dtype=LD)
    H = np.zeros((n, p), dtype=LD)
    pivots, gaps, margin = [], [], np.inf
    for k in range(p):
        i = int(np.argmax(diag))            # first occurrence of the maximum
        v = diag[i]
        margin = min(margin, float(abs(v - thresh)))
        if v < thresh:
            break
        if k:
            other = ~(X == X[i]).all(1)
            gaps.append(float(v - diag[other].max()) if other.any() else np.inf)
        d2 = np.maximum(xsq - 2 * (X @ X[i]) + xsq[i], 0)
        col = (np.exp(-LD(gamma) * d2) - H[:, :k] @ H[i, :k]) / np.sqrt(v)
        col[i] = np.sqrt(v)
        H[:, k] = col
        diag = np.maximum(diag - col * col, 0)
        diag[i] = 0
        pivots.append(i)
    return H[:, :len(pivots)], pivots, gaps, margin


def wsyrk_ref(A, w):
    """A^T diag(w) A and |A|^T |w| |A| in np.longdouble."""
    A, w = np.asarray(A, dtype=LD), np.asarray(w, dtype=LD)
    return A.T @ (w[:, None] * A), np.abs(A).T @ (np.abs(w)[:, None] * np.abs(A))


def tall_tv_ref(A, s, V):
    A, s, V = (np.asarray(t, dtype=LD) for t in (A, s, V))
    return A.T @ (s[:, None] * V), np.abs(A).T @ np.abs(s[:, None] * V)


def tall_v_ref(A, s, T):
    A, s, T = (np.asarray(t, dtype=LD) for t in (A, s, T))
    return s[:, None] * (A @ T), np.abs(s)[:, None] * (np.abs(A) @ np.abs(T))
