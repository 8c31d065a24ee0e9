"""numpy restatement of the multi-asset semantics (include/omc.h).  TEST INFRASTRUCTURE ONLY.

table()     the host constants of a basket (what omc_basket_table returns): the lower Cholesky factor of rho row by row
            (Cholesky-Banachiewicz) in float64, a / b to float32 bits, the index of the initial spots and the geometric
            basket's own GBM (G0, sigma_G, q_G) -- in the order of operations the header states, with the C library's
            pow / sqrt (math.pow, math.sqrt).  Raises ValueError where the library refuses rho.
assets()    the d asset matrices in float64 from independent float32 normals z[k] [N][P] (the tests pass the C oracle's
            orc.gbm_normals at the tagged offsets pair_offset + (k << 40)): y_i = sum_{k <= i} Lf[i][k] z_k, the step
            s_i *= exp2(b_i y_i + a_i), partner with every normal flipped; columns p and p + P are the partners.
index()     the index matrix from asset matrices: arithmetic in float64 with the float32 weights; best-of / worst-of from
            the FLOAT32 products wf_k * s_k (what the kernel compares: bit for bit on float32 asset matrices); geometric
            G0f * prod (s_k / s0f_k)^wf_k in float64.
"""
import math

import numpy as np

KINDS = {"basket": 0, "arithmetic": 0, "geometric": 1, "best-of": 2, "worst-of": 3}
L2E = 1.4426950408889634074


def cholesky(rho):
    """row by row; ValueError as the library's -31"""
    rho = np.asarray(rho, np.float64)
    d = rho.shape[0]
    if rho.shape != (d, d) or not np.all(np.isfinite(rho)):
        raise ValueError("rho")
    if np.any(np.abs(np.diag(rho) - 1.0) > 1e-12) or np.any(np.abs(rho - rho.T) > 1e-12):
        raise ValueError("rho")
    L = np.zeros((d, d))
    for i in range(d):
        for j in range(i + 1):
            s = float(rho[i, j])
            for m in range(j):
                s -= L[i, m] * L[j, m]
            if j == i:
                if not s > 1e-12:
                    raise ValueError("rho is not positive definite")
                L[i, j] = math.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return L


def table(S0, sigma, q, w, rho, kind, r, T, n_steps):
    """-> (L float64 [d][d], a float32 [d], b float32 [d], x0, (G0, sigma_G, q_G))"""
    d = len(S0)
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    rho = np.asarray(rho, np.float64)
    L = cholesky(rho)
    arith, G0, var, drift = 0.0, 1.0, 0.0, 0.0
    ws = [w[i] * S0[i] for i in range(d)]
    for i in range(d):
        arith += ws[i]
        G0 *= math.pow(S0[i], w[i])
        for j in range(d):
            var += w[i] * w[j] * sigma[i] * sigma[j] * float(rho[i, j])
        drift += w[i] * (r - q[i] - sigma[i] * sigma[i] / 2.0)
    x0 = (arith, G0, max(ws), min(ws))[kind]
    dt = T / n_steps
    a = np.array([np.float32(((r - q[i]) - 0.5 * sigma[i] * sigma[i]) * dt * L2E) for i in range(d)], np.float32)
    b = np.array([np.float32(sigma[i] * math.sqrt(dt) * L2E) for i in range(d)], np.float32)
    return L, a, b, x0, (G0, math.sqrt(var), r - drift - var / 2.0)


def assets(z, S0, a, b, L):
    """z [d][N][P] independent normals -> float64 [d][N+1][2P]"""
    z = np.asarray(z, np.float64)
    d, N, P = z.shape
    Lf = np.asarray(L, np.float32).astype(np.float64)
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    out = np.empty((d, N + 1, 2 * P))
    for i in range(d):
        y = sum(Lf[i, k] * z[k] for k in range(i + 1))
        s0 = float(np.float32(S0[i]))
        out[i, 0] = s0
        out[i, 1:, :P] = s0 * np.exp2(np.cumsum(b64[i] * y + a64[i], axis=0))
        out[i, 1:, P:] = s0 * np.exp2(np.cumsum(-b64[i] * y + a64[i], axis=0))
    return out


def index(A, w, kind, S0=None, G0=None):
    """A [d][N+1][M] asset matrices (float32 or float64) -> the index matrix [N+1][M]; the geometric kind needs S0, G0"""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    wf = np.asarray(w, np.float32)
    d = len(wf)
    if kind == 0:
        return sum(np.float64(wf[k]) * np.asarray(A[k], np.float64) for k in range(d))
    if kind == 1:
        g = np.full(np.asarray(A[0]).shape, float(np.float32(G0)))
        for k in range(d):
            g = g * (np.asarray(A[k], np.float64) / float(np.float32(S0[k]))) ** float(wf[k])
        return g
    if np.asarray(A).dtype == np.float32:
        prods = [wf[k] * np.asarray(A[k], np.float32) for k in range(d)]  # float32 products, as the kernel forms them
    else:
        prods = [np.float64(wf[k]) * np.asarray(A[k], np.float64) for k in range(d)]
    x = prods[0]
    for k in range(1, d):
        x = np.maximum(x, prods[k]) if kind == 2 else np.minimum(x, prods[k])
    return x
