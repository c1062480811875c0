"""CPU ORACLE helper (test infrastructure): the four-point homography fit of tests/homography_oracle.py
evaluated in multi-precision arithmetic (mpmath), as the arbiter between two double-precision implementations (LAPACK in the
NumPy definition, Householder QR and one-sided Jacobi on the GPU), and the symmetric transfer error in the same arithmetic."""
import mpmath as mp
import numpy as np


def _condition(pts):
    """Four (x, y) mpf pairs -> (centroid x, centroid y, sqrt(2) / mean distance, or None for four coincident points)."""
    cx = sum(p[0] for p in pts) / 4
    cy = sum(p[1] for p in pts) / 4
    dist = sum(mp.sqrt((x - cx) ** 2 + (y - cy) ** 2) for x, y in pts) / 4
    return cx, cy, (None if dist == 0 else mp.sqrt(2) / dist)


def fit_homography_mp(sample: np.ndarray, dps: int = 50):
    """sample (4, 4) float64 rows {xa, ya, xb, yb} -> (H (9,) float64 rounded from a `dps`-digit computation, scaled to
    ||H||_F = 1 with det H >= 0; sigma_8 / sigma_1 of the conditioned 8 x 9 system as an mpf).  The conditioning and the
    system are those of homography_oracle.fit.  A sample that is not finite, or whose four points coincide in one image,
    gives (NaNs, mpf nan)."""
    sample = np.asarray(sample, dtype=np.float64)
    assert sample.shape == (4, 4)
    nothing = np.full(9, np.nan), mp.mpf("nan")
    if not np.all(np.isfinite(sample)):
        return nothing
    with mp.workdps(dps):
        a = [(mp.mpf(float(r[0])), mp.mpf(float(r[1]))) for r in sample]
        b = [(mp.mpf(float(r[2])), mp.mpf(float(r[3]))) for r in sample]
        (cax, cay, sa), (cbx, cby, sb) = (_condition(pts) for pts in (a, b))
        if sa is None or sb is None:
            return nothing
        A = mp.matrix(8, 9)
        for i in range(4):
            x, y = (a[i][0] - cax) * sa, (a[i][1] - cay) * sa
            u, v = (b[i][0] - cbx) * sb, (b[i][1] - cby) * sb
            for j, value in enumerate([x, y, 1, 0, 0, 0, -u * x, -u * y, -u]):
                A[2 * i, j] = value
            for j, value in enumerate([0, 0, 0, x, y, 1, -v * x, -v * y, -v]):
                A[2 * i + 1, j] = value
        _, sigma, V = mp.svd_r(A, full_matrices=True)
        order = sorted(range(8), key=lambda k: sigma[k], reverse=True)
        ratio = sigma[order[7]] / sigma[order[0]]
        ht = [V[8, j] for j in range(9)]
        # H = T_b^-1 H~ T_a
        Ta = mp.matrix([[sa, 0, -sa * cax], [0, sa, -sa * cay], [0, 0, 1]])
        Tb_inv = mp.matrix([[1 / sb, 0, cbx], [0, 1 / sb, cby], [0, 0, 1]])
        H = Tb_inv * mp.matrix([ht[0:3], ht[3:6], ht[6:9]]) * Ta
        norm = mp.sqrt(sum(H[r, c] ** 2 for r in range(3) for c in range(3)))
        H = H / norm
        if mp.det(H) < 0:
            H = -H
        return np.array([float(H[r, c]) for r in range(3) for c in range(3)]), ratio


def transfer_error_mp(H, item, dps: int = 50):
    """The symmetric transfer error of one item {xa, ya, xb, yb} under H (9,), the formula of homography_oracle.transfer_error
    evaluated with `dps` digits on the float64 inputs as given: an mpf, +inf where p2 <= 0 or q2 <= 0 (in exact sign), and
    nan where H or the item is not finite."""
    H = [float(v) for v in np.ravel(H)]
    item = [float(v) for v in item]
    if not (np.all(np.isfinite(H)) and np.all(np.isfinite(item))):
        return mp.mpf("nan")
    with mp.workdps(dps):
        h = [mp.mpf(v) for v in H]
        xa, ya, xb, yb = (mp.mpf(v) for v in item)
        g = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
             h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
             h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
        p = [h[3 * k] * xa + h[3 * k + 1] * ya + h[3 * k + 2] for k in range(3)]
        q = [g[3 * k] * xb + g[3 * k + 1] * yb + g[3 * k + 2] for k in range(3)]
        if p[2] <= 0 or q[2] <= 0:
            return mp.inf
        return (p[0] / p[2] - xb) ** 2 + (p[1] / p[2] - yb) ** 2 + (q[0] / q[2] - xa) ** 2 + (q[1] / q[2] - ya) ** 2
