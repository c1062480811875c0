"""Five-point essential-matrix solver: the host definition of the device fit in ``csrc/sfm_five_point.h`` (same steps, same
operation order, fp64), vectorised over a batch of samples.

Five K-normalised correspondences (a_i, b_i), a = (xa, ya, 1), b = (xb, yb, 1); every E with b_i^T E a_i = 0 on the five,
det E = 0 and 2 E E^T E - tr(E E^T) E = 0 (Nister, PAMI 2004):
  1. null basis of the 5 x 9 epipolar system by Householder QR of its 9 x 5 transpose (the last four columns of Q);
     SFM_FIT_DEGENERATE when min |r_kk| <= 1e-9 max |r_kk| (numerical rank < 5) or an input is not finite.  X, Y, Z, W are
     the four columns mixed by the fixed orthogonal ``MIX``: the last column of Q alone is orthogonal to the true E of
     every motion with E[2][2] = 0 (pure translations, forward motion, rolls about the optical axis), whose solution would
     then lie at infinity in (x, y, z);
  2. E = x X + y Y + z Z + W turns the ten constraints into ten cubics in x, y, z: a 10 x 20 coefficient matrix in the
     monomial order of ``CUBIC``, whose left 10 x 10 block is Gauss-Jordan eliminated with partial pivoting;
  3. rows e - z f, g - z h, i - z j of the reduced system give a 3 x 3 matrix B(z) with B(z) (x, y, 1)^T = 0; its
     determinant is a degree-10 polynomial n(z);
  4. the real roots of n by a Sturm sequence: the k-th smallest is isolated by bisection on the sign-change count (at most
     ``ISOLATE_STEPS`` steps), then polished by Newton's method kept inside its bracket (at most ``POLISH_STEPS``);
  5. each root z: (x, y, 1) is proportional to the cross product of two rows of B(z), the pair (of (0, 1), (0, 2), (1, 2),
     the first on ties) whose product has the largest third component; (x, y, z) is then polished by ``REFINE_STEPS``
     Newton steps on the three equations B(z) (x, y, 1)^T = 0, whose coefficients come straight from the elimination: the
     roots of n carry the cancellation of its expansion (1e-6 in E at small parallax, forward motion), the polished ones
     the conditioning of the elimination alone.  ``CONSTRAINT_STEPS`` Gauss-Newton steps on the ten constraints themselves,
     evaluated on E = x X + y Y + z Z + W (their 10 x 3 Jacobian by the normal equations), then take the elimination out of
     the result as well.  E is scaled to ||E||_F = sqrt(2) with its largest-magnitude entry (the first in row-major order on
     ties) positive.
Candidates come in the ascending order of the roots of n; the polish of step 5 can move z past a neighbouring root, and two
nearly double roots can be polished onto the same solution, which then comes twice.  The fit scores each one on item 5 with the SED as it is made and keeps the best
(strict <, from +inf); a sample without a real solution gives 9 NaNs and flag 0.
"""
from __future__ import annotations

import numpy as np

from .eight_point import EightPointCalculationError

# numerical rank < 5 of the 5 x 9 system: min |r_kk| <= RANK_FLOOR * max |r_kk| of its Householder QR
RANK_FLOOR = 1e-9
ISOLATE_STEPS = 80
POLISH_STEPS = 100
REFINE_STEPS = 2
CONSTRAINT_STEPS = 2
MAX_CANDIDATES = 10

# X, Y, Z, W = MIX @ (the last four columns of Q): orthogonal (the rows of the left-multiplication matrix of the quaternion
# (2, 4, 5, 6), of norm 9), no entry zero, so that W has a component along every column
MIX = [[2.0 / 9.0, -4.0 / 9.0, -5.0 / 9.0, -6.0 / 9.0],
       [4.0 / 9.0, 2.0 / 9.0, -6.0 / 9.0, 5.0 / 9.0],
       [5.0 / 9.0, 6.0 / 9.0, 2.0 / 9.0, -4.0 / 9.0],
       [6.0 / 9.0, -5.0 / 9.0, 4.0 / 9.0, 2.0 / 9.0]]

# monomials as exponents of (x, y, z); LIN: the linear entries of E, QUAD: products of two, CUBIC: Nister's order, whose
# first ten columns are eliminated and whose last ten are xz^2, xz, x, yz^2, yz, y, z^3, z^2, z, 1
LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
QUAD = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
CUBIC = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


LMUL = [[QUAD.index(_add(LIN[i], LIN[j])) for j in range(4)] for i in range(4)]
QMUL = [[CUBIC.index(_add(QUAD[q], LIN[i])) for i in range(4)] for q in range(10)]


class FivePointCalculationError(EightPointCalculationError):
    """A sampled six-tuple is degenerate for the five-point solver (its 5 x 9 system has numerical rank < 5, an input is not
    finite or an index is out of range).  A subclass of EightPointCalculationError, so existing handlers catch it."""


Degenerate = FivePointCalculationError


def _mul_ll(a, b):
    out = [0.0] * 10
    for i in range(4):
        for j in range(4):
            out[LMUL[i][j]] = out[LMUL[i][j]] + a[i] * b[j]
    return out


def _mul_ql(q, a):
    out = [0.0] * 20
    for k in range(10):
        for i in range(4):
            out[QMUL[k][i]] = out[QMUL[k][i]] + q[k] * a[i]
    return out


def null_basis(a: np.ndarray, b: np.ndarray):
    """a, b: (M, 5, 2) K-normalised coordinates -> (basis (M, 4, 9), degenerate (M,) bool).  Step 1."""
    xa, ya, xb, yb = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    one = np.ones_like(xa)
    # A = Q^T: column i is the epipolar row of item i, entry 3 j + k = b_j a_k
    A = [[c[:, i] for i in range(5)] for c in (xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, one)]
    vs, betas, r = [], [], []
    for k in range(5):
        ss = np.zeros_like(xa[:, 0])
        for i in range(k, 9):
            ss = ss + A[i][k] * A[i][k]
        norm = np.sqrt(ss)
        alpha = np.where(A[k][k] >= 0.0, -norm, norm)
        v = [A[i][k] for i in range(k, 9)]
        v[0] = v[0] - alpha
        vv = np.zeros_like(ss)
        for t in range(9 - k):
            vv = vv + v[t] * v[t]
        with np.errstate(divide="ignore", invalid="ignore"):
            beta = np.where(vv > 0.0, 2.0 / vv, 0.0)
        for j in range(k + 1, 5):
            s = np.zeros_like(ss)
            for t in range(9 - k):
                s = s + v[t] * A[k + t][j]
            s = s * beta
            for t in range(9 - k):
                A[k + t][j] = A[k + t][j] - s * v[t]
        vs.append(v)
        betas.append(beta)
        r.append(np.abs(alpha))
    rmax = np.maximum.reduce(r)
    rmin = np.minimum.reduce(r)
    finite = np.all(np.isfinite(a), axis=(1, 2)) & np.all(np.isfinite(b), axis=(1, 2))
    degenerate = ~(rmin > RANK_FLOOR * rmax) | ~finite
    q = np.zeros((xa.shape[0], 4, 9))
    for m in range(4):
        y = [np.zeros_like(rmax) for _ in range(9)]
        y[5 + m] = np.ones_like(rmax)
        for k in range(4, -1, -1):
            s = np.zeros_like(rmax)
            for t in range(9 - k):
                s = s + vs[k][t] * y[k + t]
            s = s * betas[k]
            for t in range(9 - k):
                y[k + t] = y[k + t] - s * vs[k][t]
        q[:, m] = np.stack(y, axis=1)
    basis = np.zeros_like(q)
    for m in range(4):
        basis[:, m] = ((MIX[m][0] * q[:, 0] + MIX[m][1] * q[:, 1]) + MIX[m][2] * q[:, 2]) + MIX[m][3] * q[:, 3]
    return basis, degenerate


def coefficient_matrix(basis: np.ndarray) -> np.ndarray:
    """(M, 4, 9) null basis -> (M, 10, 20): row 0 det E, rows 1..9 (2 E E^T E - tr(E E^T) E)_ij row-major.  Step 2."""
    e = [[basis[:, m, i] for m in range(4)] for i in range(9)]   # entry i as a linear polynomial in (x, y, z, 1)

    def sub(p, q):
        return [p[i] - q[i] for i in range(len(p))]

    cof0 = sub(_mul_ll(e[4], e[8]), _mul_ll(e[5], e[7]))
    cof1 = sub(_mul_ll(e[3], e[8]), _mul_ll(e[5], e[6]))
    cof2 = sub(_mul_ll(e[3], e[7]), _mul_ll(e[4], e[6]))
    d0, d1, d2 = _mul_ql(cof0, e[0]), _mul_ql(cof1, e[1]), _mul_ql(cof2, e[2])
    rows = [[(d0[c] - d1[c]) + d2[c] for c in range(20)]]
    eet = {}
    for i in range(3):
        for j in range(i, 3):
            m0, m1, m2 = _mul_ll(e[3 * i], e[3 * j]), _mul_ll(e[3 * i + 1], e[3 * j + 1]), _mul_ll(e[3 * i + 2], e[3 * j + 2])
            eet[i, j] = eet[j, i] = [(m0[c] + m1[c]) + m2[c] for c in range(10)]
    tr = [(eet[0, 0][c] + eet[1, 1][c]) + eet[2, 2][c] for c in range(10)]
    lam = {}
    for i in range(3):
        for k in range(3):
            lam[i, k] = [2.0 * eet[i, k][c] - tr[c] if i == k else 2.0 * eet[i, k][c] for c in range(10)]
    for i in range(3):
        for j in range(3):
            c0, c1, c2 = _mul_ql(lam[i, 0], e[j]), _mul_ql(lam[i, 1], e[3 + j]), _mul_ql(lam[i, 2], e[6 + j])
            rows.append([(c0[c] + c1[c]) + c2[c] for c in range(20)])
    return np.stack([np.stack([np.broadcast_to(v, basis.shape[:1]) for v in row], axis=1) for row in rows], axis=1)


def gauss_jordan(M: np.ndarray) -> np.ndarray:
    """Reduce the left 10 x 10 block of (M, 10, 20) to the identity (partial pivoting, first maximum) -> right block."""
    M = M.copy()
    ar = np.arange(M.shape[0])
    for c in range(10):
        p = c + np.argmax(np.abs(M[:, c:, c]), axis=1)
        row_c = M[ar, c].copy()
        M[ar, c] = M[ar, p]
        M[ar, p] = row_c
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / M[:, c, c]
            M[:, c, c + 1:] = M[:, c, c + 1:] * inv[:, None]
            M[:, c, c] = 1.0
            for r in range(10):
                if r != c:
                    f = M[:, r, c]
                    M[:, r, c + 1:] = M[:, r, c + 1:] - f[:, None] * M[:, c, c + 1:]
                    M[:, r, c] = 0.0
    return M[:, :, 10:]


def _conv(a, b):
    out = [0.0] * (len(a) + len(b) - 1)
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] = out[i + j] + a[i] * b[j]
    return out


def _horner(c, x):
    v = c[-1]
    for i in range(len(c) - 2, -1, -1):
        v = v * x + c[i]
    return v


def _horner_d(c, x):
    """The derivative of the polynomial c at x."""
    k = len(c) - 1
    v = float(k) * c[k]
    for i in range(k - 1, 0, -1):
        v = v * x + float(i) * c[i]
    return v


def _det3(m):
    return ((m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]))
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def hidden_polynomials(B: np.ndarray):
    """(M, 10, 10) right block -> (rows, n): the three rows of B(z) as (x, y, 1) coefficient polynomials and det B(z), all as
    lists of ascending coefficients (arrays over M).  Step 3."""
    def rows(e, f):
        be, bf = B[:, e], B[:, f]
        px = [be[:, 2], be[:, 1] - bf[:, 2], be[:, 0] - bf[:, 1], -bf[:, 0]]
        py = [be[:, 5], be[:, 4] - bf[:, 5], be[:, 3] - bf[:, 4], -bf[:, 3]]
        p1 = [be[:, 9], be[:, 8] - bf[:, 9], be[:, 7] - bf[:, 8], be[:, 6] - bf[:, 7], -bf[:, 6]]
        return px, py, p1

    kx, ky, k1 = rows(4, 5)
    lx, ly, l1 = rows(6, 7)
    mx, my, m1 = rows(8, 9)
    p1 = [u - v for u, v in zip(_conv(ky, l1), _conv(k1, ly))]
    p2 = [u - v for u, v in zip(_conv(k1, lx), _conv(kx, l1))]
    p3 = [u - v for u, v in zip(_conv(kx, ly), _conv(ky, lx))]
    t1, t2, t3 = _conv(p1, mx), _conv(p2, my), _conv(p3, m1)
    n = [(t1[i] + t2[i]) + t3[i] for i in range(11)]
    return ((kx, ky, k1), (lx, ly, l1), (mx, my, m1)), n


def _max_abs(c):
    m = np.abs(c[0])
    for v in c[1:]:
        m = np.maximum(m, np.abs(v))
    return m


def sturm_chain(n):
    """Normalised n (degree 10), its derivative and the Sturm chain s_0..s_10 (s_k of degree 10 - k, each scaled by a
    positive factor to max |coefficient| = 1) -> (n, dn, chain, ok)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = _max_abs(n)
        n = [c / scale for c in n]
        dn = [(i + 1) * n[i + 1] for i in range(10)]
        ds = _max_abs(dn)
        chain = [n, [c / ds for c in dn]]
        for k in range(2, 11):
            a, b = chain[k - 2], chain[k - 1]
            db = len(b) - 1
            q1 = a[db + 1] / b[db]
            q0 = (a[db] - q1 * b[db - 1]) / b[db]
            r = [(a[i] - q1 * b[i - 1]) - q0 * b[i] if i > 0 else a[0] - q0 * b[0] for i in range(db)]
            rs = _max_abs(r)
            chain.append([-(c / rs) for c in r])
    ok = np.ones_like(scale, dtype=bool)
    for s in chain:
        for c in s:
            ok &= np.isfinite(c)
    ok &= chain[0][10] != 0.0
    return n, dn, chain, ok


def root_bound(n):
    """Fujiwara's bound on the moduli of the roots of n (degree 10): 2 max(|n_9 / n_10|, |n_8 / n_10|^(1/2), ...,
    |n_0 / (2 n_10)|^(1/10)) -- within a factor 2 of the largest root, where Cauchy's 1 + max |n_i / n_10| can be orders of
    magnitude above it and cost the bisection as many steps."""
    lead = np.abs(n[10])
    m = np.abs(n[9]) / lead
    for k in range(2, 11):
        q = np.abs(n[10 - k]) / lead
        if k == 10:
            q = 0.5 * q
        m = np.maximum(m, q ** (1.0 / k))
    return 2.0 * m


def sign_changes(chain, x):
    changes = np.zeros(np.shape(x), dtype=np.int64)
    last = np.zeros(np.shape(x), dtype=np.int64)
    for s in chain:
        v = _horner(s, x)
        sg = (v > 0).astype(np.int64) - (v < 0).astype(np.int64)
        changes += ((sg != 0) & (last != 0) & (sg != last)).astype(np.int64)
        last = np.where(sg != 0, sg, last)
    return changes


def sed_value(e, xa, ya, xb, yb):
    """csrc/sfm_math.h sfm::sed_value, same operation order (e: list of 9 arrays)."""
    lb0 = (xb * e[0] + yb * e[3]) + e[6]
    lb1 = (xb * e[1] + yb * e[4]) + e[7]
    lb2 = (xb * e[2] + yb * e[5]) + e[8]
    r = (lb0 * xa + lb1 * ya) + lb2
    la0 = (e[0] * xa + e[1] * ya) + e[2]
    la1 = (e[3] * xa + e[4] * ya) + e[5]
    da = la0 * la0 + la1 * la1
    db = lb0 * lb0 + lb1 * lb1
    return (1.0 / da + 1.0 / db) * (r * r)


def _constraints(e):
    """det E and 2 E E^T E - tr(E E^T) E (row-major) of e (9 arrays) -> (F (10), G = E E^T, tr G, the cofactors of E)."""
    G = [[(e[3 * r] * e[3 * c] + e[3 * r + 1] * e[3 * c + 1]) + e[3 * r + 2] * e[3 * c + 2] for c in range(3)] for r in range(3)]
    tr = (G[0][0] + G[1][1]) + G[2][2]
    cof = [e[4] * e[8] - e[5] * e[7], e[5] * e[6] - e[3] * e[8], e[3] * e[7] - e[4] * e[6],
           e[7] * e[2] - e[8] * e[1], e[8] * e[0] - e[6] * e[2], e[6] * e[1] - e[7] * e[0],
           e[1] * e[5] - e[2] * e[4], e[2] * e[3] - e[0] * e[5], e[0] * e[4] - e[1] * e[3]]
    F = [(e[0] * cof[0] + e[1] * cof[1]) + e[2] * cof[2]]
    for r in range(3):
        for c in range(3):
            F.append(2.0 * ((G[r][0] * e[c] + G[r][1] * e[3 + c]) + G[r][2] * e[6 + c]) - tr * e[3 * r + c])
    return F, G, tr, cof


def _constraints_along(e, d, G, tr, cof):
    """The derivative of ``_constraints`` at e in the direction d (9 arrays)."""
    H = [[(d[3 * r] * e[3 * c] + d[3 * r + 1] * e[3 * c + 1]) + d[3 * r + 2] * e[3 * c + 2] for c in range(3)] for r in range(3)]
    dtr = 2.0 * ((H[0][0] + H[1][1]) + H[2][2])
    dF = cof[0] * d[0]
    for i in range(1, 9):
        dF = dF + cof[i] * d[i]
    out = [dF]
    for r in range(3):
        for c in range(3):
            a = ((H[r][0] + H[0][r]) * e[c] + (H[r][1] + H[1][r]) * e[3 + c]) + (H[r][2] + H[2][r]) * e[6 + c]
            b = (G[r][0] * d[c] + G[r][1] * d[3 + c]) + G[r][2] * d[6 + c]
            out.append((2.0 * (a + b) - dtr * e[3 * r + c]) - tr * d[3 * r + c])
    return out


def _candidate(basis, rows, z):
    B = [[_horner(p, z) for p in row] for row in rows]
    x = y = w = None
    for r, q in ((0, 1), (0, 2), (1, 2)):
        (a1, b1, c1), (a2, b2, c2) = B[r], B[q]
        u0, u1, u2 = b1 * c2 - c1 * b2, c1 * a2 - a1 * c2, a1 * b2 - b1 * a2
        if w is None:
            x, y, w = u0, u1, u2
        else:
            take = np.abs(u2) > np.abs(w)
            x, y, w = np.where(take, u0, x), np.where(take, u1, y), np.where(take, u2, w)
    x = x / w
    y = y / w
    for _ in range(REFINE_STEPS):   # Newton on F_r = a_r(z) x + b_r(z) y + c_r(z), r = 0, 1, 2 (Cramer's rule)
        F, J = [], []
        for row in rows:
            a, b, c = (_horner(p, z) for p in row)
            da, db, dc = (_horner_d(p, z) for p in row)
            F.append((a * x + b * y) + c)
            J.append([a, b, (da * x + db * y) + dc])
        D = _det3(J)
        dx = _det3([[F[r], J[r][1], J[r][2]] for r in range(3)]) / D
        dy = _det3([[J[r][0], F[r], J[r][2]] for r in range(3)]) / D
        dz = _det3([[J[r][0], J[r][1], F[r]] for r in range(3)]) / D
        ok = np.isfinite(dx) & np.isfinite(dy) & np.isfinite(dz)   # a singular Jacobian: keep the point
        x = np.where(ok, x - dx, x)
        y = np.where(ok, y - dy, y)
        z = np.where(ok, z - dz, z)
    for _ in range(CONSTRAINT_STEPS):   # Gauss-Newton on the constraints of E = x X + y Y + z Z + W
        e = [((x * basis[:, 0, i] + y * basis[:, 1, i]) + z * basis[:, 2, i]) + basis[:, 3, i] for i in range(9)]
        F, G, tr, cof = _constraints(e)
        J = [_constraints_along(e, [basis[:, m, i] for i in range(9)], G, tr, cof) for m in range(3)]
        A = [[None] * 3 for _ in range(3)]
        g = [None] * 3
        for a in range(3):
            for b in range(a, 3):
                acc = J[a][0] * J[b][0]
                for k in range(1, 10):
                    acc = acc + J[a][k] * J[b][k]
                A[a][b] = A[b][a] = acc
            acc = J[a][0] * F[0]
            for k in range(1, 10):
                acc = acc + J[a][k] * F[k]
            g[a] = acc
        D = _det3(A)
        dx = _det3([[g[r], A[r][1], A[r][2]] for r in range(3)]) / D
        dy = _det3([[A[r][0], g[r], A[r][2]] for r in range(3)]) / D
        dz = _det3([[A[r][0], A[r][1], g[r]] for r in range(3)]) / D
        ok = np.isfinite(dx) & np.isfinite(dy) & np.isfinite(dz)
        x = np.where(ok, x - dx, x)
        y = np.where(ok, y - dy, y)
        z = np.where(ok, z - dz, z)
    e = [((x * basis[:, 0, i] + y * basis[:, 1, i]) + z * basis[:, 2, i]) + basis[:, 3, i] for i in range(9)]
    ss = np.zeros_like(z)
    for i in range(9):
        ss = ss + e[i] * e[i]
    scale = np.sqrt(2.0 / ss)
    big = np.abs(e[0])
    lead = e[0]
    for i in range(1, 9):
        take = np.abs(e[i]) > big
        big = np.where(take, np.abs(e[i]), big)
        lead = np.where(take, e[i], lead)
    s = np.where(lead < 0.0, -scale, scale)
    return [v * s for v in e]


def solve(a: np.ndarray, b: np.ndarray, item5=None):
    """a, b: (M, 5, 2) K-normalised coordinates of the solved items; item5: (M, 4) = (xa, ya, xb, yb) of the choosing item
    or None.  Returns (candidates (M, 10, 9) NaN-padded in the order of the roots of n, count (M,), degenerate (M,), E (M, 9):
    the candidate with the strictly smallest SED on item 5 (NaN when none; only with item5))."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    M = a.shape[0]
    with np.errstate(all="ignore"):
        basis, degenerate = null_basis(a, b)
        B = gauss_jordan(coefficient_matrix(basis))
        rows, n = hidden_polynomials(B)
        n, dn, chain, ok = sturm_chain(n)
        ok &= ~degenerate
        bound = root_bound(n)
        ok &= np.isfinite(bound)
        bound = np.where(ok, bound, 1.0)
        lo = -bound
        vlo = sign_changes(chain, lo)
        v_end = sign_changes(chain, bound)
        cands = np.full((M, MAX_CANDIDATES, 9), np.nan)
        count = np.zeros(M, dtype=np.int64)
        best = np.full(M, np.inf)
        E = np.full((M, 9), np.nan)
        for slot in range(MAX_CANDIDATES):
            active = ok & (vlo - v_end > 0)
            if not active.any():
                break
            hi = bound.copy()
            vhi = v_end.copy()
            for _ in range(ISOLATE_STEPS):   # the smallest root of (lo, bound] alone in (lo, hi]
                need = active & (vlo - vhi > 1)
                if not need.any():
                    break
                mid = 0.5 * (lo + hi)
                vm = sign_changes(chain, mid)
                left = need & (vlo - vm >= 1)
                right = need & ~(vlo - vm >= 1)
                hi = np.where(left, mid, hi)
                vhi = np.where(left, vm, vhi)
                lo = np.where(right, mid, lo)
                vlo = np.where(right, vm, vlo)
            # Newton inside the bracket (lo, hi]
            ba, bb = lo.copy(), hi.copy()
            fa = _horner(n, ba)
            z = 0.5 * (ba + bb)
            run = active.copy()
            for _ in range(POLISH_STEPS):
                if not run.any():
                    break
                f = _horner(n, z)
                df = _horner(dn, z)
                hit = f == 0.0
                same = f * fa > 0.0
                ba = np.where(run & same, z, ba)
                fa = np.where(run & same, f, fa)
                bb = np.where(run & ~same, z, bb)
                zn = z - f / df
                conv = np.abs(zn - z) <= 1e-15 * np.abs(z)   # a Newton step at the rounding level: done
                zn = np.where(((zn > ba) & (zn < bb)) | conv, zn, 0.5 * (ba + bb))
                z = np.where(run & ~hit, zn, z)
                run &= ~hit & ~conv
            e = _candidate(basis, rows, z)
            ev = np.stack(e, axis=1)
            cands[active, slot] = ev[active]
            count += active
            if item5 is not None:
                sed = sed_value(e, item5[:, 0], item5[:, 1], item5[:, 2], item5[:, 3])
                take = active & (sed < best)
                best = np.where(take, sed, best)
                E = np.where(take[:, None], ev, E)
            lo = np.where(active, hi, lo)
            vlo = np.where(active, vhi, vlo)
    return cands, count, degenerate, E


def fit_corr(corr: np.ndarray, S: np.ndarray):
    """corr (N, 4) K-normalised {xa, ya, xb, yb}; S (H, >= 6) sample indices -> (E (H, 9), flags (H,) int32), the device
    fit's contract: flag 1 (SFM_FIT_DEGENERATE) for an index out of range or a degenerate sample, 9 NaNs for no solution."""
    corr = np.asarray(corr, dtype=np.float64)
    S = np.asarray(S)[:, :6].astype(np.int64)
    n = corr.shape[0]
    bad = np.any((S < 0) | (S >= n), axis=1)
    pts = corr[np.where(bad[:, None], 0, S)]
    _, _, degenerate, E = solve(pts[:, :5, 0:2], pts[:, :5, 2:4], pts[:, 5])
    flags = (degenerate | bad).astype(np.int32)
    E[flags != 0] = np.nan
    return E, flags


def candidates_corr(corr: np.ndarray, S: np.ndarray):
    """Every candidate of each sample: (cands (H, 10, 9) NaN-padded, count (H,)); degenerate samples have none."""
    corr = np.asarray(corr, dtype=np.float64)
    S = np.asarray(S)[:, :6].astype(np.int64)
    n = corr.shape[0]
    bad = np.any((S < 0) | (S >= n), axis=1)
    pts = corr[np.where(bad[:, None], 0, S)]
    cands, count, degenerate, _ = solve(pts[:, :5, 0:2], pts[:, :5, 2:4])
    drop = degenerate | bad
    cands[drop] = np.nan
    count[drop] = 0
    return cands, count


def five_point(coords_a: np.ndarray, coords_b: np.ndarray) -> np.ndarray:
    """E (3, 3) from six K-normalised pairs (rows 0-4 solved, row 5 chooses); raises ``Degenerate`` for a degenerate sample.
    NaNs when the sample has no real solution."""
    a = np.asarray(coords_a, dtype=np.float64).reshape(1, 6, 2)
    b = np.asarray(coords_b, dtype=np.float64).reshape(1, 6, 2)
    item5 = np.concatenate([a[:, 5], b[:, 5]], axis=1)
    _, _, degenerate, E = solve(a[:, :5], b[:, :5], item5)
    if degenerate[0]:
        raise Degenerate("the five-point system has numerical rank < 5")
    return E[0].reshape(3, 3)
