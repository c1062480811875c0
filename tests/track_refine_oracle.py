"""NumPy definition of the sub-pixel refinement of track observations (csrc/sfm_track_refine.hip).

All arithmetic is float64 with + - * / and sqrt in the order written here and no libm, so the device is compared byte for byte.

  window     n = (2r+1)^2 samples, sample k = row * (2r+1) + col at offset (dx, dy) = (col - r, row - r)
  sums       every sum over the window has one order: the values are laid out in 64 * SPL slots, SPL = ceil(n / 64), slot k
             holding sample k and 0.0 beyond n; lane l = k mod 64 adds its slots l, l + 64, ... in ascending order; the 64 lane
             sums are then combined by s = s + s[lane xor m] for m = 32, 16, 8, 4, 2, 1.  A mean is the sum divided by float(n).
  bilinear   x0 = min(floor(u), W - 2), fx = u - x0 (the same in y), top = p00 + fx (p10 - p00), bot = p01 + fx (p11 - p01),
             top + fy (bot - top): section 6ai's formula; the min matters only when u + 1 rounds up to W - 1
  template   the grey values around the reference's integer pixel; T = (g - mean) / sqrt(sum (g - mean)^2)
  iteration  u = t0 + (A00 dx + A01 dy), v = t1 + (A10 dx + A11 dy); every sample needs 1 <= u < W - 2 and 1 <= v < H - 2;
             I = bilinear(u, v), gx = 0.5 (bilinear(u + 1, v) - bilinear(u - 1, v)), gy likewise; I0 = I - mean(I),
             s = sqrt(sum I0^2), res = T - I0 / s; J_c = (gx, gy, gx dx, gx dy, gy dx, gy dy)_c / s less its mean;
             H = sum J J^T, b = sum J res, H_ii += 1e-9 trace(H) (the trace added from H_00 up); Cholesky with every sum by
             sequential subtraction (csrc/sfm_lm.h factor<6> with rel = 0 / solve<6>); t += delta[0:2], A += delta[2:6]
  statuses   see ``refine``; every status but OK returns the integer input position and warp0
"""
import numpy as np

OK, REFERENCE, BAD_INDEX, OUTSIDE, FLAT, SINGULAR, DIVERGED, LOW_CORRELATION = range(8)
STATUS_NAMES = ("ok", "reference", "bad_index", "outside", "flat", "singular", "diverged", "low_correlation")
WAVE = 64
_LANES = np.arange(WAVE)
F = np.float64


def window_sum(p):
    """The sum of each row of ``p`` [m, 64 * SPL] (or of one vector) in the definition's order."""
    p = np.asarray(p, dtype=F)
    single = p.ndim == 1
    p = p.reshape(1, -1) if single else p
    acc = p[:, :WAVE].copy()
    for j in range(1, p.shape[1] // WAVE):
        acc = acc + p[:, WAVE * j:WAVE * (j + 1)]
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, _LANES ^ m]
    return acc[0, 0] if single else acc[:, 0].copy()


def bilinear(image, u, v):
    """``image`` int64 / float64 [H, W]; u, v float64 arrays inside 0 <= u <= W - 1, 0 <= v <= H - 1."""
    H, W = image.shape
    xf, yf = np.minimum(np.floor(u), F(W - 2)), np.minimum(np.floor(v), F(H - 2))
    fx, fy = u - xf, v - yf
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    p00, p10, p01, p11 = (image[y0, x0].astype(F), image[y0, x0 + 1].astype(F), image[y0 + 1, x0].astype(F),
                          image[y0 + 1, x0 + 1].astype(F))
    top = p00 + fx * (p10 - p00)
    bot = p01 + fx * (p11 - p01)
    return top + fy * (bot - top)


def factor(A):
    """(ok, L) of csrc/sfm_lm.h factor<6> with rel = 0."""
    N = len(A)
    L = np.zeros((N, N), dtype=F)
    ok = True
    for j in range(N):
        s = A[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        ok = ok and bool(s > F(0.0) * A[j, j])
        L[j, j] = np.sqrt(np.fmax(s, F(0.0)))
        for i in range(j + 1, N):
            x = A[i, j]
            for k in range(j):
                x = x - L[i, k] * L[j, k]
            L[i, j] = x / L[j, j]
    return ok, L


def solve(L, b):
    """(finite, x) of csrc/sfm_lm.h solve<6>."""
    N = len(b)
    y, x = np.zeros(N, dtype=F), np.zeros(N, dtype=F)
    for j in range(N):
        v = b[j]
        for k in range(j):
            v = v - L[j, k] * y[k]
        y[j] = v / L[j, j]
    for j in range(N - 1, -1, -1):
        v = y[j]
        for k in range(j + 1, N):
            v = v - L[k, j] * x[k]
        x[j] = v / L[j, j]
    return bool(np.all(np.isfinite(x))), x


class Window:
    def __init__(self, radius):
        side = 2 * radius + 1
        self.n = side * side
        self.slots = WAVE * ((self.n + WAVE - 1) // WAVE)
        k = np.arange(self.n)
        self.col, self.row = k % side - radius, k // side - radius
        self.dx, self.dy = self.col.astype(F), self.row.astype(F)
        self.count = F(self.n)

    def pad(self, values):
        """[..., n] -> [..., slots] with 0.0 beyond n."""
        values = np.asarray(values, dtype=F)
        out = np.zeros(values.shape[:-1] + (self.slots,), dtype=F)
        out[..., :self.n] = values
        return out

    def sum(self, values):
        return window_sum(self.pad(values))

    def centre(self, values):
        """(values - mean, sum of its squares)"""
        centred = values - self.sum(values) / self.count
        return centred, self.sum(centred * centred)


def _positions(w, t, A, W, H):
    u = t[0] + (A[0] * w.dx + A[1] * w.dy)
    v = t[1] + (A[2] * w.dx + A[3] * w.dy)
    with np.errstate(invalid="ignore"):
        inside = (F(1.0) <= u) & (u < F(W - 2)) & (F(1.0) <= v) & (v < F(H - 2))
    return u, v, bool(np.all(inside))


def refine_one(image, x, y, ref_image, xq, yq, warp0, radius, max_iterations, min_step, max_shift, min_correlation, window=None):
    """One observation against its reference -> (status, (x, y), warp [4], correlation, iterations).  ``image`` / ``ref_image``:
    uint8 planes; the pixels are inside their planes (``refine`` checks that)."""
    w = Window(radius) if window is None else window
    warp0 = np.asarray(warp0, dtype=F).reshape(4)
    start = (F(x), F(y))
    nan = F(np.nan)

    def stop(status, correlation=nan, solves=0):
        return status, start, warp0.copy(), correlation, solves

    Hq, Wq = ref_image.shape
    if xq - radius < 0 or xq + radius > Wq - 1 or yq - radius < 0 or yq + radius > Hq - 1:
        return stop(OUTSIDE)
    g = ref_image[yq + w.row, xq + w.col].astype(F)
    T, ss = w.centre(g)
    if ss == 0.0:
        return stop(FLAT)
    T = T / np.sqrt(ss)
    img = np.asarray(image)
    H, W = img.shape
    t = [start[0], start[1]]
    A = warp0.copy()
    min_step2, max_shift2 = F(min_step) * F(min_step), F(max_shift) * F(max_shift)
    one, half = F(1.0), F(0.5)
    solves = 0
    with np.errstate(all="ignore"):
        for _ in range(max_iterations):
            u, v, inside = _positions(w, t, A, W, H)
            if not inside:
                return stop(OUTSIDE, solves=solves)
            I = bilinear(img, u, v)
            gx = half * (bilinear(img, u + one, v) - bilinear(img, u - one, v))
            gy = half * (bilinear(img, u, v + one) - bilinear(img, u, v - one))
            I0, ss = w.centre(I)
            if ss == 0.0:
                return stop(FLAT, solves=solves)
            s = np.sqrt(ss)
            res = T - I0 / s
            J = np.stack([gx / s, gy / s, gx * w.dx / s, gx * w.dy / s, gy * w.dx / s, gy * w.dy / s])
            J = J - (w.sum(J) / w.count)[:, None]
            pairs = [(c, d) for c in range(6) for d in range(c, 6)]
            sums = w.sum(np.stack([J[c] * J[d] for c, d in pairs] + [J[c] * res for c in range(6)]))
            Hm = np.zeros((6, 6), dtype=F)
            for (c, d), value in zip(pairs, sums[:21]):
                Hm[c, d] = Hm[d, c] = value
            b = sums[21:]
            trace = Hm[0, 0]
            for c in range(1, 6):
                trace = trace + Hm[c, c]
            ridge = F(1e-9) * trace
            for c in range(6):
                Hm[c, c] = Hm[c, c] + ridge
            ok, L = factor(Hm)
            if not ok:
                return stop(SINGULAR, solves=solves)
            finite, delta = solve(L, b)
            if not finite:
                return stop(SINGULAR, solves=solves)
            solves += 1
            t = [t[0] + delta[0], t[1] + delta[1]]
            A = A + delta[2:]
            sx, sy = t[0] - start[0], t[1] - start[1]
            if sx * sx + sy * sy > max_shift2:
                return stop(DIVERGED, solves=solves)
            if delta[0] * delta[0] + delta[1] * delta[1] < min_step2:
                break
        u, v, inside = _positions(w, t, A, W, H)
        if not inside:
            return stop(OUTSIDE, solves=solves)
        I0, ss = w.centre(bilinear(img, u, v))
        if ss == 0.0:
            return stop(FLAT, solves=solves)
        correlation = w.sum(T * (I0 / np.sqrt(ss)))
    if correlation >= F(min_correlation):
        return OK, (t[0], t[1]), A, correlation, solves
    return stop(LOW_CORRELATION, correlation, solves)


class Result:
    def __init__(self, M):
        self.xy = np.zeros((M, 2), dtype=F)
        self.warp = np.zeros((M, 4), dtype=F)
        self.correlation = np.zeros(M, dtype=F)
        self.iterations = np.zeros(M, dtype=np.int32)
        self.status = np.zeros(M, dtype=np.int32)

    def arrays(self):
        return {"xy": self.xy, "warp": self.warp, "correlation": self.correlation, "iterations": self.iterations,
                "status": self.status}


def refine(planes, plane, x, y, reference, warp0, radius=7, max_iterations=10, min_step=1e-3, max_shift=3.0, min_correlation=0.8):
    """The definition of ``sfm_refine_observations``.  ``planes``: the uint8 planes in table order; the other arguments as the
    entry point takes them."""
    plane, x, y, reference = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (plane, x, y, reference))
    warp0 = np.asarray(warp0, dtype=F).reshape(-1, 4)
    M = len(plane)
    out = Result(M)
    w = Window(radius)

    def inside(p, px, py):
        return 0 <= p < len(planes) and 0 <= px < planes[p].shape[1] and 0 <= py < planes[p].shape[0]

    for o in range(M):
        q = int(reference[o])
        record = (BAD_INDEX, (F(x[o]), F(y[o])), warp0[o].copy(), F(np.nan), 0)
        if q == o or q == -1:
            record = (REFERENCE,) + record[1:]
        elif 0 <= q < M and inside(int(plane[o]), int(x[o]), int(y[o])) and inside(int(plane[q]), int(x[q]), int(y[q])):
            record = refine_one(planes[plane[o]], int(x[o]), int(y[o]), planes[plane[q]], int(x[q]), int(y[q]), warp0[o], radius,
                                max_iterations, min_step, max_shift, min_correlation, w)
        out.status[o], out.xy[o], out.warp[o], out.correlation[o], out.iterations[o] = record
    return out
