"""NumPy definition of the similarity alignment (csrc/sfm_similarity.h, csrc/sfm_similarity.hip): the
least-squares model of a set computed two ways — by the SVD with the determinant correction (Umeyama 1991) and by the
eigenvector of Horn's 4 x 4 quaternion matrix (Horn 1987) —, the error of a pair in the device's operation order, scoring, gate,
aggregation and selection by the rules of the other oracles, the Philox sampler, and the refit rounds.

A model is 13 doubles: R row-major (9) | t (3) | s, with b ~ s R a + t."""
import numpy as np

from oracle import sfm_oracle as orc

SAMPLE = 3
MODEL = 13
DEGENERATE_FLOOR = 1e-9
FIT_DEGENERATE = 1   # SFM_FIT_DEGENERATE


# ---- the model of a set ---------------------------------------------------------------------------------------------------
def moments(a, b):
    """(M, sa2, sb2, mu_a, mu_b) of paired (k, 3) arrays: M = sum b' a'^T."""
    mua, mub = a.mean(axis=0), b.mean(axis=0)
    da, db = a - mua, b - mub
    return db.T @ da, float(np.sum(da * da)), float(np.sum(db * db)), mua, mub


def _finish(R, trace, d, sa2, sb2, mua, mub):
    with np.errstate(all="ignore"):
        s = np.float64(trace) / np.float64(sa2)
        t = mub - s * (R @ mua)
        model = np.concatenate([R.reshape(9), t, [s]])
        ok = d > DEGENERATE_FLOOR * np.sqrt(sa2 * sb2) and sa2 > 0.0 and s > 0.0 and np.isfinite(s) and np.all(np.isfinite(model))
        ratio = np.float64(d) / np.sqrt(np.float64(sa2) * sb2)
    return model, (0 if ok else FIT_DEGENERATE), float(ratio)


def model_svd(a, b):
    """(model, flag, d / sqrt(sa2 sb2)) by the SVD of M with the determinant correction."""
    M, sa2, sb2, mua, mub = moments(a, b)
    if not np.all(np.isfinite(M)):
        return np.full(MODEL, np.nan), FIT_DEGENERATE, float("nan")
    U, sig, Vt = np.linalg.svd(M)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0])
    R = U @ D @ Vt
    det = np.linalg.det(M)
    d = sig[1] + (np.sign(det) * sig[2] if det != 0.0 else 0.0)
    return _finish(R, float(np.sum(R * M)), d, sa2, sb2, mua, mub)


def model_horn(a, b):
    """The same by the eigenvector of the largest eigenvalue of Horn's matrix; d is half the gap to the second largest."""
    M, sa2, sb2, mua, mub = moments(a, b)
    if not np.all(np.isfinite(M)):
        return np.full(MODEL, np.nan), FIT_DEGENERATE, float("nan")
    S = M.T   # S[i][j] = sum a'_i b'_j
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, V = np.linalg.eigh(N)
    q0, qx, qy, qz = V[:, 3] / np.linalg.norm(V[:, 3])
    R = np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                  [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                  [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])
    return _finish(R, float(np.sum(R * M)), 0.5 * (w[3] - w[2]), sa2, sb2, mua, mub)


def model_parts(model):
    return float(model[12]), model[:9].reshape(3, 3), model[9:12]


def model_gap(m1, m2, pairs):
    """How far two models of the same data are apart: max |dR|, |ds| / s and |dt| over the natural length of side B
    (the largest of |t|, s max |a| and max |b|)."""
    s1, R1, t1 = model_parts(m1)
    s2, R2, t2 = model_parts(m2)
    length = max(np.max(np.abs(t2)), s2 * np.max(np.abs(pairs[:, :3])), np.max(np.abs(pairs[:, 3:])), 1e-300)
    return max(float(np.max(np.abs(R1 - R2))), abs(s1 - s2) / s2, float(np.max(np.abs(t1 - t2))) / length)


def fit(pairs, S, route=model_svd):
    """Models (h, 13), flags (h,) and the degeneracy ratios d / sqrt(sa2 sb2) of the samples S[:, :3] of pairs (n, 6); a row
    with an index outside [0, n) is flagged."""
    n = len(pairs)
    models, flags, ratios = np.full((len(S), MODEL), np.nan), np.zeros(len(S), dtype=np.int32), np.zeros(len(S))
    for k, row in enumerate(np.asarray(S)[:, :SAMPLE]):
        bad = np.any((row < 0) | (row >= n))
        idx = np.where((row < 0) | (row >= n), 0, row)
        models[k], flags[k], ratios[k] = route(pairs[idx, :3], pairs[idx, 3:])
        if bad:
            flags[k] = FIT_DEGENERATE
    return models, flags, ratios


# ---- the error, in the device's operation order -----------------------------------------------------------------------------
def error(model, pairs):
    """e of every pair (n, 6) under one model: p_k = (R[3k] ax + R[3k+1] ay) + R[3k+2] az, r_k = (s p_k + t_k) - b_k,
    e = (r_0^2 + r_1^2) + r_2^2, each operation rounded on its own."""
    m = np.asarray(model, dtype=np.float64)
    ax, ay, az, bx, by, bz = (pairs[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        p0 = (m[0] * ax + m[1] * ay) + m[2] * az
        p1 = (m[3] * ax + m[4] * ay) + m[5] * az
        p2 = (m[6] * ax + m[7] * ay) + m[8] * az
        r0 = (m[12] * p0 + m[9]) - bx
        r1 = (m[12] * p1 + m[10]) - by
        r2 = (m[12] * p2 + m[11]) - bz
        return (r0 * r0 + r1 * r1) + r2 * r2


def _sequential_sum(values):
    """The sum of `values` added one by one from 0.0, as a lane of the device adds them."""
    with np.errstate(all="ignore"):
        return float(np.cumsum(values)[-1]) if len(values) else 0.0


def score_table(pairs, models, S, thr):
    """(cnt, s1, s2) of every hypothesis in the device's summation order: every item with e <= thr in item order, then each
    sample item in sample order — one that passed leaves the count, one that did not enters the sums."""
    h = len(models)
    cnt, s1, s2 = np.zeros(h, dtype=np.int32), np.zeros(h), np.zeros(h)
    n = len(pairs)
    for k in range(h):
        e = error(models[k], pairs)
        with np.errstate(invalid="ignore"):
            passed = e <= thr
        c, a1 = int(np.count_nonzero(passed)), _sequential_sum(e[passed])
        with np.errstate(all="ignore"):
            a2 = _sequential_sum(e[passed] * e[passed])
            for i in S[k, :SAMPLE]:
                i = int(i) if 0 <= i < n else 0
                if passed[i]:
                    c -= 1
                else:
                    a1 = a1 + e[i]
                    a2 = a2 + e[i] * e[i]
        cnt[k], s1[k], s2[k] = c, a1, a2
    return cnt, s1, s2


def aggregate(cnt, s1, s2, method, sample=SAMPLE):
    """ransac.py's aggregation on (count, sum, sum of squares) with `sample` sample items; method 0 sum, 1 square, 2 mean, 3 rms."""
    nn = np.asarray(cnt, dtype=np.float64) + float(sample)
    with np.errstate(all="ignore"):
        return [s1, s2, s1 / nn, np.sqrt(s2 / nn)][method]


def select(cnt, s1, s2, flags, min_extra, method):
    """The host rule: lowest aggregated error among hypotheses with cnt >= min_extra, a finite error and no flag; earliest
    index on ties.  Returns (best index or -1, its error or inf)."""
    err = aggregate(cnt, s1, s2, method)
    with np.errstate(invalid="ignore"):
        ok = (cnt >= min_extra) & (err < np.inf) & (flags == 0)
    if not ok.any():
        return -1, np.inf
    best = int(np.argmin(np.where(ok, err, np.inf)))
    return best, float(err[best])


def mask(pairs, models, S, best, thr):
    """uint8 (n,): 2 for the three sample items of hypothesis ``best``, 1 other items with e <= thr, 0 otherwise; all zero for
    best < 0."""
    out = np.zeros(len(pairs), dtype=np.uint8)
    if best < 0:
        return out
    with np.errstate(invalid="ignore"):
        out[error(models[best], pairs) <= thr] = 1
    out[S[best, :SAMPLE]] = 2
    return out


# ---- the sampler ------------------------------------------------------------------------------------------------------------
def sample_table(seed, h_begin, h_count, n):
    """Rows of philox_sample8(seed, h_begin + h) as the fit launch stores them: the first min(8, n) positions of the
    Fisher-Yates shuffle of range(n) (oracle/sfm_oracle.py::philox_sample_table, which this is for n >= 8), -1 behind them."""
    seed &= 2**64 - 1
    if n >= 8:
        return orc.philox_sample_table(seed, h_begin, h_count, n)
    h = np.arange(h_begin, h_begin + h_count, dtype=np.uint64)
    ctr = np.zeros((h_count, 4), dtype=np.uint32)
    ctr[:, 0] = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (h >> np.uint64(32)).astype(np.uint32)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = []
    for block in (0, 1):
        ctr[:, 2] = block
        words.append(orc.philox4x32_10(ctr, key))
    u = np.concatenate(words, axis=1).astype(np.uint64)
    S = np.full((h_count, 8), -1, dtype=np.int32)
    for row in range(h_count):
        order = list(range(n))
        for k in range(n):
            j = k + int((int(u[row, k]) * (n - k)) >> 32)
            order[k], order[j] = order[j], order[k]
            S[row, k] = order[k]
    return S


# ---- the refit rounds -------------------------------------------------------------------------------------------------------
def refit_wins(count, err, best_count, best_err):
    return count > best_count or (count == best_count and err < best_err)


def refine(pairs, model_in, mask_in, err_in, thr, method, rounds, route=model_svd):
    """sfm_similarity_refine of one entry -> (model_out, mask_out, info dict)."""
    best, keep = np.array(model_in, dtype=np.float64), (np.asarray(mask_in) != 0).astype(np.uint8)
    best_err, accepted, rounds_run = float(err_in), 0, 0
    for _ in range(rounds):
        idx = np.nonzero(keep)[0]
        if len(idx) < SAMPLE:
            break
        rounds_run += 1
        model, flag, _ = route(pairs[idx, :3], pairs[idx, 3:])
        if flag:
            break
        e = error(model, pairs)
        with np.errstate(invalid="ignore"):
            passed = e <= thr
        count = int(np.count_nonzero(passed))
        err = float(aggregate(np.array([count]), np.array([np.sum(e[passed])]), np.array([np.sum(e[passed] ** 2)]), method, 0)[0])
        if not refit_wins(count, err, int(np.count_nonzero(keep)), best_err):
            break
        best, keep, best_err, accepted = model, passed.astype(np.uint8), err, accepted + 1
    return best, keep, dict(error=best_err, count=int(np.count_nonzero(keep)), accepted=accepted, rounds_run=rounds_run)


def pass_outcome(pairs, seed, h_begin, h_count, thr, min_extra, method):
    """One whole pass on the host: (S, models, flags, cnt, s1, s2, best, err, mask)."""
    S = sample_table(seed, h_begin, h_count, len(pairs))
    models, flags, _ = fit(pairs, S)
    cnt, s1, s2 = score_table(pairs, models, S, thr)
    best, err = select(cnt, s1, s2, flags, min_extra, method)
    return S, models, flags, cnt, s1, s2, best, err, mask(pairs, models, S, best, thr)
