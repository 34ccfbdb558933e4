"""Cases and the numpy oracle of the sparse-GP gene test (csrc/gene_gp.hip, utilities.gene_spatial_gp), shared by
test_gene_gp_cases.py (CPU), test_hip_gene_gp.py and test_gene_gp_api.py (GPU).  Nothing here touches a GPU; the chunk of
the projection and the tolerance of the refinement are read from the library's host-only plan queries.

The oracle is dense fp64 numpy: K_zx, Phi = Lz^-1 K_zx, eigh(Phi Phi^T), the profiled bound F(t), t = log delta, its maximum
by a 2001-point scan and bisection on dF/dt.  Projections come three ways: ``P_ref`` (every sum by math.fsum), ``P_emu`` (the
device's order emulated: separately rounded products added sequentially inside a chunk of the row, the chunks folded in
order) and, in the GPU tests, the device's.

The tolerances are measured here, not chosen:
  RTOL_P  3 x the worst |P_emu - P_ref| / sum |v k| over every sum of every case
  RTOL_F  3 x the worst |F_emu - F_ref| / N at the oracle's optimum, F_emu the oracle's bound on the emulated projections
"""
import functools
import math

import numpy as np

D = 48
JITTER = 1e-6
DELTA_MAX = 1e6
SCAN = 2001
KIND_ID = {"rbf": 0, "matern32": 1, "matern12": 4, "matern52": 5}

# delta_min: the default 1e-3 where the noise-free gene reaches it.  Elsewhere the trace term N - sum lam of these few
# inducing points keeps every optimum above it (1.4e-3 in the smallest case, 5e-3 under Matern-3/2): those cases search from a
# delta_min just above that, so that every case has an optimum at the lower bound
#        name              N     M   d  n_ell  kernel     delta_min
CASES = {
    "n65_m8_d1":       (65,    8,  1, 1, "rbf",      2e-3),
    "n257_m63_d2":     (257,  63,  2, 4, "matern32", 1e-1),
    "n257_m64_d3":     (257,  64,  3, 4, "rbf",      1e-3),
    "n1037_m65_d2":    (1037, 65,  2, 9, "rbf",      1e-3),
    "n1037_m129_d2":   (1037, 129, 2, 4, "matern32", 1e-1),
}
API_CASE = "n257_m63_d2"

# gene rows
EMPTY, ONE, FULL, CONST, CHUNK_M1, CHUNK_0, CHUNK_P1 = 0, 1, 2, 3, 4, 5, 6
NOISE = tuple(range(7, 16))            # Poisson noise, three means x three draws
PLANTED = tuple(range(16, 46))         # planted structure: three length scales x two amplitudes x five draws
SMOOTH = 46                            # noise-free, in the span of the inducing points
HUGE = 47


def _fma(a, b, c):
    """a * b + c with one rounding (Dekker's product, Knuth's sum), vectorised: the device's fma in the squared distance."""
    p = a * b
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    es = (p - (s - bb)) + (c - bb)
    return s + (es + e)


def kernel_matrix(kind, ell, Z, X):
    """k_ell(Z, X) (M, N) of unit variance with the device's operations in its order (cov.h, CovF64)."""
    d = Z.shape[1]
    acc = np.zeros((Z.shape[0], X.shape[0]))
    for k in range(d):
        df = Z[:, k][:, None] - X[:, k][None, :]
        acc = _fma(df, df, acc)
    if kind == "rbf":
        return np.exp((-0.5 / (ell * ell)) * acc)
    r = np.sqrt(acc)
    if kind == "matern12":
        return np.exp(-((1.0 / ell) * r))
    cf = (1.7320508075688772935 if kind == "matern32" else 2.2360679774997896964) / ell
    t = cf * r
    lin = _fma(np.full_like(r, cf), r, np.ones_like(r))
    if kind == "matern32":
        return lin * np.exp(-t)
    return (lin + t * t / 3.0) * np.exp(-t)


def default_lengthscales(X, M, n):
    side = X.max(axis=0) - X.min(axis=0)
    h = float(np.exp(np.log(side).sum() / X.shape[1])) / M ** (1.0 / X.shape[1])
    top = 0.5 * float(side.max())
    if n == 1:
        return np.array([math.sqrt(h * top)])
    return np.exp(np.linspace(math.log(h), math.log(top), n))


def plan_chunk(N, nnz, M, n_ell):
    from gpzoo_amd import ops
    return ops.gene_kernel_project_plan(N, D, max(nnz, 0), M, n_ell)["gene_chunk"]


def plan_tol_t(M, n_ell):
    from gpzoo_amd import ops
    return ops.gene_gp_profile_plan(D, M, n_ell)["tol_t"]


@functools.lru_cache(maxsize=None)
def build_case(name):
    """Coordinates, inducing points, length scales and the (D, N) fp32 values (a zero is not stored) of a case."""
    N, M, d, n_ell, kind, delta_min = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20261021)
    X = rng.random((N, d))
    Z = X[rng.choice(N, M, replace=False)] + 1e-3 * rng.standard_normal((M, d))
    ell = default_lengthscales(X, M, n_ell)
    chunk = plan_chunk(N, 0, M, n_ell)
    V = np.zeros((D, N))

    def some(n):
        return rng.choice(N, min(n, N), replace=False)

    V[ONE, some(1)] = 1.75
    V[FULL] = 0.25 + rng.random(N)
    V[CONST] = 2.0
    for g, n in ((CHUNK_M1, chunk - 1), (CHUNK_0, chunk), (CHUNK_P1, chunk + 1)):
        idx = some(n)
        V[g, idx] = np.log1p(1.0 + rng.poisson(1.0, idx.size))
    for j, g in enumerate(NOISE):
        V[g] = np.log1p(rng.poisson((0.05, 0.5, 5.0)[j % 3], N))
    planted = ell[[0, n_ell // 2, n_ell - 1]] if n_ell > 1 else ell[0] * np.array([0.7, 1.0, 1.4])
    planted_ell = {}
    for j, g in enumerate(PLANTED):
        lp = planted[j % 3]
        amp = (1.0, 2.0)[(j // 3) % 2]
        K = kernel_matrix("rbf", lp, X, X) + 1e-6 * np.eye(N)
        f = np.linalg.cholesky(K) @ rng.standard_normal(N)
        f -= f.mean()
        V[g] = np.log1p(rng.poisson(np.exp(math.log(2.0 if N > 100 else 8.0) + amp * f)))
        planted_ell[g] = (0, n_ell // 2, n_ell - 1)[j % 3]
    w = rng.standard_normal(M)
    f = w @ kernel_matrix(kind, ell[-1], Z, X)
    V[SMOOTH] = f - f.min() + 0.125
    V[HUGE, some(1)] = 3.0e4
    V = V.astype(np.float32)
    return dict(name=name, N=N, M=M, d=d, n_ell=n_ell, kernel=kind, X=X, Z=Z, ell=ell, V=V, chunk=chunk, planted_ell=planted_ell,
                delta_range=(delta_min, DELTA_MAX))


def F_terms(t, p2, lam, yy, N):
    """(F, Q, g, dg) of the profiled bound at t = log delta (arrays broadcast over a leading axis of t)."""
    t = np.asarray(t, dtype=np.float64)[..., None]
    dl = np.exp(t)
    w = 1.0 / (dl + lam)
    s1, s2, s3 = (p2 * w).sum(-1), (p2 * w * w).sum(-1), (p2 * w * w * w).sum(-1)
    l1, l2, lg = (lam * w).sum(-1), (lam * w * w).sum(-1), np.log(dl + lam).sum(-1)
    dl, t = dl[..., 0], t[..., 0]
    c = N - lam.sum()
    M = lam.size
    with np.errstate(invalid="ignore", divide="ignore"):
        Q = yy - s1
        F = -0.5 * (N * math.log(2 * math.pi) + N * np.log(Q / (dl * N)) + N + (N - M) * t + lg + c / dl)
        u = dl * s2 / Q
        g = N * u - l1 - c / dl
        dg = N * (u - 2 * dl * dl * s3 / Q - u * u) + dl * l2 + c / dl
    return F, Q, g, dg


def null_loglik(yy, N):
    return -0.5 * N * (math.log(2 * math.pi * yy / N) + 1.0)


def maximise(p2, lam, yy, N, t_lo, t_hi):
    """The oracle's optimum of one (gene, length scale): dict(status, t, F, s2, tau2, curvature, near_tied)."""
    out = dict(status=3, t=math.nan, F=math.nan, s2=math.nan, tau2=math.nan, curvature=math.nan, near_tied=False)
    if not (yy > 0 and math.isfinite(yy)):
        return out
    ts = np.linspace(t_lo, t_hi, SCAN)
    F, Q, _, _ = F_terms(ts, p2, lam, yy, N)
    if not (np.all(Q > 0) and np.all(np.isfinite(F))):
        return out
    i = int(np.argmax(F))
    left = np.concatenate(([True], F[1:] > F[:-1]))
    right = np.concatenate((F[:-1] >= F[1:], [True]))
    peaks = np.sort(F[left & right])[::-1]
    out["near_tied"] = bool(peaks.size >= 2 and peaks[0] - peaks[1] <= 1e-6 * N)
    one = lambda t: [float(v) for v in F_terms(t, p2, lam, yy, N)]
    if i == 0 and one(t_lo)[2] >= 0:
        t, st = t_lo, 2
    elif i == SCAN - 1 and one(t_hi)[2] <= 0:
        t, st = t_hi, 1
    else:
        a, b = ts[max(i - 1, 0)], ts[min(i + 1, SCAN - 1)]
        for _ in range(200):                   # g < 0 below the maximum, > 0 above it
            t = 0.5 * (a + b)
            if one(t)[2] < 0:
                a = t
            else:
                b = t
            if b - a <= 1e-13:
                break
        t, st = 0.5 * (a + b), 0
    Fv, Qv, _, dg = one(t)
    dl = math.exp(t)
    out.update(status=st, t=t, F=Fv, s2=Qv / (dl * N), tau2=Qv / N, curvature=0.25 * dg)
    return out


def _project(K, rows, how, chunk):
    """sum_{stored} v k for one gene: K (M, nnz_g) its columns in row order, rows the values."""
    terms = K * rows[None, :]
    if how == "fsum":
        return np.array([math.fsum(r) for r in terms]), np.abs(terms).sum(axis=1)
    n = terms.shape[1]
    if n == 0:
        return np.zeros(K.shape[0]), np.zeros(K.shape[0])
    parts = [np.cumsum(terms[:, s:s + chunk], axis=1)[:, -1] for s in range(0, n, chunk)]
    tot = 0.0 + parts[0]
    for q in parts[1:]:
        tot = tot + q
    return tot, None


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Everything the tests compare against, computed once per session."""
    c = build_case(name)
    N, M, n_ell, kind = c["N"], c["M"], c["n_ell"], c["kernel"]
    V = c["V"].astype(np.float64)
    offset = V.sum(axis=1) / N
    Y = V - offset[:, None]
    yty = (Y * Y).sum(axis=1)
    t_lo, t_hi = (math.log(v) for v in c["delta_range"])
    P_ref = np.zeros((n_ell, D, M))
    P_emu = np.zeros((n_ell, D, M))
    P_abs = np.zeros((n_ell, D, M))
    lam = np.zeros((n_ell, M))
    p_ref = np.zeros((n_ell, D, M))
    p_emu = np.zeros((n_ell, D, M))
    gamma = np.zeros(n_ell)
    cond = np.zeros(n_ell)
    stored = [np.flatnonzero(c["V"][g]) for g in range(D)]
    for l, e in enumerate(c["ell"]):
        K = kernel_matrix(kind, e, c["Z"], c["X"])
        Kzz = kernel_matrix(kind, e, c["Z"], c["Z"]) + JITTER * np.eye(M)
        cond[l] = np.linalg.cond(Kzz)
        Lz = np.linalg.cholesky(Kzz)
        Phi = np.linalg.solve(Lz, K)
        w, U = np.linalg.eigh(Phi @ Phi.T)
        lam[l] = np.clip(w, 0.0, None)
        k1 = K.sum(axis=1)
        phi1 = Phi.sum(axis=1)
        gamma[l] = (lam[l].sum() - phi1 @ phi1 / N) / (N - 1)
        for g in range(D):
            P_ref[l, g], P_abs[l, g] = _project(K[:, stored[g]], V[g, stored[g]], "fsum", c["chunk"])
            P_emu[l, g], _ = _project(K[:, stored[g]], V[g, stored[g]], "emu", c["chunk"])
        R = U.T @ np.linalg.inv(Lz)
        p_ref[l] = (P_ref[l] - offset[:, None] * k1[None, :]) @ R.T
        p_emu[l] = (P_emu[l] - offset[:, None] * k1[None, :]) @ R.T
    keys = ("status", "t", "F", "s2", "tau2", "curvature", "near_tied")
    fit = {k: np.zeros((D, n_ell), dtype=(np.int32 if k == "status" else bool if k == "near_tied" else np.float64)) for k in keys}
    F_emu = np.full((D, n_ell), np.nan)
    for g in range(D):
        for l in range(n_ell):
            r = maximise(p_ref[l, g] ** 2, lam[l], yty[g], N, t_lo, t_hi)
            for k in keys:
                fit[k][g, l] = r[k]
            if r["status"] != 3:
                F_emu[g, l] = float(F_terms(r["t"], p_emu[l, g] ** 2, lam[l], yty[g], N)[0])   # F is flat in t there
    with np.errstate(invalid="ignore", divide="ignore"):
        null = np.where(yty > 0, -0.5 * N * (np.log(2 * math.pi * np.where(yty > 0, yty, 1.0) / N) + 1.0), np.nan)
    best = np.argmax(np.where(np.isnan(fit["F"]), -np.inf, fit["F"]), axis=1)
    return dict(case=c, offset=offset, yty=yty, lam=lam, P_ref=P_ref, P_emu=P_emu, P_abs=P_abs, p_ref=p_ref, p_emu=p_emu, fit=fit,
                F_emu=F_emu, null=null, best=best, gamma=gamma, cond=cond, t_range=(t_lo, t_hi))


def dense_bound(name, g, l, s2, tau2):
    """F(s, tau) = log N(y | 0, s Phi^T Phi + tau I) - (s / 2 tau)(N - sum lam) by the dense N x N evaluation."""
    c = build_case(name)
    o = oracle(name)
    N, M = c["N"], c["M"]
    K = kernel_matrix(c["kernel"], c["ell"][l], c["Z"], c["X"])
    Lz = np.linalg.cholesky(kernel_matrix(c["kernel"], c["ell"][l], c["Z"], c["Z"]) + JITTER * np.eye(M))
    Phi = np.linalg.solve(Lz, K)
    y = c["V"][g].astype(np.float64) - o["offset"][g]
    C = s2 * (Phi.T @ Phi) + tau2 * np.eye(N)
    _, logdet = np.linalg.slogdet(C)
    ll = -0.5 * (N * math.log(2 * math.pi) + logdet + y @ np.linalg.solve(C, y))
    return ll - 0.5 * (s2 / tau2) * (N - (Phi * Phi).sum())


@functools.lru_cache(maxsize=None)
def tolerances():
    """(RTOL_P, RTOL_F), measured over every case."""
    ep, ef = 0.0, 0.0
    for name in CASES:
        o = oracle(name)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(o["P_emu"] - o["P_ref"]) / o["P_abs"]
        ep = max(ep, float(np.nanmax(np.where(o["P_abs"] > 0, rel, 0.0))))
        ef = max(ef, float(np.nanmax(np.abs(o["F_emu"] - o["fit"]["F"]))) / o["case"]["N"])
    return 3.0 * ep, 3.0 * ef


def delta_tolerance(name):
    """(D, n_ell) allowed |t_device - t_oracle|: 10 tol_t plus the shift RTOL_F allows at the oracle's curvature
    (F falls by curvature x shift^2 off the optimum)."""
    o = oracle(name)
    c = o["case"]
    _, rtol_f = tolerances()
    with np.errstate(invalid="ignore", divide="ignore"):
        shift = np.sqrt(rtol_f * c["N"] / np.abs(o["fit"]["curvature"]))
    return 10.0 * plan_tol_t(c["M"], c["n_ell"]) + np.where(np.isfinite(shift), shift, 0.0)
