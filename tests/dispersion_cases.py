"""Seeded cases and the fp64 numpy oracle of the gene-wise negative-binomial dispersion fit (gpzoo_amd/csrc/gene_dispersion.hip,
``utilities.gene_dispersion``).  Everything here runs on the CPU.

Counts (D = 48 genes, N spots) depend on N alone; a case is (N, sizes) with sizes one of ``SIZE_VARIANTS``:

  totals    the spots' total counts                    ones      all ones (the kernel's equal-sizes branch)
  uniform   seeded values in (0.3, 3)                  holes     three spots emptied of all counts, then the totals (the
                                                                 emptied spots have size 0 and contribute nothing)

Gene rows, by index (``row_kinds``):

  empty        no stored entry                                  one        a single count of 3
  every        a count at every spot                            constant   the same count at every spot
  g-1, g, g+1  that many stored entries for the plan's gene_chunk g (gamma-Poisson rows where they do not fit N)
  gp           gamma-Poisson counts, theta in GP_THETAS x mean in MEANS, rate proportional to a seeded spot effect
  poisson      Poisson counts at the same means
  big          counts up to about 3000 at 40 spots (all spots at N = 7), zeros elsewhere
  ge16         a count >= 16 at every spot: every stored entry takes the large-count branch
  spike        one count of 20 000 among zeros
  the rest     gamma-Poisson rows with seeded theta in (0.1, 50) and mean in (0.2, 20)

The oracle evaluates the score, its scale A, the gain and the Poisson log-likelihood from terms that have no cancellation
inside them, with explicit sums over k:

  a_n = theta h(x_n),  h(x) = x / (1 + x) - log1p(x)  [for x <= 1/2: -x^2 / ((1 + x)(2 + x)) - 2 s^3 P(s^2), s = x / (2 + x),
                                                       P(z) = 1/3 + z/5 + ..., from log1p(x) = 2 atanh(s)]
  b_n = theta sum_{k < y} (mu_n - k) / ((theta + k)(theta + mu_n))
  S = sum a_n + sum b_n,   A = sum |a_n| + sum |b_n|,   H = dS/dt (t = log theta) from the derivatives of the same terms
  gain = sum_n theta (x_n - log1p(x_n)) + sum_stored sum_{k < y} log((theta + k) / (theta + mu_n))
  poisson_loglik = sum_stored [y log mu_n - lgamma(y + 1)] - sum y

and finds the root by bisection in t to 1e-13.  ``mp_terms`` is the same score, gain and Poisson log-likelihood from mpmath's
digamma and loggamma at 50 digits, which tests/test_dispersion_cases.py holds the oracle against on three genes.  The sign
changes along the grid come from ``fast_score``, the plain form over a histogram of the counts: it is exact enough for a
sign and costs O(max y + N) per point instead of O(sum y + N)."""
from __future__ import annotations

import functools
import math

import numpy as np

D = 48
NS = (7, 257, 1037, 4099)
SIZE_VARIANTS = ("totals", "ones", "uniform", "holes")
CASES = [(N, v) for N in NS for v in SIZE_VARIANTS]
THETA_RANGE = (1e-4, 1e6)
NARROW_RANGE = (1.0, 10.0)
NARROW_CASES = [(257, "uniform"), (1037, "ones"), (1037, "holes"), (4099, "totals")]      # the cases run over NARROW_RANGE too
RTOL = 1e-11                     # gene_rank_cases.DEVIANCE_RTOL, the same argument: sums of <= 4099 terms plus the device's log
ORACLE_RTOL = 1e-13              # what the oracle itself holds against mpmath, x A
BISECT_TOL = 1e-13
GRID = 801
GP_THETAS = (0.05, 0.5, 2.0, 10.0, 100.0)
MEANS = (0.05, 1.0, 30.0)
N_REST = 20


def plan():
    """The plan query (host only): gene_chunk, workgroups, tol_t, partials_bytes."""
    from gpzoo_amd import ops
    return ops.gene_dispersion_plan(NS[-1], D, 1)


def granularity() -> int:
    return plan()["gene_chunk"]


def row_kinds(N: int) -> dict:
    g = granularity()
    kinds = {"empty": 0, "one": 1, "every": 2, "constant": 3}
    for j, n in enumerate((g - 1, g, g + 1)):
        if n <= N:
            kinds[f"g{n - g:+d}"] = 4 + j
    j = 7
    for th in GP_THETAS:
        for m in MEANS:
            kinds[f"gp-{th:g}-{m:g}"] = j
            j += 1
    for m in MEANS:
        kinds[f"poisson-{m:g}"] = j
        j += 1
    for name in ("big", "ge16", "spike"):
        kinds[name] = j
        j += 1
    assert j + N_REST == D
    return kinds


def holes(N: int):
    return np.array([2, N // 2, N - 4]) if N > 7 else np.array([3])


@functools.lru_cache(maxsize=None)
def counts(N: int, variant: str = "full") -> np.ndarray:
    """(D, N) float32 counts (exact in fp32), read-only."""
    rng = np.random.default_rng(2000 + N)
    g = granularity()
    kinds = row_kinds(N)
    effect = rng.uniform(0.5, 1.5, N)

    def gamma_poisson(theta, mean):
        return rng.poisson(rng.gamma(theta, mean * effect / theta))

    Y = np.zeros((D, N))
    Y[kinds["one"], N // 2 + 1] = 3
    Y[kinds["every"]] = rng.integers(1, 40, N)
    Y[kinds["constant"]] = 5
    for j, n in enumerate((g - 1, g, g + 1)):
        if n <= N:
            Y[4 + j, rng.choice(N, n, replace=False)] = rng.integers(1, 9, n)
        else:
            Y[4 + j] = gamma_poisson(1.0, 2.0 + j)
    for th in GP_THETAS:
        for m in MEANS:
            Y[kinds[f"gp-{th:g}-{m:g}"]] = gamma_poisson(th, m)
    for m in MEANS:
        Y[kinds[f"poisson-{m:g}"]] = rng.poisson(m * effect)
    where = rng.choice(N, min(N, 40), replace=False)
    Y[kinds["big"], where] = np.round(np.exp(rng.uniform(0.0, np.log(3000.0), where.size)))
    Y[kinds["big"], where[0]] = 2999
    Y[kinds["ge16"]] = rng.integers(16, 60, N)
    Y[kinds["ge16"], :2] = (16, 17)
    Y[kinds["spike"], N // 3] = 20000
    for d in range(D - N_REST, D):
        Y[d] = gamma_poisson(np.exp(rng.uniform(np.log(0.1), np.log(50.0))), np.exp(rng.uniform(np.log(0.2), np.log(20.0))))
    Y[D - 1] = np.maximum(Y[D - 1], 1.0)                     # every spot has counts before the holes are cut
    if variant == "holes":
        Y[:, holes(N)] = 0
    else:
        assert variant == "full"
    out = Y.astype(np.float32)
    assert (out == Y).all() and (Y >= 0).all() and Y.max() < 2 ** 24
    out.setflags(write=False)
    return out


def case_counts(N: int, sizes: str) -> np.ndarray:
    return counts(N, "holes" if sizes == "holes" else "full")


@functools.lru_cache(maxsize=None)
def case_sizes(N: int, sizes: str) -> np.ndarray:
    if sizes in ("totals", "holes"):
        out = case_counts(N, sizes).astype(np.float64).sum(axis=0)
    elif sizes == "ones":
        out = np.ones(N)
    else:
        assert sizes == "uniform"
        out = np.random.default_rng(70 + N).uniform(0.3, 3.0, N)
    out.setflags(write=False)
    return out


# ---- the terms ------------------------------------------------------------------------------------------------------------

def _atanh_tail(z):
    p = np.full_like(z, 1.0 / 25)
    for j in range(23, 2, -2):
        p = p * z + 1.0 / j
    return p


def h(x):
    """x / (1 + x) - log1p(x), x >= 0."""
    x = np.asarray(x, dtype=np.float64)
    small = x <= 0.5
    xs = np.where(small, x, 0.0)
    s = xs / (2.0 + xs)
    series = -(xs * xs) / ((1.0 + xs) * (2.0 + xs)) - 2.0 * s ** 3 * _atanh_tail(s * s)
    xl = np.where(small, 1.0, x)
    return np.where(small, series, xl / (1.0 + xl) - np.log1p(xl))


def xml(x):
    """x - log1p(x), x >= 0."""
    x = np.asarray(x, dtype=np.float64)
    small = x <= 0.5
    xs = np.where(small, x, 0.0)
    s = xs / (2.0 + xs)
    series = s * xs - 2.0 * s ** 3 * _atanh_tail(s * s)
    xl = np.where(small, 1.0, x)
    return np.where(small, series, xl - np.log1p(xl))


class Gene:
    """The null of one gene of a case and its stored entries flattened over k: entry j with count y_j owns the y_j
    consecutive elements K = 0 .. y_j - 1 of ``K`` / ``MUK`` from ``starts[j]``."""

    def __init__(self, y_row, size):
        y = np.asarray(y_row, dtype=np.float64)
        self.sum = y.sum()
        self.p = self.sum / size.sum() if self.sum > 0 else 0.0
        self.mu = self.p * size                                     # (N,)
        self.y_all = y
        nz = np.nonzero(y)[0]
        self.y = y[nz]
        self.mu_st = self.mu[nz]
        yi = self.y.astype(np.int64)
        self.starts = np.concatenate([[0], np.cumsum(yi)[:-1]]).astype(np.int64) if nz.size else np.zeros(0, dtype=np.int64)
        total = int(yi.sum())
        self.K = (np.arange(total) - np.repeat(self.starts, yi)).astype(np.float64)
        self.MUK = np.repeat(self.mu_st, yi)
        self.hist = np.bincount(yi)[::-1].cumsum()[::-1][1:].astype(np.float64) if nz.size else np.zeros(0)   # entries with y > k

    def _entry_sums(self, v):
        return np.add.reduceat(v, self.starts) if self.starts.size else np.zeros(0)

    def score(self, theta):
        """(S, A, H) at theta."""
        x = self.mu / theta
        a = theta * h(x)
        q = x / (1.0 + x)
        da = a + theta * (q * q)
        K, MU = self.K, self.MUK
        b = theta * self._entry_sums((MU - K) / ((theta + K) * (theta + MU)))
        db = b + theta * theta * self._entry_sums((K - MU) * (2.0 * theta + K + MU) / (((theta + K) * (theta + MU)) ** 2))
        return a.sum() + b.sum(), np.abs(a).sum() + np.abs(b).sum(), da.sum() + db.sum()

    def fast_score(self, thetas):
        """S at every theta of an array from sum_k c_k / (theta + k), c_k = the entries with y > k: the plain form, which
        loses theta / y digits -- for the sign of S on a grid only."""
        th = np.asarray(thetas, dtype=np.float64)[:, None]
        x = self.mu[None, :] / th
        a = (th * (x / (1.0 + x) - np.log1p(x))).sum(axis=1)
        k = np.arange(self.hist.size, dtype=np.float64)[None, :]
        out = np.empty(th.shape[0])
        for i in range(0, th.shape[0], 64):                          # (64, max y) at a time
            t = th[i:i + 64]
            out[i:i + 64] = (t * ((self.hist[None, :] / (t + k)).sum(axis=1, keepdims=True)
                                  - (self.y[None, :] / (t + self.mu_st[None, :])).sum(axis=1, keepdims=True)))[:, 0]
        return a + out

    def gain(self, theta):
        """(gain, sum of |terms|): a term is one spot's bracket or one stored entry's sum over k."""
        z = theta * xml(self.mu / theta)
        K, MU = self.K, self.MUK
        arg = (K - MU) / (theta + MU)
        near = np.abs(arg) <= 0.5
        logs = np.where(near, np.log1p(np.where(near, arg, 0.0)), np.log(np.where(near, 1.0, (theta + K) / (theta + MU))))
        e = self._entry_sums(logs)
        return z.sum() + e.sum(), np.abs(z).sum() + np.abs(e).sum()

    def poisson_loglik(self):
        """(value, scale)."""
        if self.y.size == 0:
            return 0.0, 0.0
        lg = np.array([math.lgamma(v + 1.0) for v in self.y])
        t = self.y * np.log(self.mu_st) - lg
        return t.sum() - self.sum, np.abs(t).sum() + self.sum

    def moment_start(self, theta_range):
        """(theta_0, den, scale of den): sum mu^2 / (sum (y - mu)^2 - sum y), theta_max where that is <= 0, clipped."""
        num = (self.mu ** 2).sum()
        sq = ((self.y_all - self.mu) ** 2).sum()
        den = sq - self.sum
        th = num / den if den > 0 else theta_range[1]
        return min(max(th, theta_range[0]), theta_range[1]), den, (self.y_all ** 2).sum() + 3.0 * num + self.sum


@functools.lru_cache(maxsize=None)
def genes(N: int, sizes: str):
    Y, size = case_counts(N, sizes), case_sizes(N, sizes)
    return tuple(Gene(Y[d], size) for d in range(D))


@functools.lru_cache(maxsize=None)
def solve(N: int, sizes: str, theta_range=THETA_RANGE) -> dict:
    """The oracle's fit of every gene of a case, arrays of D: theta, status, gain, gain_scale, poisson_loglik, pl_scale, and
    at the root (status 0) S, A, H; S_lo / A_lo and S_hi / A_hi at the ends of the range (NaN for a gene without counts)."""
    t_lo, t_hi = math.log(theta_range[0]), math.log(theta_range[1])
    out = {k: np.full(D, np.nan) for k in ("theta", "S", "A", "H", "S_lo", "A_lo", "S_hi", "A_hi")}
    out.update({k: np.zeros(D) for k in ("gain", "gain_scale", "poisson_loglik", "pl_scale")})
    out["status"] = np.zeros(D, dtype=np.int32)
    for d, g in enumerate(genes(N, sizes)):
        if g.sum == 0:
            out["status"][d] = 4
            continue
        out["poisson_loglik"][d], out["pl_scale"][d] = g.poisson_loglik()
        out["S_hi"][d], out["A_hi"][d], _ = g.score(theta_range[1])
        out["S_lo"][d], out["A_lo"][d], _ = g.score(theta_range[0])
        if out["S_hi"][d] >= 0:
            out["status"][d], out["theta"][d] = 1, np.inf
            continue
        if out["S_lo"][d] <= 0:
            out["status"][d], out["theta"][d] = 2, theta_range[0]
        else:
            lo, hi = t_lo, t_hi
            while hi - lo > BISECT_TOL:
                mid = 0.5 * (lo + hi)
                if g.score(math.exp(mid))[0] > 0:
                    lo = mid
                else:
                    hi = mid
            out["theta"][d] = math.exp(0.5 * (lo + hi))
            out["S"][d], out["A"][d], out["H"][d] = g.score(out["theta"][d])
        out["gain"][d], out["gain_scale"][d] = g.gain(out["theta"][d])
    for v in out.values():
        v.setflags(write=False)
    return out


def sign_changes(N: int, sizes: str, theta_range=THETA_RANGE) -> np.ndarray:
    """(D,) how often the score changes sign along GRID points in t over the range."""
    t = np.linspace(math.log(theta_range[0]), math.log(theta_range[1]), GRID)
    out = np.zeros(D, dtype=np.int64)
    for d, g in enumerate(genes(N, sizes)):
        if g.sum > 0:
            s = np.sign(g.fast_score(np.exp(t)))
            s = s[s != 0]
            out[d] = int((s[1:] != s[:-1]).sum())
    return out


def mp_terms(g: Gene, theta: float):
    """(S, gain, poisson_loglik) of a gene at theta from mpmath at 50 digits: digamma and loggamma differences."""
    import mpmath as mp
    with mp.workdps(50):
        th = mp.mpf(theta)
        S = mp.mpf(0)
        G = mp.mpf(0)
        for m in g.mu:
            x = mp.mpf(float(m)) / th
            S += th * (x / (1 + x) - mp.log1p(x))
            G += th * (x - mp.log1p(x))
        P = -mp.mpf(float(g.sum))
        for y, m in zip(g.y, g.mu_st):
            y, m = mp.mpf(float(y)), mp.mpf(float(m))
            S += th * (mp.digamma(y + th) - mp.digamma(th) - y / (th + m))
            G += mp.loggamma(y + th) - mp.loggamma(th) - y * mp.log(th + m)
            P += y * mp.log(m) - mp.loggamma(y + 1)
        return S, G, P
