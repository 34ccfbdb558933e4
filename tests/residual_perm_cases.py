"""Cases and fp64 oracles for tests/test_hip_residual_perm.py: Geary's C, the kurtosis and the permutation null of the
residuals of a fitted count model (csrc/residual.hip, the column passes of csrc/spatial_stats.hip).  TEST INFRASTRUCTURE
ONLY; numpy, importable without a GPU -- tests/test_residual_perm_cases.py checks everything here on the CPU.

The residual cases, their oracle and their fp32 emulation are those of tests/residual_cases.py, used as they are.  Added here:

  geary_c / kurtosis      of the rows of a (G, B) residual array: geary_cases' direct centred sums
  perm_stats              I and C of the PERMUTED array r^pi[n] = r[pi[n]] scored over the FIXED table -- the definition
  relabelled_stats        I and C of the unpermuted array over T_pi[pi[i], m] = pi[nbr[i, m]] -- what the device computes;
                          the CPU test holds the two together
  counts_bracket          moran_perm_cases.counts_bracket's construction around given observed and simulated values

TOLERANCES.  Against the entry's OWN residuals (``ops.count_residuals`` pushed through these oracles) every statistic is a
centred fp64 sum of fp32 values: MORAN_ATOL = 1e-10 (geary_cases.GEARY_ATOL_ROWS is the same number), relative above 1 as
in test_hip_residual_autocorr._close; the kurtosis within geary_cases.KURTOSIS_RTOL.  BAND = 2 x 1e-10 for the counts.
End to end from the model inputs, I holds within residual_cases.I_ATOL.  For C, measured the way I_ATOL was: the emulated
fp32 residuals pushed through the fp64 Geary oracle against the oracle's own, over ``case_table`` of every case of TABLE,
both kinds and both families (``measure()``, python tests/residual_perm_cases.py):
    worst |C(emulated) - C(oracle)| = 3.84e-07  (case lt56, deviance, Poisson)
x 3, rounded up to one significant digit: C_ATOL = 2e-6.  It is larger than I_ATOL (9e-7; worst 2.85e-07 on the same
case) because C's numerator is a sum of SQUARED differences of residuals: at a probe (a count of thousands beside a rate
of tens, |r| ~ 1e3) an error e of the residual enters as 2 |r| e, while I's cross products carry it once.
"""
from __future__ import annotations

import functools

import numpy as np

import geary_cases as Y
import moran_perm_cases as M
import residual_cases as R

MORAN_ATOL = Y.GEARY_ATOL_ROWS       # 1e-10
BAND = 2.0 * MORAN_ATOL
C_ATOL = 2e-6
P = 19                               # 16 + 3: the last batch of the plan's choice is partial; so is 3's and 32 covers all

PLANTED_P = 199
PLANTED_PERM_SEED = 4242


# ---- statistics of a residual array ---------------------------------------------------------------------------------------

def geary_c(res, nbr):
    """(G,) Geary's C of every row of res (G, B) over nbr (B, K): geary_cases.geary_oracle."""
    return Y.geary_oracle(np.asarray(res, dtype=np.float64), np.asarray(nbr))


def kurtosis(res):
    """(G,) m4 / m2^2 of every row of res: geary_cases.kurtosis_oracle (extended precision)."""
    return Y.kurtosis_oracle(np.asarray(res, dtype=np.float64))["kurtosis"]


def stats(res, nbr):
    """dict(I, C, mean, var, kurtosis) of the rows of res."""
    I, mean, var = R.morans_i(res, nbr)
    return dict(I=I, C=geary_c(res, nbr), mean=mean, var=var, kurtosis=kurtosis(res))


def perm_stats(res, nbr, perms):
    """(I, C), (G, P) each: the statistics of res[:, pi] over the fixed table, per row pi of perms."""
    res = np.asarray(res, dtype=np.float64)
    I = np.stack([R.morans_i(res[:, pi], nbr)[0] for pi in perms], axis=1)
    C = np.stack([geary_c(res[:, pi], nbr) for pi in perms], axis=1)
    return I, C


def relabelled_stats(res, nbr, pi):
    """(I, C), (G,) each: res unpermuted over the relabelled table T_pi (moran_perm_cases.relabelled)."""
    T = M.relabelled(np.asarray(nbr), pi)
    return R.morans_i(res, T)[0], geary_c(res, T)


def perms_of(B, P_=P, identity_first=True, seed=0):
    """(P, B) int32: the identity first (where asked for), then permutations from default_rng(31 + B + seed)."""
    rng = np.random.default_rng(31 + B + seed)
    rows = [np.arange(B)] if identity_first else []
    while len(rows) < P_:
        rows.append(rng.permutation(B))
    return np.stack(rows).astype(np.int32)


def counts_bracket(observed, sims, band=BAND):
    """(ge, le, band), int64 (G,) each: the permutations definitely above, definitely below, and inside the band, which may
    count either way.  A correct n_ge lies in [ge, ge + band], n_le in [le, le + band]."""
    diff = np.asarray(sims) - np.asarray(observed)[:, None]
    return ((diff > band).sum(axis=1).astype(np.int64), (diff < -band).sum(axis=1).astype(np.int64),
            (np.abs(diff) <= band).sum(axis=1).astype(np.int64))


# ---- C end to end -----------------------------------------------------------------------------------------------------------

def c_error(c, nbr):
    """(worst |C(emulated residuals) - C(oracle residuals)| over kinds and families, where)."""
    worst = (0.0, "")
    for kind in R.KINDS:
        for family in R.FAMILIES:
            ref = geary_c(R.oracle_residuals(c, kind, family), nbr)
            got = geary_c(R.emulate_residuals(c, kind, family), nbr)
            worst = max(worst, (float(np.abs(got - ref).max()), f"{c['name']} {kind} {family}"))
    return worst


@functools.lru_cache(maxsize=None)
def c_error_worst():
    """c_error over ``case_table`` of every case of TABLE (the cases ``make_case`` settles on)."""
    return max(c_error(R.make_case(name), R.case_table(R.make_case(name))) for name, *_ in R.TABLE)


def measure():
    worst = (0.0, "")
    for name, *_ in R.TABLE:
        c = R._draw(name, *next(r for r in R.TABLE if r[0] == name)[1:4], 0)
        worst = max(worst, c_error(c, R.case_table(c)))
    print(f"worst C: {worst[0]:.3e} ({worst[1]}); x 3 = {3 * worst[0]:.3e}")


# ---- the enumeration: 7 spots, all 5040 relabellings -----------------------------------------------------------------------

ENUM_D = 5


@functools.lru_cache(maxsize=None)
def enum_case():
    """The 7-spot case ``one_gene`` drawn at D = 5: five genes, B = 7, one factor."""
    return R._draw("enum", ENUM_D, Y.ENUM_N, 1, 0)


def enum_moments(res, nbr):
    """Per row of res (G, 7): dict(EI, EC, VI, VC) -- the mean and the population variance of I and C over all 5040
    relabellings, by enumeration in fp64 (geary_cases.enum_statistics)."""
    out = dict(EI=[], EC=[], VI=[], VC=[])
    for x in np.asarray(res, dtype=np.float64):
        I, C = Y.enum_statistics(x, nbr)
        out["EI"].append(I.mean()), out["EC"].append(C.mean()), out["VI"].append(I.var()), out["VC"].append(C.var())
    return {k: np.array(v) for k, v in out.items()}


# ---- planted structure --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planted_perms():
    """(199, 400) int32: rows np.random.default_rng(4242).permutation(400), drawn in order."""
    rng = np.random.default_rng(PLANTED_PERM_SEED)
    out = np.stack([rng.permutation(400) for _ in range(PLANTED_P)]).astype(np.int32)
    out.setflags(write=False)
    return out


def fdr_bh(p):
    """Benjamini-Hochberg adjusted p-values (no NaN here): q_(i) = min_{j >= i} min(1, m p_(j) / j)."""
    p = np.asarray(p, dtype=np.float64)
    order = np.argsort(-p, kind="stable")
    m = p.size
    q = np.minimum.accumulate(np.minimum(1.0, p[order] * m / np.arange(m, 0, -1)))
    out = np.empty(m)
    out[order] = q
    return out


@functools.lru_cache(maxsize=None)
def planted_oracle(kind, family, mode):
    """dict(n_ge, n_le, p, selected) of the planted case on the fp64 oracle: p is the p-value for positive autocorrelation,
    (n_ge + 1) / 200 for Moran and (n_le + 1) / 200 for Geary; selected the genes with fdr_bh(p) <= 0.05."""
    c = R.planted_case()
    res = R.oracle_residuals(c, kind, family)
    I, C = perm_stats(res, c["nbr"], planted_perms())
    obs, sims = (R.morans_i(res, c["nbr"])[0], I) if mode == "moran" else (geary_c(res, c["nbr"]), C)
    n_ge, n_le = (sims >= obs[:, None]).sum(axis=1), (sims <= obs[:, None]).sum(axis=1)
    p = ((n_ge if mode == "moran" else n_le) + 1.0) / (PLANTED_P + 1.0)
    # the margin of every comparison: no simulated value within the end-to-end tolerance of the observed one may decide a count
    margin = float(np.abs(sims - obs[:, None]).min())
    return dict(n_ge=n_ge, n_le=n_le, p=p, selected=np.flatnonzero(fdr_bh(p) <= 0.05), margin=margin)


if __name__ == "__main__":
    measure()
