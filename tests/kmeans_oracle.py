"""numpy fp64 oracle of kmeans_inducing_points (gpz_kmeans_seed / _lloyd / _assign), by brute force (TEST INFRASTRUCTURE
ONLY; importable without a GPU).

The arithmetic is the contract the kernels share: d^2 from direct differences in fp64, each square rounded, added in
coordinate order, NaN -> +inf; the label is the arg-min over (d^2, centre index); centres stay fp64 and X is not centred;
one Lloyd iteration is sklearn's ``lloyd_iter`` + the stopping rules of ``_kmeans_single_lloyd`` with
``_relocate_empty_clusters_dense`` given a defined pairing; seeding is sklearn's ``_kmeans_plusplus`` with the random
stream ``u`` passed in.  Sums here run in ascending index; the kernels' orders differ (fixed trees), which moves a sum by
a few ulp: comparisons of sums are to 1e-12, comparisons of choices (labels, indices, iteration counts) are exact on
inputs whose choices are not within rounding of a tie (``min_gap`` / the margins returned below say how far they are)."""
from __future__ import annotations

import math

import numpy as np


def d2_matrix(X, C):
    """(n, m) fp64 squared distances, direct differences, squares rounded separately, coordinate order; NaN -> +inf."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    s = (X[:, None, 0] - C[None, :, 0]) ** 2
    for k in range(1, X.shape[1]):
        s = s + (X[:, None, k] - C[None, :, k]) ** 2
    s[np.isnan(s)] = np.inf
    return s


def assign(X, C, gap=False, rows=2048):
    """labels (N,) int64 = arg-min over (d^2, index) and the (N,) minimal d^2; with ``gap`` also the smallest relative
    difference between a point's best and second-best d^2 (inf for one centre)."""
    X = np.asarray(X, dtype=np.float64)
    N = len(X)
    labels, best, g = np.empty(N, np.int64), np.empty(N), np.inf
    for r in range(0, N, rows):
        D = d2_matrix(X[r:r + rows], C)
        lab = D.argmin(axis=1)                      # the first minimum: ties to the lower index
        labels[r:r + rows] = lab
        best[r:r + rows] = D[np.arange(len(lab)), lab]
        if gap and D.shape[1] > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            b, s = two[:, 0], two[:, 1]
            ok = np.isfinite(s) & (s > 0)
            rel = np.where(ok, (s - b) / np.where(ok, s, 1.0), np.where(s > b, 1.0, 0.0))   # 0 = an exact tie
            g = min(g, float(rel.min()))
    return (labels, best, g) if gap else (labels, best)


def inertia_of(X, C, labels):
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    diff = X - C[labels]
    s = diff[:, 0] ** 2
    for k in range(1, X.shape[1]):
        s = s + diff[:, k] ** 2
    return float(s.sum())


def far_points(d2, n):
    """The n points with the largest d^2, descending, ties to the lower index."""
    order = np.lexsort((np.arange(len(d2)), -d2))
    return order[:n]


def lloyd_iter(X, C):
    """One iteration from the centres C: (C_new, labels, shift, relocated pairs [(point, from, to), ...])."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    M = len(C)
    labels, best = assign(X, C)
    sums = np.zeros_like(C)
    np.add.at(sums, labels, X)                      # in ascending point index
    counts = np.bincount(labels, minlength=M).astype(np.int64)
    moved = []
    empty = np.flatnonzero(counts == 0)
    if len(empty) and best.max() > 0:
        for n, to in zip(far_points(best, len(empty)), empty):
            frm = labels[n]
            sums[frm] -= X[n]
            sums[to] = X[n]
            counts[frm] -= 1
            counts[to] = 1
            moved.append((int(n), int(frm), int(to)))
    C_new = C.copy()
    has = counts > 0
    C_new[has] = sums[has] * (1.0 / counts[has])[:, None]
    shift = float(((C_new - C) ** 2).sum())
    return C_new, labels, shift, moved


def tolerance(X, tol):
    return float(tol) * float(np.mean(np.var(np.asarray(X, dtype=np.float64), axis=0)))


def lloyd(X, C0, max_iter=300, tol=1e-4, gap=False):
    """dict(centres, labels, inertia, n_iter, converged, shifts, relocated, relabelled[, min_gap]) of Lloyd from C0."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(C0, dtype=np.float64)
    tol_abs = tolerance(X, tol)
    prev = np.full(len(X), -1, np.int64)
    converged, shifts, relocated, g = False, [], 0, np.inf
    for it in range(max_iter):
        if gap:
            g = min(g, assign(X, C, gap=True)[2])
        C, labels, shift, moved = lloyd_iter(X, C)
        shifts.append(shift)
        relocated += len(moved)
        if np.array_equal(labels, prev):
            converged = "labels"
            break
        if shift <= tol_abs:
            converged = "tol"
            break
        prev = labels
    relabelled = converged != "labels"
    if relabelled:
        if gap:
            g = min(g, assign(X, C, gap=True)[2])
        labels, _ = assign(X, C)
    out = dict(centres=C, labels=labels, inertia=inertia_of(X, C, labels), n_iter=it + 1, converged=converged, shifts=shifts,
               relocated=relocated, relabelled=relabelled)
    if gap:
        out["min_gap"] = g
    return out


def n_trials(M):
    return 2 + int(math.log(M))


def seed(X, M, u):
    """k-means++ from the draws u (M, T): (indices (M,) int64, draw_margin, win_margin).  draw_margin: the smallest
    distance of a draw u pot from the cumulative-sum entries on either side of it, over pot; win_margin: the smallest
    relative lead of a winning potential over the runner-up among candidates at other positions."""
    X = np.asarray(X, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    N, T = len(X), u.shape[1]
    idx = np.empty(M, np.int64)
    idx[0] = min(N - 1, int(math.floor(u[0, 0] * N)))
    closest = d2_matrix(X, X[idx[:1]])[:, 0]
    draw_margin, win_margin = np.inf, np.inf
    for c in range(1, M):
        cum = np.cumsum(closest)
        pot = cum[-1]
        target = u[c] * pot
        cand = np.minimum(np.searchsorted(cum, target, side="left"), N - 1)
        if pot > 0:
            lo = np.where(cand > 0, cum[np.maximum(cand - 1, 0)], -np.inf)
            draw_margin = min(draw_margin, float(np.min(np.minimum(cum[cand] - target, target - lo)) / pot))
        D = np.minimum(closest[None, :], d2_matrix(X[cand], X))
        pots = D.sum(axis=1)
        best = int(np.argmin(pots))                 # the first minimum: ties to the lower t
        others = pots[(X[cand] != X[cand[best]]).any(axis=1)]      # (a copy of the same point has the same potential, bit for bit)
        if len(others) and pots[best] > 0:
            win_margin = min(win_margin, float((others.min() - pots[best]) / pots[best]))
        idx[c] = cand[best]
        closest = D[best]
    return idx, draw_margin, win_margin


def kmeans(X, M, random_state=None, max_iter=300, tol=1e-4):
    """The whole of kmeans_inducing_points(init="k-means++"): seeding from default_rng(random_state), then Lloyd."""
    u = np.random.default_rng(random_state).random((M, n_trials(M)))
    idx, _, _ = seed(X, M, u)
    out = lloyd(X, np.asarray(X, dtype=np.float64)[idx], max_iter, tol)
    out["seed_indices"] = idx
    return out
