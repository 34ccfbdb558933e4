"""Case builders of the sparse-count KL NMF tests (tests/test_sparse_nmf_cases.py on the CPU, tests/test_hip_nmf_sparse.py on
the GPU).  Imports numpy, the numpy oracle and -- for the plan query only -- the library's host entry; no GPU needed.

A case is a dense X (N, D) of integer counts with starts (W0, H0): the planted counts of ``nmf_oracle.planted_counts`` with
every entry kept with probability ``density``, then the forced rows and columns written over that.  The counts are small
integers, exact in float32, so the SparseCounts of ``X.T`` holds exactly X and the oracle on the dense X is the yardstick.
Every chunk length and instance boundary used to size a case comes from ``plan()`` (gpz_nmf_kl_sparse_plan)."""
from __future__ import annotations

import functools

import numpy as np

import nmf_oracle as O


@functools.lru_cache(maxsize=None)
def plan(N=1, D=1, L=1, nnz=0, dtype=None):
    """gpz_nmf_kl_sparse_plan: host only.  The library is built first if it is not there (as tests/test_abi.py does)."""
    import torch
    from gpzoo_amd import build, ops
    build.build(force=False, verbose=False)
    return ops.nmf_kl_sparse_plan(N, D, L, nnz, torch.float32 if dtype is None else dtype)


def instance_boundaries():
    """Every L in 1..64 that is the last of its kernel instance, ascending (the padded sizes themselves)."""
    return sorted({plan(L=L)["factors_padded"] for L in range(1, 65)})


def boundary_factors():
    """One L at and one L just above every kernel-instance boundary, within 1..64."""
    b = instance_boundaries()
    return sorted({L for x in b for L in (x, x + 1) if L <= 64})


def build(N, D, L, density=0.2, seed=0, empty=True, full_gene=False, full_spot=False, gene_lengths=(), spot_lengths=(),
          zero_last=True, all_zero=False):
    """dict(X, W0, H0, claims).  In the order they are applied (a later one overrides an earlier one where they meet):
    full_gene   gene 1 is non-zero at every spot
    full_spot   spot 1 holds every gene
    gene_lengths  gene 2 + i has exactly gene_lengths[i] non-zeros, at the first spots that are not the empty spot
    spot_lengths  spot 4 + i has exactly spot_lengths[i] non-zeros, at the last genes that are neither forced nor empty
    empty       spot 3 and gene 0 are all zero (needs N > 3)
    zero_last   the last component of W0 and of H0 is zero (L > 2): the zero-rowsum and zero-colsum rules are taken
    all_zero    X = 0
    ``claims`` records which rows carry which property, for the structure check."""
    rng = np.random.default_rng(7000 + 31 * N + 17 * D + L + seed)
    X = O.planted_counts(N, D, L, 1000 + N + D + L + seed)
    X = X * (rng.random(X.shape) < density)
    claims = {}
    empty = empty and N > 3 and D > 1
    e_spot, e_gene = (3, 0) if empty else (-1, -1)
    if full_gene:
        X[:, 1] = np.maximum(X[:, 1], 1.0)
        claims["full_gene"] = 1
    if full_spot:
        X[1, :] = np.maximum(X[1, :], 1.0)
        claims["full_spot"] = 1
    spots = np.array([n for n in range(N) if n != e_spot])
    for i, m in enumerate(gene_lengths):
        g = 2 + i
        assert g < D and m <= len(spots) and not full_spot
        X[:, g] = 0.0
        X[spots[:m], g] = 1.0 + (np.arange(m) % 3)
        claims.setdefault("gene_lengths", []).append((g, int(m)))
    free = np.array([d for d in range(D) if d != e_gene and not (2 <= d < 2 + len(gene_lengths)) and not (full_gene and d == 1)])
    for i, m in enumerate(spot_lengths):
        s = 4 + i
        assert s < N and m <= len(free)
        X[s, :] = np.where(np.isin(np.arange(D), free), 0.0, X[s, :])
        X[s, free[len(free) - m:]] = 1.0 + (np.arange(m) % 2)
        claims.setdefault("spot_lengths", []).append((s, int(m), free))
    if empty:
        X[e_spot] = 0.0
        X[:, e_gene] = 0.0
        claims["empty"] = (e_spot, e_gene)
    if all_zero:
        X[:] = 0.0
        claims["all_zero"] = True
    W0 = np.abs(rng.standard_normal((N, L))) + 0.05
    H0 = np.abs(rng.standard_normal((L, D))) + 0.05
    if zero_last and L > 2:
        W0[:, L - 1] = 0.0
        H0[L - 1] = 0.0
        claims["zero_last"] = L - 1
    return dict(X=X, W0=W0, H0=H0, claims=claims)


def check_structure(case):
    """Asserts that the case has what its claims say; returns the number of properties checked."""
    X, c = case["X"], case["claims"]
    N, D = X.shape
    assert (X >= 0).all() and (X == np.round(X)).all() and X.max() < 2 ** 24          # integer counts, exact in float32
    n = 0
    if "all_zero" in c:
        assert not X.any()
        return 1
    e_spot, e_gene = c.get("empty", (-1, -1))
    if "empty" in c:
        assert not X[e_spot].any() and not X[:, e_gene].any()
        n += 1
    if "full_gene" in c:
        rows = [r for r in range(N) if r != e_spot]
        assert (X[rows, c["full_gene"]] > 0).all()
        n += 1
    if "full_spot" in c:
        cols = [d for d in range(D) if d != e_gene]
        assert (X[c["full_spot"], cols] > 0).all()
        n += 1
    for g, m in c.get("gene_lengths", []):
        assert int((X[:, g] > 0).sum()) == m, (g, m)
        n += 1
    for s, m, free in c.get("spot_lengths", []):
        assert int((X[s, free] > 0).sum()) == m, (s, m)
        n += 1
    if "zero_last" in c:
        assert not case["W0"][:, c["zero_last"]].any() and not case["H0"][c["zero_last"]].any()
        assert (np.delete(case["W0"], c["zero_last"], 1) > 0).all() and (np.delete(case["H0"], c["zero_last"], 0) > 0).all()
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def named(name):
    """The named cases both test files use.  Sizes come from the plan query."""
    p = plan()
    c, sc, rows = p["gene_chunk"], p["spot_chunk"], p["colsum_rows"]
    if name == "one":
        case = build(1, 1, 1, density=0.3, empty=False)
        case["X"][0, 0] = max(case["X"][0, 0], 2.0)          # the one entry is a forced one
        return case
    if name == "small":
        return build(63, 17, 3, density=0.3, full_gene=True)
    if name == "chunked":                       # gene rows of exactly c, c + 1 and 2 c + 1 non-zeros
        return build(2 * c + 2, 40, 5, density=0.15, gene_lengths=(c, c + 1, 2 * c + 1), full_gene=True)
    if name == "spot_chunked":                  # the same for spot rows, if the W pass cuts them
        assert sc > 0
        return build(70, 2 * sc + 8, 5, density=0.15, spot_lengths=(sc, sc + 1, 2 * sc + 1))
    if name == "lanes_wrap":                    # 64 k + 1 genes and a spot holding every one: the lanes wrap, with a tail
        return build(70, 64 * 3 + 1, 2, density=0.2, full_spot=True, empty=False)
    if name == "colsum_block":                  # the column sums of W cross into a second partial block
        return build(rows + 1, 33, 4, density=0.25)
    if name == "all_zero":
        return build(40, 12, 3, all_zero=True, empty=False)
    if name.startswith("L"):
        return build(130, 70, int(name[1:]), density=0.2)
    raise KeyError(name)


def names():
    out = ["one", "small"] + [f"L{L}" for L in boundary_factors()] + ["chunked", "lanes_wrap", "colsum_block", "all_zero"]
    if plan()["spot_chunk"] > 0:
        out.insert(out.index("chunked") + 1, "spot_chunked")
    return out


@functools.lru_cache(maxsize=None)
def oracle_iterates(name, stops=(1, 10, 200)):
    """{iterations: (W, H)} of the numpy oracle on the dense X of a named case, computed once."""
    case = named(name)
    W, H = case["W0"].copy(), case["H0"].copy()
    out, done = {}, 0
    for it in stops:
        for _ in range(it - done):
            W = O.update_w(case["X"], W, H)
            H = O.update_h(case["X"], W, H)
        done = it
        out[it] = (W.copy(), H.copy())
    return out


def counts_of(X):
    """The SparseCounts (D genes, N spots) of a dense X (N, D), on the CPU."""
    import torch
    from gpzoo_amd.likelihoods import SparseCounts
    return SparseCounts(torch.as_tensor(np.ascontiguousarray(X.T)))
