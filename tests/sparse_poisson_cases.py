"""Case builders and the fp64 oracle of the SPARSE formulas for tests/test_hip_poisson_sparse.py (TEST INFRASTRUCTURE ONLY;
plain torch, importable without a GPU -- tests/test_sparse_poisson_cases.py checks everything here on the CPU).

The operation is gpz_poisson_nsf_sparse (csrc/poisson_sparse.hip): the Poisson step of tests/poisson_cases.py evaluated
from the non-zeros of y.  A *case* is a dict as ``poisson_cases.make_case`` builds it, with y thinned to a few per cent
density; ``c["y"]`` is the (D, N) count matrix of the whole data set and, for a batch case, ``c["idx"]`` lists the spots
the parameters (mean, scale, eps, V: B columns) belong to.  ``batch_dense(c)`` is the (D, B) array the dense formula sees.

Boundaries (the gene pass's chunk length, the spot pass's sample group) come from the library's own host-only plan query,
``ops.poisson_nsf_sparse_plan``; nothing here restates them.  Probe counts as in poisson_cases: large counts at the first
and last entry of every chunk and at the first and last gene and spot, each worth at least ten tolerances in every output
it feeds, so that one dropped or doubled non-zero fails the project's usual Poisson tolerances."""
from __future__ import annotations

import torch

import poisson_cases as PC

OUTPUTS = PC.OUTPUTS


def plan(N, B, D, Lt, E, nnz=0):
    from gpzoo_amd import ops
    return ops.poisson_nsf_sparse_plan(N, B, D, Lt, E, nnz)


def chunk_length() -> int:
    return plan(1037, 1037, 80, 20, 3)["gene_chunk"]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def make_sparse_case(N, D, Lt, E, seed, density=0.05, B=None, idx=None, rows=None, cols=None, empty_rows=(), empty_cols=(),
                     values=None, probes=()):
    """``poisson_cases.make_case`` parameters for B (default N) columns and a (D, N) y thinned to ``density``.
    rows: {gene: sorted list of the spots where it is non-zero (exactly those)}; cols: {spot: list of genes} likewise;
    empty_rows / empty_cols are zeroed last; values: {(gene, spot): value}; probes: (gene, spot, count) written last."""
    B = N if idx is None and B is None else (len(idx) if idx is not None else B)
    p = PC.make_case(B, D, Lt, E, seed=seed)
    g = torch.Generator().manual_seed(90000 + 7919 * seed + 13 * N + D)
    y = torch.poisson(1.0 + 3.0 * torch.rand(D, N, generator=g, dtype=torch.float64), generator=g) + 1.0
    y = y * (torch.rand(D, N, generator=g) < density)
    for d, spots in (rows or {}).items():
        y[d, :] = 0.0
        y[d, list(spots)] = 1.0 + (torch.arange(len(spots), dtype=torch.float64) % 5)
    for n, genes in (cols or {}).items():
        y[:, n] = 0.0
        y[list(genes), n] = 1.0 + (torch.arange(len(genes), dtype=torch.float64) % 4)
    for d in empty_rows:
        y[d, :] = 0.0
    for n in empty_cols:
        y[:, n] = 0.0
    for (d, n), v in (values or {}).items():
        y[d, n] = v
    for d, n, cnt in probes:
        y[d, n] = float(cnt)
    c = dict(p, N=N, B=B, y=PC._f32_exact(y), probes=list(probes), seed=seed)
    if idx is not None:
        c["idx"] = torch.as_tensor(idx, dtype=torch.int64)
    return c


def batch_dense(c) -> torch.Tensor:
    return c["y"][:, c["idx"]] if "idx" in c else c["y"]


def dense_view(c) -> dict:
    """The case as poisson_cases.reference / sharpness read it: N = B columns, y = the batch's dense counts, probes in
    batch columns."""
    if "idx" not in c:
        return c
    pos = {int(n): j for j, n in enumerate(c["idx"].tolist())}
    return dict(c, N=c["B"], y=batch_dense(c), probes=[(d, pos[n], cnt) for d, n, cnt in c["probes"] if n in pos])


def sharpen(build, positions, need=PC.SHARP_AIM):
    """build(probes) -> case.  Counts start at 1000 + (37 i mod 1000) and grow (at most 20 000) until every probe is worth
    ``need`` tolerances in every output, judged by the fp64 reference alone (poisson_cases.make_probe_case's loop)."""
    probes = PC.probe_counts(positions)
    for _ in range(8):
        c = build(probes)
        nxt = []
        for (d, n, cnt), s in zip(probes, PC.sharpness(dense_view(c))):
            worst = min(s.values())
            if worst < need and cnt < PC.COUNT_MAX:
                cnt = min(PC.COUNT_MAX, int(cnt * min(max(1.5 * need / max(worst, 1e-30), 1.5), 20.0)) + 1)
            nxt.append((d, n, cnt))
        if nxt == probes:
            break
        probes = nxt
    return c


def _spread(N, m, seed):
    """m distinct spots of N, ascending (a fixed pseudo-random subset)."""
    g = torch.Generator().manual_seed(4100 + seed)
    return sorted(torch.randperm(N, generator=g)[:m].tolist())


_cache: dict = {}


def _cached(name, fn):
    if name not in _cache:
        _cache[name] = fn()
    return _cache[name]


# 1. factor counts and samples: every kernel-instance boundary the issue names, and a sample count beyond the group size
FACTOR_SHAPES = [(130, 80, Lt, 3) for Lt in (1, 4, 5, 20, 63, 64)]
SAMPLE_SHAPES = [(130, 80, 7, E) for E in (1, 2, 20, 33)]


def shape_case(shape):
    N, D, Lt, E = shape
    return _cached(("shape",) + tuple(shape), lambda: sharpen(
        lambda pr: make_sparse_case(N, D, Lt, E, seed=100 + Lt + 64 * E, density=0.08, probes=pr),
        [(0, 0), (D - 1, N - 1), (0, N - 1), (D - 1, 0)]))


# 2. chunk boundaries
CHUNK_GENES = {"C-1": 3, "C": 17, "C+1": 40, "2C+1": 62, "full": 79}     # the genes that carry the named row lengths
CHUNK_SHAPE = (1037, 80, 20, 3)


def chunk_rows():
    C, N = chunk_length(), CHUNK_SHAPE[0]
    assert 2 * C + 1 <= N, "the chunk case needs a row of 2C + 1 non-zeros"
    lens = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1, "full": N}
    return {CHUNK_GENES[k]: _spread(N, m, i) for i, (k, m) in enumerate(lens.items())}


def chunk_probe_positions():
    """First and last entry of every chunk of the five long rows; first and last gene and spot."""
    C, (N, D, _, _) = chunk_length(), CHUNK_SHAPE
    out = [(0, 0), (D - 1, N - 1)]
    for d, spots in chunk_rows().items():
        for lo in range(0, len(spots), C):
            hi = min(lo + C, len(spots)) - 1
            out += [(d, spots[lo]), (d, spots[hi])]
    return sorted(set(out))


def chunk_case():
    N, D, Lt, E = CHUNK_SHAPE
    return _cached("chunk", lambda: sharpen(
        lambda pr: make_sparse_case(N, D, Lt, E, seed=201, density=0.04, rows=chunk_rows(), probes=pr), chunk_probe_positions()))


DENSE_COLUMN_SHAPE, DENSE_COLUMN = (66, 2100, 5, 2), 31


def dense_column_case():
    N, D, Lt, E = DENSE_COLUMN_SHAPE
    return _cached("column", lambda: sharpen(
        lambda pr: make_sparse_case(N, D, Lt, E, seed=202, density=0.02, cols={DENSE_COLUMN: range(D)}, probes=pr),
        [(0, DENSE_COLUMN), (D - 1, DENSE_COLUMN), (0, 0), (D - 1, N - 1), (1049, DENSE_COLUMN)]))


# 3. degenerate structure
def empties_case():
    """Empty gene rows and spot columns, the first and the last of each among them."""
    N, D = 130, 80
    return _cached("empties", lambda: sharpen(
        lambda pr: make_sparse_case(N, D, 20, 3, seed=301, density=0.06, empty_rows=(0, 41, D - 1), empty_cols=(0, 66, 67, N - 1),
                                    probes=pr), [(1, 1), (D - 2, N - 2)]))


def no_counts_case():
    return _cached("nnz0", lambda: make_sparse_case(70, 37, 5, 3, seed=302, density=0.0))


def one_count_case():
    return _cached("nnz1", lambda: make_sparse_case(70, 37, 5, 3, seed=303, density=0.0, values={(21, 44): 7.0}))


def single_case():
    return _cached("1x1", lambda: make_sparse_case(1, 1, 3, 2, seed=304, density=0.0, values={(0, 0): 4.0}))


def values_case():
    """Counts of 256 and more and non-integer values (poisson_cases.COUNT_VALUES, its zero included: a stored zero)."""
    vals = {((7 * i + 3) % 80, (31 * i + 5) % 130): v for i, v in enumerate(PC.COUNT_VALUES * 6)}
    return _cached("values", lambda: make_sparse_case(130, 80, 20, 3, seed=305, density=0.05, values=vals))


# 4. batches of an N = 1037 data set
BATCH_N, BATCH_D = 1037, 80
BATCH_EMPTY_COLS = (0, 500, 501, 1036)
BATCH_HIDDEN_GENE = 11           # non-zero only in spots that the "hidden" batch leaves out


def _perm(seed):
    return torch.randperm(BATCH_N, generator=torch.Generator().manual_seed(seed)).tolist()


def batch_indices():
    p = _perm(77)
    hidden_spots = set(_spread(BATCH_N, 40, 9))
    return {"B1": [p[5]], "B70": p[:70], "perm": p,
            "empty_cols": list(BATCH_EMPTY_COLS) + [n for n in p[:60] if n not in BATCH_EMPTY_COLS],
            "hidden_gene": [n for n in p if n not in hidden_spots][:70]}


def batch_case(name):
    idx = batch_indices()[name]
    rows = {BATCH_HIDDEN_GENE: _spread(BATCH_N, 40, 9)}

    def build(pr):
        return make_sparse_case(BATCH_N, BATCH_D, 20, 3, seed=400, density=0.05, idx=idx, rows=rows,
                                empty_cols=BATCH_EMPTY_COLS, probes=pr)
    first, last = idx[0], idx[-1]
    if name == "empty_cols":
        first, last = idx[len(BATCH_EMPTY_COLS)], idx[-1]
    return _cached(("batch", name), lambda: sharpen(build, sorted({(0, first), (BATCH_D - 1, last)})))


BATCH_NAMES = ("B1", "B70", "perm", "empty_cols", "hidden_gene")


def all_cases():
    """(name, case) of every case of the GPU suite."""
    out = [("Lt%d-E%d" % s[2:], shape_case(s)) for s in FACTOR_SHAPES + SAMPLE_SHAPES]
    out += [("chunks", chunk_case()), ("dense_column", dense_column_case()), ("empties", empties_case()),
            ("nnz0", no_counts_case()), ("nnz1", one_count_case()), ("1x1", single_case()), ("values", values_case())]
    out += [("batch_" + b, batch_case(b)) for b in BATCH_NAMES]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# reference: the sparse formulas in fp64
# ---------------------------------------------------------------------------------------------------------------------

def sparse_reference(c, with_lgamma, dtype=torch.float64) -> dict:
    """ll (python float) and dmean, dscale, dW, dV by the formulas of csrc/poisson_sparse.hip's header, evaluated from the
    non-zeros of the batch's counts in plain torch (no autograd)."""
    y = batch_dense(c).to(dtype)
    mean, scale, eps, W, V = (c[k].to(dtype) for k in ("mean", "scale", "eps", "W", "V"))
    D, Lt = W.shape
    E, _, B = eps.shape
    d, n = torch.nonzero(y, as_tuple=True)
    yk = y[d, n]
    expF = torch.exp(mean + scale * eps)                                  # (E, Lt, B)
    Z = torch.einsum("kl,elk->ek", W[d], expF[:, :, n])                   # (E, nnz)
    q = yk / Z
    cl = W.sum(0)
    t = torch.einsum("l,eln->en", cl, expF)
    s = torch.einsum("n,eln->l", V, expF)
    ll = ((yk * torch.log(V[n] * Z)).sum() - (V * t).sum()) / E
    if with_lgamma:
        ll = ll - torch.lgamma(yk + 1.0).sum()
    dW = (torch.zeros(D, Lt, dtype=dtype).index_add_(0, d, torch.einsum("ek,elk->kl", q, expF[:, :, n])) - s) / E
    dexpF = torch.zeros(E, Lt, B, dtype=dtype).index_add_(2, n, torch.einsum("ek,kl->elk", q, W[d]))
    dexpF = (dexpF - V[None, None, :] * cl[None, :, None]) / E
    dV = torch.zeros(B, dtype=dtype).index_add_(0, n, yk) / V - t.sum(0) / E
    return dict(ll=float(ll), dmean=(dexpF * expF).sum(0).double(), dscale=(dexpF * expF * eps).sum(0).double(),
                dW=dW.double(), dV=dV.double())


def reference(c, with_lgamma) -> dict:
    """poisson_cases.reference (fp64 autograd of the DENSE formula) on the batch's dense counts: what the GPU tests compare
    with.  Cached there; do not modify what it returns."""
    return PC.reference(dense_view(c), with_lgamma)
