"""Case builders, the fp64 oracle and the decomposed formulas for tests/test_hip_nb_sparse.py (TEST INFRASTRUCTURE ONLY;
plain torch, importable without a GPU -- tests/test_sparse_nb_cases.py checks everything here on the CPU).

The operation is gpz_nb_nsf_sparse (csrc/nb_sparse.hip): the negative-binomial step of tests/nb_cases.py on counts held as
their non-zeros.  A *case* is a dict as ``sparse_poisson_cases.make_sparse_case`` builds it (the structure: thinned counts
of the whole data set in ``c["y"]``, ``c["idx"]`` for a batch) plus ``c["theta"]`` as ``nb_cases`` chooses it: log-spaced
0.3 ... 50 over the genes, or one given value; ``theta_over`` raises single genes' theta where a probe needs it.

The oracle is ``nb_cases.oracle``: fp64 autograd through ``NegativeBinomial.log_prob`` on ``batch_dense(c)``.
``decomposed`` evaluates the header formulas of csrc/nb_sparse.hip -- zero part plus non-zero part, no autograd.

Boundaries (the gene pass's chunk length, the kernel instances) come from the library's host-only plan query,
``ops.nb_nsf_sparse_plan``.  Probe counts as in sparse_poisson_cases: large counts at the first and last entry of every
gene chunk and at the first and last gene and spot, each worth at least ten tolerances in the value (with and without the
lgamma term), in its row of dW and in its entry of dV -- the outputs linear in y.  dtheta is logarithmic in y and is not
required to reach the aim."""
from __future__ import annotations

import math

import torch

import nb_cases as NB
import poisson_cases as PC
import sparse_poisson_cases as SC

GRADS = ("mean", "scale", "W", "V", "theta")
LL_REL, LL_ABS, G_RTOL, G_ATOL = 5e-5, 1e-3, 1e-3, 1e-3      # nb_cases.check
THETA_MAX = 50.0                                             # the top of nb_cases' range of theta


def plan(N, B, D, Lt, E, nnz=0):
    from gpzoo_amd import ops
    return ops.nb_nsf_sparse_plan(N, B, D, Lt, E, nnz)


def chunk_length() -> int:
    return plan(1037, 1037, 80, 20, 3)["gene_chunk"]


def theta_of(D, theta=None, theta_over=None) -> torch.Tensor:
    if theta is None:
        th = torch.logspace(math.log10(0.3), math.log10(THETA_MAX), D) if D > 1 else torch.tensor([0.3])
    else:
        th = torch.full((D,), float(theta))
    for d, v in (theta_over or {}).items():
        th[d] = float(v)
    return PC._f32_exact(th)


def make_nb_case(N, D, Lt, E, seed, theta=None, theta_over=None, stored_zeros=(), **kw) -> dict:
    """``sparse_poisson_cases.make_sparse_case`` plus theta.  stored_zeros: (gene, spot) positions where y is 0 and the
    SparseCounts of the GPU test nevertheless stores an entry (value 0)."""
    c = SC.make_sparse_case(N, D, Lt, E, seed, **kw)
    c["theta"] = theta_of(D, theta, theta_over)
    c["stored_zeros"] = list(stored_zeros)
    for d, n in c["stored_zeros"]:
        c["y"][d, n] = 0.0
    return c


batch_dense = SC.batch_dense
dense_view = SC.dense_view


def dense_inputs(c) -> dict:
    """The case as nb_cases.oracle reads it: the batch's parameters and its dense counts (copies: the oracle marks its
    fp64 inputs as requiring a gradient)."""
    return dict({k: c[k].clone() for k in ("mean", "scale", "eps", "W", "V", "theta")}, y=batch_dense(c))


_reference_of: dict = {}


def reference(c, with_lgamma):
    """(value, gradients) of nb_cases.oracle on the batch's dense counts.  One autograd pass per case: the gradients do not
    depend on the lgamma(y + 1) term and the value differs by its sum.  Kept per case; do not modify what it returns."""
    key = id(c)
    if key not in _reference_of:
        ll, g = NB.oracle(dense_inputs(c), with_lgamma=False)
        _reference_of[key] = (c, ll, g, float(torch.lgamma(batch_dense(c).double() + 1.0).sum()))
    _, ll, g, lg = _reference_of[key]
    return (ll - lg if with_lgamma else ll), g


def decomposed(c, with_lgamma, dtype=torch.float64):
    """(value, gradients) by the formulas at the head of csrc/nb_sparse.hip: the zero part over every (e, d, n) of the
    batch, which reads no counts, plus the non-zero part over the batch's non-zeros.  Plain torch, no autograd."""
    y = batch_dense(c).to(dtype)
    mean, scale, eps, W, V, th = (c[k].to(dtype) for k in ("mean", "scale", "eps", "W", "V", "theta"))
    E = eps.shape[0]
    expF = torch.exp(mean + scale * eps)                                  # (E, Lt, B)
    # zero part
    Z = torch.einsum("dl,eln->edn", W, expF)
    x = V * Z / th[:, None]
    u = 1.0 + x
    ll = -(th[:, None] * torch.log1p(x)).sum() / E
    G0 = -(V / u) / E                                                     # (E, D, B)
    dV = -(Z / u).sum((0, 1)) / E
    dth = (-torch.log1p(x) + x / u).sum((0, 2)) / E
    dW = torch.einsum("edn,eln->dl", G0, expF)
    dexpF = torch.einsum("dl,edn->eln", W, G0)
    # non-zero part
    d, n = torch.nonzero(y, as_tuple=True)
    yk, thk = y[d, n], th[d]
    Zk = torch.einsum("kl,elk->ek", W[d], expF[:, :, n])                  # (E, nnz)
    muk = V[n] * Zk
    r = 1.0 / (muk + thk)
    ll = ll + (yk * torch.log(muk * r)).sum() / E + (torch.lgamma(yk + thk) - torch.lgamma(thk)).sum()
    if with_lgamma:
        ll = ll - torch.lgamma(yk + 1.0).sum()
    dG = yk * thk * r / Zk / E                                            # (E, nnz)
    dW = dW.index_add(0, d, torch.einsum("ek,elk->kl", dG, expF[:, :, n]))
    dexpF = dexpF.index_add(2, n, torch.einsum("ek,kl->elk", dG, W[d]))
    dV = dV.index_add(0, n, (yk * thk * r).sum(0) / V[n] / E)
    dth = dth.index_add(0, d, torch.digamma(yk + thk) - torch.digamma(thk) - (yk * r).sum(0) / E)
    g = dict(mean=(dexpF * expF).sum(0), scale=(dexpF * expF * eps).sum(0), W=dW, V=dV, theta=dth)
    return float(ll), {k: v.double() for k, v in g.items()}


def tolerance(ref_grads, k) -> torch.Tensor:
    """The elementwise bound of nb_cases.check for gradient k."""
    want = ref_grads[k]
    return G_ATOL * (float(want.abs().max()) + 1e-30) + G_RTOL * want.abs()


def ll_tolerance(ref_ll) -> float:
    return max(LL_REL * abs(ref_ll), LL_ABS)


def sharpness(c) -> list:
    """Per probe (in the order of dense_view(c)["probes"]): what its count contributes to the value without and with the
    lgamma term, to its row of dW and to its entry of dV, in tolerances of the GPU comparison.  By the fp64 oracle alone:
    the contribution of one entry is the non-zero part's term for it, the tolerances come from ``reference``."""
    v = dense_view(c)
    (ll0, g), (ll1, _) = reference(c, False), reference(c, True)
    tW, tV = tolerance(g, "W"), tolerance(g, "V")
    expF = torch.exp(c["mean"] + c["scale"] * c["eps"])
    out = []
    for d, j, cnt in v["probes"]:
        y, th = float(cnt), c["theta"][d]
        x = expF[:, :, j]                                                 # (E, Lt)
        Z = x @ c["W"][d]
        mu = c["V"][j] * Z
        r = 1.0 / (mu + th)
        val = float((y * torch.log(mu * r)).mean() + torch.lgamma(y + th) - torch.lgamma(th))
        dWc = ((y * th * r / Z)[:, None] * x).mean(0)
        dVc = float((y * th * r).mean() / c["V"][j])
        out.append(dict(ll=abs(val) / ll_tolerance(ll0), ll_lgamma=abs(val - math.lgamma(y + 1.0)) / ll_tolerance(ll1),
                        dW=float((dWc.abs() / tW[d]).max()), dV=abs(dVc) / float(tV[j])))
    return out


def sharpen(build, positions, need=PC.SHARP_AIM):
    """build(probes, theta_over) -> case.  sparse_poisson_cases.sharpen with this file's sharpness: counts start at
    1000 + (37 i mod 1000) and grow (at most 20 000, poisson_cases.COUNT_MAX) until every probe is worth ``need``.  A probe
    that is still short at the cap has its gene's theta raised fourfold (at most to 50, the top of the range): under a
    small theta the density's tail is heavy and even a count of 20 000 changes the value by little."""
    probes, over = PC.probe_counts(positions), {}
    for _ in range(12):
        c = build(probes, dict(over))
        nxt, raised = [], dict(over)
        for (d, n, cnt), s in zip(probes, sharpness(c)):
            worst = min(s.values())
            if worst < need and cnt < PC.COUNT_MAX:
                cnt = min(PC.COUNT_MAX, int(cnt * min(max(1.5 * need / max(worst, 1e-30), 1.5), 20.0)) + 1)
            elif worst < need and float(c["theta"][d]) < THETA_MAX:
                raised[d] = min(THETA_MAX, 4.0 * float(c["theta"][d]))
            nxt.append((d, n, cnt))
        if nxt == probes and raised == over:
            break
        probes, over = nxt, raised
    return c


_cases: dict = {}


def _cached(name, fn):
    if name not in _cases:
        _cases[name] = fn()
    return _cases[name]


def _corners(D, N):
    return sorted({(0, 0), (D - 1, N - 1), (0, N - 1), (D - 1, 0)})


# 1. factor counts: both ends of the kernel instances the issue names; samples: one, a partial and more than one LDS group
# of the zero part's gene pass (4), and 33 = the host split (32 + 1)
FACTOR_SHAPES = [(130, 80, Lt, 3) for Lt in (1, 4, 5, 20, 33, 40, 63, 64)]
SAMPLE_SHAPES = [(130, 80, 7, E) for E in (1, 2, 5, 20, 33)]


def shape_case(shape):
    N, D, Lt, E = shape
    return _cached(("shape",) + tuple(shape), lambda: sharpen(
        lambda pr, over: make_nb_case(N, D, Lt, E, seed=100 + Lt + 64 * E, density=0.08, probes=pr, theta_over=over),
        _corners(D, N)))


# 2. tile edges of the zero part: nb_cases.SWEEP's (D, B, Lt, E) -- B in {1, 63, 64, 65, 500} x D in {1, 7, 130, 257}, a
# single gene over many tiles, a single spot under every gene block, a ragged 16-gene group, more than four 64-gene
# blocks, and every kernel instance of both parts
TILE_SHAPES = [(N, D, Lt, E) for D, N, Lt, E, _, _ in NB.SWEEP]


def tile_case(shape):
    N, D, Lt, E = shape
    return _cached(("tile",) + tuple(shape), lambda: sharpen(
        lambda pr, over: make_nb_case(N, D, Lt, E, seed=500 + N + D + Lt, density=0.08, probes=pr, theta_over=over),
        _corners(D, N)))


# 2b. both ends of every kernel instance of the zero part on nb_cases.INSTANCE_ENDS' shape: (B, D, Lt, E) = (68, 40, Lt, 2)
# has aligned rows, a full and a ragged spot tile, two full 16-gene groups and a partial one in a single launch of each pass
INSTANCE_END_SHAPES = [(N, D, Lt, E) for D, N, Lt, E in NB.INSTANCE_ENDS]


def instance_end_case(shape):
    N, D, Lt, E = shape
    return _cached(("ends",) + tuple(shape), lambda: sharpen(
        lambda pr, over: make_nb_case(N, D, Lt, E, seed=700 + Lt, density=0.08, probes=pr, theta_over=over),
        _corners(D, N)))


# 3. chunk boundaries
CHUNK_GENES = SC.CHUNK_GENES
CHUNK_SHAPE = (1037, 80, 20, 3)


def chunk_rows():
    C, N = chunk_length(), CHUNK_SHAPE[0]
    assert 2 * C + 1 <= N, "the chunk case needs a row of 2C + 1 non-zeros"
    lens = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1, "full": N}
    return {CHUNK_GENES[k]: SC._spread(N, m, i) for i, (k, m) in enumerate(lens.items())}


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
        lambda pr, over: make_nb_case(N, D, Lt, E, seed=201, density=0.04, rows=chunk_rows(), probes=pr, theta_over=over),
        chunk_probe_positions()))


DENSE_COLUMN_SHAPE, DENSE_COLUMN = (66, 2100, 5, 2), 31


def dense_column_case():
    N, D, Lt, E = DENSE_COLUMN_SHAPE
    return _cached("column", lambda: sharpen(
        lambda pr, over: make_nb_case(N, D, Lt, E, seed=202, density=0.02, cols={DENSE_COLUMN: range(D)}, probes=pr,
                                      theta_over=over),
        [(0, DENSE_COLUMN), (D - 1, DENSE_COLUMN), (0, 0), (D - 1, N - 1), (1049, DENSE_COLUMN)]))


# 4. degenerate structure
def empties_case():
    """Empty gene rows and spot columns, the first and the last of each among them."""
    N, D = 130, 80
    return _cached("empties", lambda: sharpen(
        lambda pr, over: make_nb_case(N, D, 20, 3, seed=301, density=0.06, empty_rows=(0, 41, D - 1),
                                      empty_cols=(0, 66, 67, N - 1), probes=pr, theta_over=over), [(1, 1), (D - 2, N - 2)]))


def no_counts_case():
    return _cached("nnz0", lambda: make_nb_case(70, 37, 5, 3, seed=302, density=0.0))


def one_count_case():
    return _cached("nnz1", lambda: make_nb_case(70, 37, 5, 3, seed=303, density=0.0, values={(21, 44): 7.0}))


def single_case():
    return _cached("1x1", lambda: make_nb_case(1, 1, 3, 2, seed=304, density=0.0, values={(0, 0): 4.0}))


STORED_ZEROS = [(0, 0), (40, 65), (79, 129), (40, 66)]


def stored_zero_case():
    """Entries the structure stores with value 0: the first and the last of both orders, one between, and the only entry
    of an otherwise empty column."""
    return _cached("stored_zero", lambda: make_nb_case(130, 80, 20, 3, seed=306, density=0.06, empty_cols=(66,),
                                                       stored_zeros=STORED_ZEROS))


def values_case():
    """Counts of 256 and more and non-integer values (poisson_cases.COUNT_VALUES)."""
    vals = {((7 * i + 3) % 80, (31 * i + 5) % 130): v for i, v in enumerate(PC.COUNT_VALUES * 6)}
    return _cached("values", lambda: make_nb_case(130, 80, 20, 3, seed=305, density=0.05, values=vals))


BIG_ROW = 5                      # the gene of big_counts_case whose counts are not integers


def big_counts_case():
    """Counts of 16 and more only, so no entry takes the recurrences; one row of non-integer counts (below 16 among them),
    so every entry of that row takes the lgamma / digamma branch whatever its size."""
    def build():
        c = make_nb_case(130, 80, 20, 3, seed=307, density=0.08)
        y = c["y"]
        y = torch.where(y != 0, y + 15.0, y)
        y[BIG_ROW] = torch.where(y[BIG_ROW] != 0, y[BIG_ROW] - 14.75, y[BIG_ROW])
        y[BIG_ROW, 7], y[BIG_ROW, 100] = 0.5, 3.25
        c["y"] = PC._f32_exact(y)
        return c
    return _cached("big", build)


# 5. batches of an N = 1037 data set
BATCH_N, BATCH_D = SC.BATCH_N, SC.BATCH_D
BATCH_EMPTY_COLS = SC.BATCH_EMPTY_COLS
BATCH_HIDDEN_GENE = SC.BATCH_HIDDEN_GENE
BATCH_NAMES = SC.BATCH_NAMES
batch_indices = SC.batch_indices


def batch_case(name):
    idx = batch_indices()[name]
    rows = {BATCH_HIDDEN_GENE: SC._spread(BATCH_N, 40, 9)}

    def build(pr, over):
        return make_nb_case(BATCH_N, BATCH_D, 20, 3, seed=400, density=0.05, idx=idx, rows=rows,
                            empty_cols=BATCH_EMPTY_COLS, probes=pr, theta_over=over)
    first, last = idx[0], idx[-1]
    if name == "empty_cols":
        first, last = idx[len(BATCH_EMPTY_COLS)], idx[-1]
    return _cached(("batch", name), lambda: sharpen(build, sorted({(0, first), (BATCH_D - 1, last)})))


# 6. near the Poisson limit: theta = 1e4 everywhere, where dtheta's terms cancel to O(1 / theta^2)
POISSON_LIMIT_SHAPE, POISSON_LIMIT_THETA = (65, 37, 5, 3), 1e4       # (B, D, Lt, E)


def poisson_limit_case():
    N, D, Lt, E = POISSON_LIMIT_SHAPE
    return _cached("limit", lambda: make_nb_case(N, D, Lt, E, seed=601, density=0.3, theta=POISSON_LIMIT_THETA))


def poisson_limit_theta_atol(c) -> torch.Tensor:
    """1e-3 sum_n |psi(y + theta) - psi(theta)| per gene, the bound tests/test_hip_nb.py::test_near_poisson_limit uses."""
    y, th = batch_dense(c), c["theta"][:, None]
    return 1e-3 * (torch.digamma(y + th) - torch.digamma(th)).abs().sum(1)


def _shape_id(s):
    return "N%d-D%d-Lt%d-E%d" % tuple(s)


def all_cases():
    """(name, case) of every case of the GPU suite."""
    out = [("factors-" + _shape_id(s), shape_case(s)) for s in FACTOR_SHAPES]
    out += [("samples-" + _shape_id(s), shape_case(s)) for s in SAMPLE_SHAPES]
    out += [("tile-" + _shape_id(s), tile_case(s)) for s in TILE_SHAPES]
    out += [("chunks", chunk_case()), ("dense_column", dense_column_case()), ("empties", empties_case()),
            ("nnz0", no_counts_case()), ("nnz1", one_count_case()), ("1x1", single_case()),
            ("stored_zero", stored_zero_case()), ("values", values_case()), ("big_counts", big_counts_case())]
    out += [("batch_" + b, batch_case(b)) for b in BATCH_NAMES]
    out += [("poisson_limit", poisson_limit_case())]
    return out
