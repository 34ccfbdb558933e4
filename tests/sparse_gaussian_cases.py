"""Case builders, the fp64 oracle and the expanded SPARSE formulas for tests/test_hip_gaussian_sparse.py (TEST INFRASTRUCTURE
ONLY; plain torch, importable without a GPU -- tests/test_sparse_gaussian_cases.py checks everything here on the CPU).

The operation is gpz_gaussian_fa_sparse (csrc/gaussian_sparse.hip): the Gaussian step of tests/gaussian_cases.py for
y = z - offset[:, None] evaluated from the stored entries of z.  A *case* is a dict: ``z`` the (D, N) fp32 matrix of the
whole data set (log1p of thinned counts over per-spot size factors, zero where the count is), ``offset`` (D,) fp64, the
parameters of ``gaussian_cases.make_inputs`` for B columns (W scaled to randn / sqrt(Lt)) and, for a batch case, ``idx``
(the spots the B columns belong to).  ``dense_inputs(c)`` is what ``gaussian_cases.oracle`` reads: the same parameters and
the fp64 dense equivalent ``z[:, idx].double() - offset[:, None]``.

The gene pass's chunk length comes from the library's own host-only plan query, ``ops.gaussian_fa_sparse_plan``; nothing
here restates it.  Probes are large values at the first and last stored entry of every chunk of the long rows and at the
first and last gene and spot.  A probe starts at 300 and, as in ``sparse_poisson_cases.sharpen``, grows until dropping or
doubling it moves every output it feeds by at least ten tolerances, judged by the fp64 oracle alone: with the noise
levels of ``gaussian_cases.make_inputs`` (1 / sd^2 spans 400 ... 0.11 across the genes) a value of 300 in a gene of sd 3 is
worth 3 tolerances in the log-likelihood and 0.3 in dmean, which both sum over all genes."""
from __future__ import annotations

import torch

import gaussian_cases as GC

PROBE = 300.0          # where every probe starts
PROBE_MAX = 1.0e5
SHARP_NEED, SHARP_AIM = 10.0, 12.0
OUTPUTS = ("value", "sse", "mean", "W", "b", "sd")
GRADS = ("mean", "scale", "W", "b", "sd")


def plan(N, B, D, Lt, nnz=0):
    from gpzoo_amd import ops
    return ops.gaussian_fa_sparse_plan(N, B, D, Lt, nnz)


def chunk_length() -> int:
    return plan(1037, 1037, 80, 20)["gene_chunk"]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def make_case(N, D, Lt, seed, density=0.08, idx=None, rows=None, empty_rows=(), empty_cols=(), probes=(), offset="center"):
    """rows: {gene: sorted list of the spots where it is stored (exactly those)}; empty_rows / empty_cols are zeroed last;
    probes: (gene, spot, value) written last; offset: "center" (the gene means of z over all N spots), "none" (zeros)
    or a number (that constant for every gene)."""
    B = N if idx is None else len(idx)
    p = GC.make_inputs(D, B, Lt, seed=seed)
    g = torch.Generator().manual_seed(70000 + 7919 * seed + 13 * N + D)
    y = torch.poisson(1.0 + 3.0 * torch.rand(D, N, generator=g, dtype=torch.float64), generator=g) + 1.0
    y = y * (torch.rand(D, N, generator=g) < density)
    sz = 0.5 + 1.5 * torch.rand(N, generator=g, dtype=torch.float64)
    for d, spots in (rows or {}).items():
        y[d, :] = 0.0
        y[d, list(spots)] = 1.0 + (torch.arange(len(spots), dtype=torch.float64) % 5)
    for d in empty_rows:
        y[d, :] = 0.0
    for n in empty_cols:
        y[:, n] = 0.0
    z = torch.log1p(y / sz[None, :]).to(torch.float32)
    for d, n, v in probes:
        z[d, n] = float(v)
    if offset == "center":
        off = z.double().mean(1)
    elif offset == "none":
        off = torch.zeros(D, dtype=torch.float64)
    else:
        off = torch.full((D,), float(offset), dtype=torch.float64)
    c = dict(mean=p["mean"], scale=p["scale"], W=p["W"] / float(Lt) ** 0.5, b=p["b"], sd=p["sd"], z=z, offset=off, N=N, B=B,
             probes=list(probes), seed=seed)
    if idx is not None:
        c["idx"] = torch.as_tensor(idx, dtype=torch.int64)
    return c


def batch_z(c) -> torch.Tensor:
    return c["z"][:, c["idx"]] if "idx" in c else c["z"]


def dense_inputs(c) -> dict:
    """The case as ``gaussian_cases.oracle`` / ``closed_form`` read it: y is the fp64 dense equivalent of the batch."""
    return dict(mean=c["mean"], scale=c["scale"], W=c["W"], b=c["b"], sd=c["sd"],
                y=batch_z(c).double() - c["offset"][:, None])


def null_ss(c) -> torch.Tensor:
    """The fp64 centred sum of squares per gene of the batch (of z: the offset cancels, and a gene without entries gives
    exactly 0)."""
    zb = batch_z(c).double()
    return ((zb - zb.mean(1, keepdim=True)) ** 2).sum(1)


def batch_probes(c):
    """The probes that lie in the batch, as (gene, batch column)."""
    if "idx" not in c:
        return list(c["probes"])
    pos = {int(n): j for j, n in enumerate(c["idx"].tolist())}
    return [(d, pos[n], v) for d, n, v in c["probes"] if n in pos]


def expression(c, device="cpu"):
    """The case's data as the library takes it: a ``SparseExpression`` (a view for a batch case)."""
    from gpzoo_amd.likelihoods import SparseCounts, SparseExpression
    e = SparseExpression(SparseCounts(c["z"]), c["offset"]).to(device)
    return e[:, c["idx"].to(device)] if "idx" in c else e


def with_probe(c, d, n, value) -> dict:
    """The case with the stored entry (gene d, spot n of the data set) set to ``value`` (0: dropped); the offset stays."""
    z = c["z"].clone()
    z[d, n] = value
    return dict(c, z=z)


def tolerances(want: GC.Oracle) -> dict:
    """What ``gaussian_cases.check`` allows each output: the value, sse per gene, and per gradient entry the smaller of its two
    bounds (1e-3 of the entry plus 1e-3 of the largest entry; of its own row's / column's magnitude)."""
    t = dict(value=max(5e-5 * abs(want.value), 1e-3), sse=1e-5 * want.sse.abs())
    for k, ref in want.grads.items():
        t[k] = torch.minimum(1e-3 * ref.abs() + 1e-3 * (float(ref.abs().max()) + 1e-30), 1e-3 * ref.abs() + 1e-3 * want.local[k])
    return t


def sharpness(c, want=None) -> list:
    """Per probe of the batch, {output: tolerances}: by how many of its tolerances the fp64 oracle's loglik, sse[d],
    dmean[:, n], dW[d], db[d] and dsd[d] move (the largest entry of a vector output) when the probe is dropped or doubled,
    the smaller of the two.  Nothing of the code under test enters."""
    want = want or GC.oracle(dense_inputs(c))
    tol = tolerances(want)
    pos = {int(n): j for j, n in enumerate(c["idx"].tolist())} if "idx" in c else None
    out = []
    for d, n, v in c["probes"]:
        j = n if pos is None else pos[n]
        worst = {k: float("inf") for k in OUTPUTS}
        for val in (0.0, 2.0 * v):
            o = GC.oracle(dense_inputs(with_probe(c, d, n, val)))
            moved = dict(value=abs(o.value - want.value) / tol["value"],
                         sse=float((o.sse[d] - want.sse[d]).abs() / tol["sse"][d]),
                         mean=float(((o.grads["mean"][:, j] - want.grads["mean"][:, j]).abs() / tol["mean"][:, j]).max()),
                         W=float(((o.grads["W"][d] - want.grads["W"][d]).abs() / tol["W"][d]).max()),
                         b=float((o.grads["b"][d] - want.grads["b"][d]).abs() / tol["b"][d]),
                         sd=float((o.grads["sd"][d] - want.grads["sd"][d]).abs() / tol["sd"][d]))
            worst = {k: min(worst[k], moved[k]) for k in OUTPUTS}
        out.append(worst)
    return out


def sharpen(build, positions, need=SHARP_AIM):
    """build(probes) -> case.  Every probe starts at PROBE and grows (at most to PROBE_MAX) until it is worth ``need``
    tolerances in every output, judged by the fp64 oracle alone (sparse_poisson_cases.sharpen's loop)."""
    probes = [(d, n, PROBE) for d, n in positions]
    for _ in range(12):
        c = build(probes)
        nxt = []
        for (d, n, v), s in zip(probes, sharpness(c)):
            worst = min(s.values())
            if worst < need and v < PROBE_MAX:
                v = min(PROBE_MAX, float(int(v * min(max(1.5 * need / max(worst, 1e-30), 1.5), 20.0)) + 1))
            nxt.append((d, n, v))
        if nxt == probes:
            break
        probes = nxt
    return c


def _spread(N, m, seed):
    """m distinct spots of N, ascending (a fixed pseudo-random subset)."""
    g = torch.Generator().manual_seed(5100 + seed)
    return sorted(torch.randperm(N, generator=g)[:m].tolist())


_cache: dict = {}


def _cached(name, fn):
    if name not in _cache:
        _cache[name] = fn()
    return _cache[name]


# 1. factor counts: the lowest and highest of the first instance, the first of the second, the notebooks' 20 and the limit
SHAPE_D, SHAPE_N = 80, 130
FACTORS = (1, 4, 5, 20, 63, 64)
CORNERS = [(0, 0), (SHAPE_D - 1, SHAPE_N - 1)]          # the first gene and spot, the last gene and spot


def shape_case(Lt):
    return _cached(("shape", Lt), lambda: sharpen(lambda pr: make_case(SHAPE_N, SHAPE_D, Lt, seed=100 + Lt, probes=pr), CORNERS))


# 2. chunk boundaries
CHUNK_GENES = {"C-1": 3, "C": 17, "C+1": 40, "2C+1": 62, "full": 79}     # the genes that carry the named row lengths
CHUNK_SHAPE = (1037, 80, 20)                                               # N, D, Lt


def chunk_rows():
    C, N = chunk_length(), CHUNK_SHAPE[0]
    assert 2 * C + 1 <= N, "the chunk case needs a row of 2C + 1 stored entries"
    lens = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1, "full": N}
    return {CHUNK_GENES[k]: _spread(N, m, i) for i, (k, m) in enumerate(lens.items())}


def chunk_probe_positions():
    """First and last entry of every chunk of the five long rows; first and last gene and spot."""
    C, (N, D, _) = chunk_length(), CHUNK_SHAPE
    out = [(0, 0), (D - 1, N - 1)]
    for d, spots in chunk_rows().items():
        for lo in range(0, len(spots), C):
            hi = min(lo + C, len(spots)) - 1
            out += [(d, spots[lo]), (d, spots[hi])]
    return sorted(set(out))


def chunk_case():
    N, D, Lt = CHUNK_SHAPE
    return _cached("chunk", lambda: sharpen(lambda pr: make_case(N, D, Lt, seed=201, density=0.04, rows=chunk_rows(), probes=pr),
                                            chunk_probe_positions()))


# 3. degenerate structure
EMPTY_ROWS, EMPTY_COLS = (0, 41, SHAPE_D - 1), (0, 66, 67, SHAPE_N - 1)


def empties_case():
    """Empty gene rows and spot columns, the first and the last of each among them."""
    return _cached("empties", lambda: sharpen(lambda pr: make_case(SHAPE_N, SHAPE_D, 20, seed=301, density=0.06, empty_rows=EMPTY_ROWS,
                                                                  empty_cols=EMPTY_COLS, probes=pr), [(1, 1), (SHAPE_D - 2, SHAPE_N - 2)]))


def single_gene_case():
    return _cached("D1", lambda: sharpen(lambda pr: make_case(SHAPE_N, 1, 5, seed=302, density=0.3, probes=pr), [(0, 0), (0, SHAPE_N - 1)]))


# 4. batch views of the N = 1037 data set: the long rows of the chunk case hold spots outside the batch
BATCH_SIZES = {"B1": 1, "B137": 137}


def batch_indices():
    N = CHUNK_SHAPE[0]
    p = torch.randperm(N, generator=torch.Generator().manual_seed(78)).tolist()
    return {"B1": [p[5]], "B137": p[:137]}


def batch_case(name):
    N, D, Lt = CHUNK_SHAPE
    idx = batch_indices()[name]
    positions = sorted({(0, idx[0]), (D - 1, idx[-1])})
    return _cached(("batch", name), lambda: sharpen(
        lambda pr: make_case(N, D, Lt, seed=400, density=0.05, idx=idx, rows=chunk_rows(), probes=pr), positions))


def descending_case():
    idx = list(range(SHAPE_N - 1, 59, -1))
    return _cached("descending", lambda: sharpen(lambda pr: make_case(SHAPE_N, SHAPE_D, 20, seed=401, idx=idx, probes=pr),
                                                 [(0, idx[0]), (SHAPE_D - 1, idx[-1])]))


# 5. the offset
def offset50_case():
    return _cached("offset50", lambda: sharpen(lambda pr: make_case(SHAPE_N, SHAPE_D, 20, seed=501, probes=pr, offset=50.0), CORNERS))


def uncentred_case():
    return _cached("center_false", lambda: sharpen(lambda pr: make_case(SHAPE_N, SHAPE_D, 20, seed=502, probes=pr, offset="none"), CORNERS))


def case_names():
    return ["Lt%d" % Lt for Lt in FACTORS] + ["chunks", "empties", "D1", "batch_B1", "batch_B137", "descending", "offset50",
                                              "center_false"]


def case(name):
    if name.startswith("Lt"):
        return shape_case(int(name[2:]))
    if name.startswith("batch_"):
        return batch_case(name[6:])
    return {"chunks": chunk_case, "empties": empties_case, "D1": single_gene_case, "descending": descending_case,
            "offset50": offset50_case, "center_false": uncentred_case}[name]()


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

def reference(name) -> GC.Oracle:
    """``gaussian_cases.oracle`` (fp64 autograd of the DENSE closed form) on the batch's dense equivalent: what the GPU tests
    compare with.  Built once per case; do not modify what it returns."""
    return _cached(("oracle", name), lambda: GC.oracle(dense_inputs(case(name))))


def sparse_formulas(c) -> dict:
    """value, sse, ss and the five gradients by the expanded formulas of csrc/gaussian_sparse.hip's header, evaluated in fp64
    from the stored entries of the batch in plain torch (no autograd)."""
    f64 = torch.float64
    z = batch_z(c).to(f64)
    m, s, W, b, sd = (c[k].to(f64) for k in ("mean", "scale", "W", "b", "sd"))
    D, Lt = W.shape
    B = m.shape[1]
    d, n = torch.nonzero(z, as_tuple=True)
    zk = z[d, n]
    a = b + c["offset"]
    iv = 1.0 / sd ** 2
    M1, G, S2 = m.sum(1), m @ m.T, (s ** 2).sum(1)
    u, H = (iv * a) @ W, (W * iv[:, None]).T @ W
    p = a[d] + (W[d] * m[:, n].T).sum(1)
    gene = lambda v: torch.zeros(D, dtype=f64).index_add_(0, d, v)
    sse = gene(zk * (zk - 2 * p)) + B * a ** 2 + 2 * a * (W @ M1) + ((W @ G) * W).sum(1)
    R = sse + (W ** 2) @ S2
    value = (-B * (torch.log(sd) + 0.91893853320467274178) - 0.5 * iv * R).sum()
    dmean = torch.zeros(B, Lt, dtype=f64).index_add_(0, n, (iv[d] * zk)[:, None] * W[d]).T - u[:, None] - H @ m
    dscale = -s * torch.diagonal(H)[:, None]
    zm = torch.zeros(D, Lt, dtype=f64).index_add_(0, d, zk[:, None] * m[:, n].T)
    dW = iv[:, None] * (zm - a[:, None] * M1[None, :] - W @ G - S2[None, :] * W)
    db = iv * (gene(zk) - B * a - W @ M1)
    dsd = -B / sd + R / sd ** 3
    ss = gene(zk ** 2) - gene(zk) ** 2 / B
    return dict(value=float(value), sse=sse, ss=ss, grads=dict(mean=dmean, scale=dscale, W=dW, b=db, sd=dsd))


def run(c, grads=True, shift=0, device="cuda"):
    """The fused sparse step on the GPU: (loglik, sse, ss, dict of gradients keyed like the oracle's).  ``shift`` > 0 passes
    ``mean`` and ``W`` as the views ``t[shift:]`` of longer buffers (misaligned for shift % 4 != 0)."""
    from gpzoo_amd import ops

    def dev(t, sh=0):
        if not sh:
            return t.to(device)
        buf = torch.zeros(t.numel() + sh, dtype=t.dtype, device=device)
        buf[sh:] = t.reshape(-1).to(device)
        return buf[sh:].view(t.shape)
    out = ops.gaussian_fa_sparse(dev(c["mean"], shift), dev(c["scale"]), dev(c["W"], shift), dev(c["b"]), dev(c["sd"]),
                                 expression(c, device), grads=grads)
    return out[0], out[1], out[2], dict(zip(GRADS, out[3:]))
