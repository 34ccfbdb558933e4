"""Case builders and the fp64 reference for tests/test_hip_backward_forms.py (TEST INFRASTRUCTURE ONLY; plain torch,
importable without a GPU -- tests/test_backward_forms_cases.py checks everything here on the CPU).

A *case* is one problem (inputs drawn by gpzoo_amd.synthetic.make_config, then a kernel family, an input dimension and
optionally one of the two clamp recipes); an *upstream* is what a loss sends back into the pass:

    loss = sum(mean * gm) + sum(scale * gs) + sum_l w_l kl_l  (+ sum(chol * gc) when kernel gradients are asked for)

differentiated by torch autograd in fp64 through oracle/svgp_oracle.py (Matern matrices from tests/matern_oracle.py,
whose masked square root gives the library's stated zero gradient at zero distance) with respect to mu, Lu_raw, Z,
sigma, lengthscale and, multi-group, group_diff.  Nothing here names a device: the tensors of a case decide where the
oracle runs.

Every floating-point input is rounded to an fp32-representable value, so the fp32 and fp64 kernels and the oracle
evaluate the same problem."""
from __future__ import annotations

import math

import torch

KINDS = ("nsf_rbf", "rbf_scalar", "matern12", "matern32", "matern52", "mggp_nsf_rbf")
NAMES = ("mu", "Lu_raw", "Z", "sigma", "lengthscale", "group_diff")
CLAMP_MIN_RECIPE = 0.1        # var_clamp_min of the un-whitened clamp recipe
NEAR = 1e-2                   # columns this close (relative) to a clamp threshold are taken out of the scale upstream


def pad128(n: int) -> int:
    return (n + 127) // 128 * 128


# ---------------------------------------------------------------------------------------------------------------------
# the library's own launch arithmetic, restated (csrc/svgp.hip make_plan, csrc/gemmw.hip wide_nt_pieces / wide_nt_launch)
# ---------------------------------------------------------------------------------------------------------------------

def chunk_columns(N: int, M: int, L: int, chunk: int = 0) -> int:
    """Columns per chunk (make_plan): the automatic chunk holds every shape used here whole."""
    if chunk <= 0:
        chunk = max(2048, int(6.0 * (1 << 30) / (2.0 * L * pad128(M) * 8)))
    return pad128(min(chunk, N))


def nt_tiles(nblk: int) -> int:
    if nblk <= 4:
        return nblk * (nblk + 1) // 2
    mt = (nblk + 1) // 2
    return mt * (mt + 1) - (nblk & 1)


def wide_nt_pieces(Mp: int, K: int, L: int) -> int:
    """Pieces S the wide A B^T accumulation cuts its k extent K into (gemmw.hip)."""
    tiles = nt_tiles(Mp // 128) * L
    if tiles >= 384:
        r, best, best_cost = tiles / 512.0, 1, 1e30
        for S in range(1, 5):
            if S > 1 and K // S < 2048:
                break
            rounds = r * S
            cost = math.ceil(rounds - 1e-9) / rounds * (1.0 + 0.015 * (S - 1))
            if cost < best_cost - 1e-9:
                best_cost, best = cost, S
        return best
    S = (1024 if Mp // 128 <= 4 else 512) // tiles
    return max(min(S, K // 1024, 16), 1)


def piece_extent(Mp: int, K: int, L: int) -> int:
    """Ks of wide_nt_launch: ceil(ceil(K / S) / 32) * 32."""
    S = wide_nt_pieces(Mp, K, L)
    return ((K + S - 1) // S + 31) // 32 * 32


def probe_columns(N: int, M: int, L: int, chunk: int = 0) -> list:
    """Column 0 and N-1, both sides of every chunk boundary, both sides of every piece boundary Ks inside a chunk."""
    Mp, nc = pad128(M), chunk_columns(N, M, L, chunk)
    cols = {0, N - 1}
    for n0 in range(0, N, nc):
        if n0:
            cols.update((n0 - 1, n0))
        nreal = min(nc, N - n0)
        Ks = piece_extent(Mp, pad128(nreal), L)
        for b in range(n0 + Ks, n0 + nreal, Ks):
            cols.update((b - 1, b))
    return sorted(c for c in cols if 0 <= c < N)


def library_picks_algebra(N: int, M: int, full: bool, f32: bool, whitened: bool) -> bool:
    """The rule in backward_algebra's comment (csrc/svgp.hip): mu / Lu only iff N >= 0.75 Mp; all parameters iff
    N >= 2.2 Mp, un-whitened fp32 (whose M x M products run in fp64) iff N >= 4.4 Mp."""
    Mp = pad128(M)
    if not full:
        return 4 * N >= 3 * Mp
    return 10 * N >= (44 if (f32 and not whitened) else 22) * Mp


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

def _f32_exact(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float64)


def make_case(N: int, M: int, L: int, kind: str = "nsf_rbf", d: int = 2, recipe: str | None = None) -> dict:
    """fp64 CPU tensors of one problem.  ``recipe``: None, "whitened_clamp" (Z = X[50:50+M], jitter -0.02, lengthscale
    3: the data points that coincide with inducing points sit at the whitened clamp) or "unwhitened_clamp" (a tiny
    Lu and var_clamp_min = 0.1: part of the columns sit at the variance clamp)."""
    from gpzoo_amd.synthetic import make_config
    assert kind in KINDS and d in (1, 2, 3)
    cfg = 5 if kind == "mggp_nsf_rbf" else 3 if kind.startswith("matern") else 2
    c = make_config(cfg, N=N, M=M, L=L, dtype=torch.float64, kind=kind if cfg == 3 else None)
    out = dict(kind=kind, N=N, M=M, L=L, d=d, recipe=recipe, jitter=float(c["jitter"]), clamp_min=1e-6)
    X, Z = c["X"], c["Z"]
    gen = torch.Generator().manual_seed(1234 + 7 * N + 3 * M + L)
    if Z.shape[0] < M:     # N < M: the configuration draws its inducing points among the data points; the rest are drawn here
        more = M - Z.shape[0]
        Z = torch.cat([Z, (torch.rand(more, 2, generator=gen, dtype=torch.float64) - 0.5) * 200.0])
        if "gZ" in c:
            c["gZ"] = torch.cat([c["gZ"], torch.randint(0, int(c["n_groups"]), (more,), generator=gen)])
    if d == 1:
        X, Z = X[:, :1].contiguous(), Z[:, :1].contiguous()
    elif d == 3:           # a third coordinate; the inducing points stay data points (zero distances on the Matern paths)
        rows = torch.cdist(Z, X).argmin(1)
        X = torch.cat([X, (torch.rand(N, 1, generator=torch.Generator().manual_seed(77), dtype=torch.float64) - 0.5) * 200.0], 1)
        Z = X[rows].clone()
    out.update(X=X, Z=Z, mu=c["mu"], Lu_raw=c["Lu_raw"].double(),
               sigma=torch.linspace(0.8, 1.3, L, dtype=torch.float64) if L > 1 else torch.tensor([0.9], dtype=torch.float64),
               lengthscale=c["lengthscale"].reshape(-1))
    if kind == "mggp_nsf_rbf":
        out.update(gX=c["gX"], gZ=c["gZ"], n_groups=int(c["n_groups"]),
                   group_diff=torch.linspace(0.5, 0.9, L, dtype=torch.float64) * (1 - 2 * (torch.arange(L) % 2)).double())
    if recipe == "whitened_clamp":
        assert kind == "nsf_rbf" and d == 2 and M <= 200, "the recipe is positive-definite only at M <= 200"
        out["Z"] = X[50:50 + M].clone()
        out["jitter"] = -0.02
        out["sigma"] = torch.ones(L, dtype=torch.float64)
        out["lengthscale"] = torch.full((L,), 3.0, dtype=torch.float64)
    elif recipe == "unwhitened_clamp":
        assert kind == "nsf_rbf" and d == 2
        Lu = (0.02 * torch.randn(L, M, M, generator=gen, dtype=torch.float64)).tril(-1)
        Lu.diagonal(dim1=-2, dim2=-1).fill_(-3.0)
        out["Lu_raw"] = Lu
        out["sigma"] = torch.ones(L, dtype=torch.float64)
        # (with the configuration's own lengthscales, 3 to 12, the shortest latent of N=2100, M=200 has 1.6 % of its
        # columns at the clamp: too few for the per-latent condition the CPU test asserts)
        out["lengthscale"] = torch.linspace(9.0, 12.0, L, dtype=torch.float64)
        out["clamp_min"] = CLAMP_MIN_RECIPE
    else:
        assert recipe is None
    for k, v in out.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            out[k] = _f32_exact(v)
    return out


def case_key(c: dict) -> tuple:
    return (c["N"], c["M"], c["L"], c["kind"], c["d"], c["recipe"])


def embedding_of(c: dict) -> torch.Tensor:
    from oracle import svgp_oracle as O
    G = c["n_groups"]
    return O.embed_group_distances(torch.ones(G, G) - torch.eye(G)).double()


def forward_parts(c: dict, leaf: dict, whitened: bool) -> dict:
    """mean, scale, kl, chol and the variance before its clamp, on the device and in the precision of the leaves."""
    from oracle import svgp_oracle as O
    import matern_oracle as MO
    X = c["X"].to(leaf["Z"])
    dev, dt = X.device, X.dtype
    kind = c["kind"]
    if kind in ("nsf_rbf", "rbf_scalar"):
        K = lambda A, B, gA, gB: O.kernel_matrix("nsf_rbf", A, B, leaf["sigma"], leaf["lengthscale"])   # noqa: E731
    elif kind == "mggp_nsf_rbf":
        emb = embedding_of(c).to(device=dev, dtype=dt)
        K = lambda A, B, gA, gB: O.kernel_matrix(kind, A, B, leaf["sigma"], leaf["lengthscale"], gA=gA.to(dev),   # noqa: E731
                                                 gB=gB.to(dev), embedding=emb, group_diff=leaf["group_diff"])
    else:
        K = lambda A, B, gA, gB: MO.kernel_matrix(kind, A, B, leaf["sigma"], leaf["lengthscale"])       # noqa: E731
    gX, gZ = c.get("gX"), c.get("gZ")
    Kzx = K(leaf["Z"], X, gZ, gX)
    Kzz = K(leaf["Z"], leaf["Z"], gZ, gZ) + c["jitter"] * torch.eye(c["M"], dtype=dt, device=dev)
    Kxx = (leaf["sigma"] ** 2)[:, None].expand(-1, c["N"])
    if whitened:
        mean, scale, Lu, chol = O.wsvgp_moments(Kxx, Kzx, Kzz, leaf["mu"], leaf["Lu_raw"])
        kl = O.whitened_kl(leaf["mu"], Lu)
        with torch.no_grad():      # what gp.py:287 clamps at 0, relative to sigma^2
            W = torch.linalg.solve_triangular(chol, Kzx, upper=False)
            raw, thr, ref = Kxx - (W ** 2).sum(1), 0.0, Kxx
    else:
        mean, scale, Lu, chol = O.svgp_moments(Kxx, Kzx, Kzz, leaf["mu"], leaf["Lu_raw"], c["clamp_min"])
        kl = O.mvn_kl(leaf["mu"], Lu, chol)
        with torch.no_grad():      # the variance utilities.py:397 clamps at clamp_min
            W = torch.cholesky_solve(Kzx, chol)
            S = Lu @ Lu.transpose(-2, -1)
            raw = Kxx + ((W.transpose(-2, -1) @ (S - Kzz)) * W.transpose(-2, -1)).sum(-1)
            thr, ref = c["clamp_min"], torch.full_like(Kxx, c["clamp_min"])
    return dict(mean=mean, scale=scale, kl=kl, chol=chol, raw=raw.detach(), clamped=(raw <= thr).detach(),
                near=((raw - thr).abs() <= NEAR * ref).detach())


def make_leaves(c: dict, device="cpu", dtype=torch.float64, requires_grad: bool = True) -> dict:
    return {k: c[k].to(device=device, dtype=dtype).clone().requires_grad_(requires_grad) for k in NAMES if k in c}


_near_cache: dict = {}


def near_columns(c: dict, whitened: bool, device="cpu") -> torch.Tensor:
    """(L,N) bool, CPU: columns whose unclamped quantity lies within NEAR (relative) of its clamp threshold, judged by
    the fp64 oracle once per case (on ``device`` if this is the first request), so every evaluation of a case zeroes
    the same entries of gs."""
    key = case_key(c) + (whitened,)
    if key not in _near_cache:
        with torch.no_grad():
            _near_cache[key] = forward_parts(c, make_leaves(c, device, requires_grad=False), whitened)["near"].cpu()
    return _near_cache[key]


def make_upstream(c: dict, whitened: bool, which: str, chunk: int = 0, device="cpu") -> dict:
    """gm, gs (L,N), w (L,), gc (L,M,M) on the CPU in fp64 (fp32-representable).  ``which``: "dense" (seeded randn) or
    "probe" (gm and gs non-zero only on probe_columns(...), there of size 1 to 2 with either sign)."""
    N, M, L = c["N"], c["M"], c["L"]
    g = torch.Generator().manual_seed(4321 + N + 5 * M + 11 * L)
    gm = torch.randn(L, N, generator=g, dtype=torch.float64)
    gs = torch.randn(L, N, generator=g, dtype=torch.float64)
    w = torch.randn(L, generator=g, dtype=torch.float64)
    gc = torch.randn(L, M, M, generator=g, dtype=torch.float64)
    if which == "probe":
        cols = torch.tensor(probe_columns(N, M, L, chunk))
        mask = torch.zeros(N, dtype=torch.bool)
        mask[cols] = True
        unit = lambda t: torch.where(mask, torch.sign(t) * (1.0 + (t.abs() % 1.0)), torch.zeros_like(t))   # noqa: E731
        gm, gs = unit(gm), unit(gs)
    else:
        assert which == "dense"
    gs = torch.where(near_columns(c, whitened, device), torch.zeros_like(gs), gs)
    return {k: _f32_exact(v) for k, v in dict(gm=gm, gs=gs, w=w, gc=gc).items()}


def oracle_loss(c: dict, leaf: dict, whitened: bool, up: dict, kernel_grads: bool = True):
    """The scalar loss and the forward parts; ``up`` is moved to the leaves' device and precision."""
    p = forward_parts(c, leaf, whitened)
    u = {k: v.to(leaf["mu"]) for k, v in up.items()}
    loss = (p["mean"] * u["gm"]).sum() + (p["scale"] * u["gs"]).sum() + (u["w"] * p["kl"]).sum()
    if kernel_grads:
        loss = loss + (p["chol"] * u["gc"]).sum()
    return loss, p


_grad_cache: dict = {}


def oracle_grads(c: dict, whitened: bool, which: str, chunk: int = 0, device="cpu", dtype=torch.float64) -> dict:
    """Gradients of the all-parameter loss (CPU fp64 tensors) plus mean / scale, cached per (case, whitened, upstream,
    probe chunking, precision) so that every form and precision variant shares one evaluation.  mu and Lu_raw do not
    reach chol, so their gradients also serve the runs without kernel gradients."""
    key = case_key(c) + (whitened, which, chunk if which == "probe" else 0, str(dtype))
    if key not in _grad_cache:
        leaf = make_leaves(c, device, dtype)
        loss, p = oracle_loss(c, leaf, whitened, make_upstream(c, whitened, which, chunk, device), True)
        loss.backward()
        out = {k: v.grad.detach().double().cpu() for k, v in leaf.items()}
        out.update(mean=p["mean"].detach().double().cpu(), scale=p["scale"].detach().double().cpu(),
                   clamped=p["clamped"].cpu())
        _grad_cache[key] = out
    return _grad_cache[key]
