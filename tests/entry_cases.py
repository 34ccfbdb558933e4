"""Case builders, the restated launch arithmetic and the fp64 references for tests/test_hip_kernel_entries.py and
tests/test_hip_precomputed.py (TEST INFRASTRUCTURE ONLY; plain torch, importable without a GPU -- tests/test_entry_cases.py
checks everything here on the CPU).

The entries are the ones the module API calls on their own:

    gpz_kfill                         K[l,i,j] = k_l(A_i, B_j)                                     csrc/kfill.hip
    gpz_kgrad                         Kbar -> d/d(sigma, lengthscale, a) (L,3) and d/dA (nA,d)     csrc/kgrad.hip, mmops.hip
    gpz_wsvgp_precomputed(_backward)  q(F) moments from a caller's W (L,N,M), and their backward   csrc/svgp.hip

Kernel values come from the project's fp64 oracles (oracle/svgp_oracle.py::kernel_matrix, tests/matern_oracle.py::
kernel_matrix with its masked square root at r = 0), their gradients from torch autograd on fp64 leaves; the precomputed
moments are the reference's expression (gp.py:308-322) written out in torch.  Every floating-point input is rounded to an
fp32-representable value: the fp32 kernels, the fp64 kernels and the reference see one problem."""
from __future__ import annotations

import math

import torch

import matern_oracle as MO
from oracle import svgp_oracle as O

# kernel kinds, with the library's ids (include/gpzoo_hip.h, csrc/kfill.hip:67)
KIND_ID = {"rbf": 0, "matern32": 1, "mggp": 2, "distance": 3, "matern12": 4, "matern52": 5}
KINDS = ("rbf", "matern12", "matern32", "matern52", "mggp", "distance")
GRAD_KINDS = KINDS[:5]                      # the plain distance has no parameters (gpz_kgrad refuses it)
SIG, ELL, GA = (1.0, 0.8, 1.3), (2.5, 4.0, 6.0), (0.7, 0.4, 1.1)
KF_TX, KF_TY, KF_MAXL, KF_MAXTAB = 64, 4, 256, 2048       # csrc/kfill.hip:21-32


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def pad128(v: int) -> int:
    return cdiv(v, 128) * 128                # csrc/common.h:15 pad_up


def r32(t: torch.Tensor) -> torch.Tensor:
    """fp64 tensor of fp32-representable values."""
    return t.float().double()


def per_latent(base, L: int) -> torch.Tensor:
    """base cycled over the latents and scaled by 1 + l / (4 L): all L values distinct (a latent offset error in a
    split launch changes the values)."""
    return r32(torch.tensor([base[l % len(base)] * (1.0 + l / (4.0 * L)) for l in range(L)], dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# the library's own launch arithmetic, restated
# ---------------------------------------------------------------------------------------------------------------------

def kfill_plan(kind: str, L: int, nA: int, nB: int, out_f64: bool, G: int = 0, ldk: int | None = None,
               stride: int | None = None, base_off: int = 0) -> dict:
    """launch_kfill (csrc/kfill.hip:192-230).  base_off: elements between a 16-byte aligned address and K."""
    VEC, esz = (2, 8) if out_f64 else (4, 4)                          # kfill.hip:48-49 VecOf
    ldk = nB if ldk is None else ldk
    stride = nA * ldk if stride is None else stride
    # kfill.hip:195-196 vec_ok
    vec_ok = (base_off * esz) % 16 == 0 and (ldk * esz) % 16 == 0 and (stride * esz) % 16 == 0 and nB % VEC == 0
    lmax = KF_MAXL                                                    # kfill.hip:201-206
    if kind == "mggp":
        assert 1 <= G and G * G <= KF_MAXTAB
        lmax = min(KF_MAXTAB // (G * G), KF_MAXL)
    return dict(VEC=VEC, vec_ok=vec_ok, col_blocks=cdiv(nB, KF_TX * VEC), row_blocks=cdiv(nA, KF_TY),   # kfill.hip:198-199
                col_tail=nB % VEC, lmax=lmax, launches=cdiv(L, lmax))                                   # kfill.hip:208


def kgrad_plan(nB: int) -> dict:
    """The column loop of kgrad_kernel (csrc/kgrad.hip:53-54): trips of 4 slots of 64 columns; `slots` and `tail` describe
    the last trip (slots in use, lanes of its last slot; 0 = all 64)."""
    trips = cdiv(nB, 256)
    last = nB - 256 * (trips - 1)
    return dict(trips=trips, slots=cdiv(last, 64), tail=last % 64)


def kgrad_tail_class(nB: int) -> tuple:
    """(more than one trip, slots of the last trip, one lane / ragged / full last slot)."""
    p = kgrad_plan(nB)
    return (p["trips"] > 1, p["slots"], "one" if p["tail"] == 1 else "full" if p["tail"] == 0 else "ragged")


def kgrad_finish_fx(nA: int, L: int) -> tuple:
    """kgrad_finish (csrc/mmops.hip:258): fx = max(ceil(M / 256), L), and which side set it."""
    mb = cdiv(nA, 256)
    return max(mb, L), ("rows" if mb > L else "latents")


def pre_plan(L: int, N: int, M: int, esz: int, chunk: int = 0) -> dict:
    """pre_plan (csrc/svgp.hip) under a chunk width (0: the 2 GiB rule with its 1024 floor)."""
    Mp = pad128(M)
    cw = int(2.0 * (1 << 30) / (float(L) * Mp * esz))
    cw = max(cw, 1024)
    if chunk > 0:
        cw = chunk
    nc = pad128(min(cw, N))
    nchunks = cdiv(N, nc)
    last = N - (nchunks - 1) * nc
    return dict(Mp=Mp, nblk=Mp // 128, nc=nc, nchunks=nchunks, last=last, ncp_last=pad128(last))


# ---------------------------------------------------------------------------------------------------------------------
# kernel-matrix cases
# ---------------------------------------------------------------------------------------------------------------------

def kernel_case(kind: str, d: int, nA: int, nB: int, L: int = 3, seed: int = 0, G: int = 5, same: bool = False) -> dict:
    """Points uniform on [-4, 4]^d; per-latent sigma, lengthscale and a all distinct.  MGGP: G groups with a random 2-D
    embedding, every group on both sides wherever the side has at least G points.  same: B is A (K(Z, Z))."""
    g = torch.Generator().manual_seed(1000 * KIND_ID[kind] + 100 * d + seed)
    A = r32((torch.rand(nA, d, generator=g, dtype=torch.float64) - 0.5) * 8)
    B = A if same else r32((torch.rand(nB, d, generator=g, dtype=torch.float64) - 0.5) * 8)
    c = dict(kind=kind, d=d, nA=nA, nB=A.shape[0] if same else nB, L=L, A=A, B=B, sigma=per_latent(SIG, L),
             ell=per_latent(ELL, L), a=None, G=0)
    if kind == "distance":
        c["L"], c["sigma"], c["ell"] = 1, torch.ones(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64)
    if kind == "mggp":
        c["G"], c["a"] = G, per_latent(GA, L)
        c["emb"] = r32(torch.randn(G, 2, generator=g, dtype=torch.float64) * 0.8)
        c["gA"] = group_ids(nA, G)[torch.randperm(nA, generator=g)]
        c["gB"] = c["gA"] if same else group_ids(nB, G)[torch.randperm(nB, generator=g)]
    return c


def group_ids(n: int, G: int) -> torch.Tensor:
    """Every group where n >= G; fewer points than groups take ids from both ends of the range (G-1, 0, G-2, 1, ...), so the
    last entries of the (G, G) table are read."""
    i = torch.arange(n)
    return i % G if n >= G else torch.where(i % 2 == 0, G - 1 - i // 2, i // 2)


def kernel_value(c: dict, A=None, B=None, sigma=None, ell=None, a=None) -> torch.Tensor:
    """(L, nA, nB) from the oracles, in the precision of the arguments (the case's own fp64 tensors by default)."""
    A = c["A"] if A is None else A
    B = c["B"] if B is None else B
    sigma = c["sigma"] if sigma is None else sigma
    ell = c["ell"] if ell is None else ell
    k = c["kind"]
    if k == "rbf":
        return O.kernel_matrix("batched_rbf", A, B, sigma, ell)
    if k in ("matern12", "matern32", "matern52"):
        return MO.kernel_matrix(k, A, B, sigma, ell)
    if k == "mggp":        # |a| r_g^2 + 1 and p = d: group_pow = d / 2 (oracle kind batched_mggp_rbf; a > 0 here)
        return O.kernel_matrix("batched_mggp_rbf", A, B, sigma, ell, gA=c["gA"], gB=c["gB"], embedding=c["emb"].to(A.dtype),
                               group_diff=c["a"] if a is None else a)
    return MO.masked_distance(A, B)[None]


def kernel_grads(c: dict, Kbar: torch.Tensor, dtype=torch.float64) -> dict:
    """Autograd of sum(K * Kbar): theta (L,3) = d/d(sigma, lengthscale, a) (a column of zeros without a) and A (nA,d)."""
    leaves = [c[n].to(dtype).clone().requires_grad_(True) for n in ("A", "sigma", "ell")]
    if c["a"] is not None:
        leaves.append(c["a"].to(dtype).clone().requires_grad_(True))
    K = kernel_value(c, leaves[0], c["B"].to(dtype), leaves[1], leaves[2], leaves[3] if c["a"] is not None else None)
    g = torch.autograd.grad((K * Kbar.to(dtype)).sum(), leaves)
    ga = g[3] if c["a"] is not None else torch.zeros_like(g[1])
    return dict(theta=torch.stack([g[1], g[2], ga], 1), A=g[0])


def probe_columns(nB: int) -> list:
    """First and last column and the two columns next to each 64-column boundary (every 256-column boundary is one)."""
    cols = {0, nB - 1}
    for b in range(64, nB, 64):
        cols |= {b - 1, b}
    return sorted(cols)


def upstreams(c: dict) -> dict:
    """dense: randn.  probe: O(1) entries of either sign in probe_columns, zero elsewhere."""
    g = torch.Generator().manual_seed(7 + c["nA"] + 3 * c["nB"] + 11 * c["d"])
    L, nA, nB = c["L"], c["nA"], c["nB"]
    dense = r32(torch.randn(L, nA, nB, generator=g, dtype=torch.float64))
    cols = probe_columns(nB)
    mag = 0.75 + 0.5 * torch.rand(L, nA, len(cols), generator=g, dtype=torch.float64)
    sgn = torch.where(torch.rand(L, nA, len(cols), generator=g) < 0.5, -1.0, 1.0).double()
    probe = torch.zeros(L, nA, nB, dtype=torch.float64)
    probe[:, :, cols] = r32(mag * sgn)
    return dict(dense=dense, probe=probe)


def grad_tol(ref: torch.Tensor, dtype) -> torch.Tensor:
    """Element-wise tolerance of tests/test_hip_kernel_grads.py::_close."""
    top = float(ref.abs().max())
    if dtype == torch.float64:
        return 1e-9 * max(1.0, top) + 1e-5 * ref.abs()
    return 1e-3 * max(1e-3, top) + 1e-3 * ref.abs()


# fp32 inputs written in fp64: (rtol, atol) of tests/test_hip_matern_family.py
VALUE_TOL_MIXED = (1e-5, 1e-6)

# case lists ----------------------------------------------------------------------------------------------------------
MAIN_FILL = (9, 261)                                        # (nA, nB) of the kinds x d x precision grid
SWEEP_NA = (1, 3, 4, 5)
SWEEP_NB_F32 = (1, 2, 3, 4, 5, 255, 256, 257, 258, 260, 513)     # 2 and 258: the column tail of length 2
SWEEP_NB_F64 = (1, 2, 3, 127, 128, 129, 130, 256, 257)       # 130, 256: vector stores in a second column block
FILL_SPLITS = [("rbf", L, 0) for L in (256, 257, 600)] + [("mggp", 227, 3), ("mggp", 228, 3), ("mggp", 32, 8),
                                                          ("mggp", 33, 8), ("mggp", 65, 8), ("mggp", 3, 45)]
SPLIT_SHAPE = (5, 9)
ABI_LDK_PAD, ABI_STRIDE_PAD, ABI_BASE, ABI_NB, ABI_NA = (0, 1, 3, 4), (0, 5), (0, 1), (5, 8), 3
TALL = (4 * 65536 + 1, 5)

MAIN_GRAD = (5, 257)
GRAD_SWEEP_KINDS = ("rbf", "matern12", "mggp")
GRAD_SWEEP_NB = (1, 63, 64, 65, 130, 255, 256, 257, 511, 512, 513, 1025)     # 130: the last trip ends in slot u = 2
FINISH_CASES = ((1025, 5, 1), (5, 65, 7))                   # (nA, nB, L): ceil(nA / 256) > L, and L > ceil(nA / 256)


def fill_plans() -> list:
    """Every stand-alone kfill launch shape of tests/test_hip_kernel_entries.py: (kind, plan)."""
    out = []
    for kind in KINDS:
        for f64 in (False, True):
            out.append((kind, kfill_plan(kind, 3, *MAIN_FILL, f64, G=5)))
    for kind in ("rbf", "mggp"):      # fp64 outputs run from fp32 and from fp64 inputs
        for f64, nbs in ((False, SWEEP_NB_F32), (True, SWEEP_NB_F64)):
            out += [(kind, kfill_plan(kind, 3, nA, nB, f64, G=5)) for nA in SWEEP_NA for nB in nbs]
    out += [(kind, dict(kfill_plan(kind, L, *SPLIT_SHAPE, False, G=G), L=L)) for kind, L, G in FILL_SPLITS]
    for f64 in (False, True):
        for nB in ABI_NB:
            for lp in ABI_LDK_PAD:
                for sp in ABI_STRIDE_PAD:
                    for off in ABI_BASE:
                        ldk = nB + lp
                        out.append(("rbf", kfill_plan("rbf", 2, ABI_NA, nB, f64, ldk=ldk, stride=ABI_NA * ldk + sp,
                                                      base_off=off)))
    return out


def grad_cases() -> list:
    """Every stand-alone kgrad case: (name, kernel_case)."""
    out = []
    for kind in GRAD_KINDS:
        for d in (1, 2, 3, 4):
            out.append((f"main-{kind}-d{d}", kernel_case(kind, d, *MAIN_GRAD)))
    for kind in GRAD_SWEEP_KINDS:
        for nA in SWEEP_NA:
            for nB in GRAD_SWEEP_NB:
                out.append((f"sweep-{kind}-{nA}x{nB}", kernel_case(kind, 2, nA, nB, seed=nA)))
    for nA, nB, L in FINISH_CASES:
        out.append((f"finish-{nA}x{nB}-L{L}", kernel_case("rbf", 2, nA, nB, L=L)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# WSVGP.forward_precomputed
# ---------------------------------------------------------------------------------------------------------------------
R_CLAMPED, R_UNCLAMPED = (0.5, 0.8, 1.25, 1.6), (0.5, 0.8)
PRE_SHAPES = ((1, 1, 1), (2, 129, 33), (2, 128, 32), (3, 257, 129), (2, 300, 257), (2, 1300, 130))    # (L, N, M)
CHUNK_WIDTHS, CHUNK_N, CHUNK_M = (128, 256), (256, 300, 257), (33, 257)


def precomputed_case(L: int, N: int, M: int, clamped: bool = True, seed: int = 0, shared: bool = False,
                     scalar_sigma: bool = False, boost_last: float = 1.0) -> dict:
    """W = randn with row n of latent l scaled to norm r_n sigma_l, r_n cycling R_CLAMPED (or R_UNCLAMPED): sigma^2 - sum W^2
    is {0.75, 0.36, -0.56, -1.56} sigma^2, so half of the points sit at the clamp in every latent and none is closer to it
    than 0.36 sigma^2.  shared: one q(U) (mu (M,), Lu (M,M)) for the L rows of W.  boost_last: factor on the upstreams of the
    last column (the cases whose last chunk is that one column; see tests/test_entry_cases.py)."""
    g = torch.Generator().manual_seed(90000 + 1000 * L + 7 * N + M + seed + (50 if clamped else 0))
    sigma = r32(torch.tensor(1.1, dtype=torch.float64)) if scalar_sigma else per_latent(SIG, L)
    rc = R_CLAMPED if clamped else R_UNCLAMPED
    r = torch.tensor([rc[n % len(rc)] for n in range(N)], dtype=torch.float64)
    W = torch.randn(L, N, M, generator=g, dtype=torch.float64)
    W = r32(W / W.norm(dim=-1, keepdim=True) * r[None, :, None] * sigma.reshape(-1, 1, 1))
    mu = r32(torch.randn((M,) if shared else (L, M), generator=g, dtype=torch.float64))
    Lu_raw = r32(0.3 * torch.randn((M, M) if shared else (L, M, M), generator=g, dtype=torch.float64) / math.sqrt(M))
    R1 = r32(torch.randn(L, N, generator=g, dtype=torch.float64))
    R2 = r32(torch.rand(L, N, generator=g, dtype=torch.float64))
    R1[:, -1] *= boost_last
    R2[:, -1] *= boost_last
    return dict(L=L, N=N, M=M, W=W, sigma=sigma, mu=mu, Lu_raw=Lu_raw, R1=R1, R2=R2, clamped=clamped, shared=shared)


def precomputed_ref(c: dict, dtype=torch.float64, keep=None, use_mean: bool = True, use_scale: bool = True) -> dict:
    """The reference's expression (gp.py:308-322) and, by autograd, the gradients of sum(mean R1) + sum(scale R2) with respect
    to mu, the raw Lu and sigma.  keep: index of the columns of W that take part (all by default)."""
    W, R1, R2 = (c[n].to(dtype) for n in ("W", "R1", "R2"))
    if keep is not None:
        W, R1, R2 = W[:, keep], R1[:, keep], R2[:, keep]
    mu, Lur, sig = (c[n].to(dtype).clone().requires_grad_(True) for n in ("mu", "Lu_raw", "sigma"))
    Lu = Lur.tril(-1) + torch.diag_embed(torch.diagonal(Lur, dim1=-2, dim2=-1).exp())
    s2 = (sig ** 2).reshape(-1, 1) if sig.dim() else sig ** 2
    prior = s2 - (W ** 2).sum(-1)
    cov = prior.clamp(min=0.0) + ((W @ Lu) ** 2).sum(-1)
    mean = (W @ mu.unsqueeze(-1)).squeeze(-1)
    scale = cov ** 0.5
    loss = (mean * R1).sum() * (1.0 if use_mean else 0.0) + (scale * R2).sum() * (1.0 if use_scale else 0.0)
    gmu, gLu, gsig = torch.autograd.grad(loss, (mu, Lur, sig))
    return dict(mean=mean.detach(), scale=scale.detach(), Lu=Lu.detach(), prior=(prior / s2).detach(), loss=loss.detach(),
                grad_mu=gmu, grad_Lu=gLu, grad_sigma=gsig)


def chunk_columns(N: int, width: int) -> list:
    """Column ranges of the chunks the passes walk under a chunk width (pre_plan: nc = pad128(min(width, N)))."""
    nc = pad128(min(width, N))
    return [(n0, min(N, n0 + nc)) for n0 in range(0, N, nc)]


def pre_tol(ref: torch.Tensor, dtype, relative_only: bool = False) -> torch.Tensor:
    """Element-wise tolerance of the precomputed comparisons: helpers.rtol_for, atol = rtol max|ref| (0 for `scale`)."""
    rt = 1e-5 if dtype == torch.float64 else 1e-3
    return rt * ref.abs() + (0.0 if relative_only else rt * float(ref.abs().max()))


# the last chunk of these cases is ONE column: its upstreams are boosted so that dropping it is seen (test_entry_cases.py)
BOOST_ONE_COLUMN = 64.0


def chunk_cases() -> list:
    """(N, M, width, case) of the chunking tests: two exact chunks, a ragged third, a last chunk of one column."""
    out = []
    for N in CHUNK_N:
        for M in CHUNK_M:
            for w in CHUNK_WIDTHS:
                one = chunk_columns(N, w)[-1][1] - chunk_columns(N, w)[-1][0] == 1
                out.append((N, M, w, precomputed_case(2, N, M, boost_last=BOOST_ONE_COLUMN if one else 1.0)))
    return out
