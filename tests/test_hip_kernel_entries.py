"""GPU: gpz_kfill and gpz_kgrad as the module API calls them on their own, beyond their first tile -- every kind, input
dimension and precision, the column blocks, store variants, tails, latent splits and the C ABI's padded windows of the fill;
every unroll slot, trip and tail of the gradient contraction and both sides of its finishing launch -- against the fp64
oracles (oracle/svgp_oracle.py, tests/matern_oracle.py) and torch autograd through them.  The cases, the restated launch
arithmetic and the reasons the lists are worth running are in tests/entry_cases.py / tests/test_entry_cases.py.

Tolerances are the project's own: kernel values as tests/test_hip_matern_family.py (fp64 1e-9, fp32 1e-4, fp32 inputs written
in fp64 1e-5 / 1e-6), gradients tests/test_hip_kernel_grads.py::_close."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import entry_cases as E
from test_hip_kernel_grads import _close

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
PRECISIONS = {"f32-f32": (F32, F32), "f32-f64": (F32, F64), "f64-f64": (F64, F64)}


def _spec(c, dtype):
    from gpzoo_amd.ops import KernelSpec
    ga = r2 = None
    if c["kind"] == "mggp":
        emb = c["emb"].to(dtype).cuda()
        r2 = ((emb[:, None, :] - emb[None, :, :]) ** 2).sum(-1)
        ga = c["a"].to(dtype).cuda()
    return KernelSpec(E.KIND_ID[c["kind"]], c["sigma"].to(dtype).cuda(), c["ell"].to(dtype).cuda(), True, ga, r2, c["d"] / 2)


def _groups(c):
    return dict(gA=c["gA"].cuda(), gB=c["gB"].cuda()) if c["kind"] == "mggp" else {}


def _fill(c, in_dt, out_dt, jitter=0.0):
    from gpzoo_amd import ops
    return ops.kfill(_spec(c, in_dt), c["A"].to(in_dt).cuda(), c["B"].to(in_dt).cuda(), jitter=jitter, out_dtype=out_dt, **_groups(c))


def _check_values(K, ref, in_dt, out_dt, what):
    assert K.dtype == out_dt and K.shape == ref.shape, what
    if in_dt == F64:
        tol = dict(rtol=1e-9, atol=1e-9)
    elif out_dt == F32:
        tol = dict(rtol=1e-4, atol=1e-4)
    else:
        tol = dict(rtol=E.VALUE_TOL_MIXED[0], atol=E.VALUE_TOL_MIXED[1])
    torch.testing.assert_close(K.double().cpu(), ref, msg=lambda m: f"{what}: {m}", **tol)


# ---- gpz_kfill ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", E.KINDS)
def test_fill_every_kind_dimension_and_precision(kind, d, prec):
    """(9, 261): three row blocks; two column blocks in fp32 and three in fp64, the last one ragged (scalar stores).  MGGP
    with 5 groups, every group on both sides, group_pow = d / 2."""
    in_dt, out_dt = PRECISIONS[prec]
    c = E.kernel_case(kind, d, *E.MAIN_FILL)
    _check_values(_fill(c, in_dt, out_dt), E.kernel_value(c), in_dt, out_dt, f"{kind} d={d} {prec}")


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("kind", ["rbf", "mggp"])
def test_fill_column_sweep(kind, prec):
    """Columns next to the vector width and the 256 (fp32) / 128 (fp64) columns of a workgroup, rows next to the 4 of one:
    both store variants with one and several column blocks, every tail length."""
    in_dt, out_dt = PRECISIONS[prec]
    for nA in E.SWEEP_NA:
        for nB in (E.SWEEP_NB_F32 if out_dt == F32 else E.SWEEP_NB_F64):
            c = E.kernel_case(kind, 2, nA, nB, seed=nA)
            _check_values(_fill(c, in_dt, out_dt), E.kernel_value(c), in_dt, out_dt, f"{kind} {nA}x{nB} {prec}")


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("kind", E.KINDS)
def test_fill_diagonal_with_jitter_is_exact(kind, prec):
    """K(Z, Z, jitter): the diagonal is sigma^2 + jitter bit for bit (exp(0) = 1; den = 1 between equal groups), the rest
    the oracle's."""
    in_dt, out_dt = PRECISIONS[prec]
    jitter = 0.0123
    c = E.kernel_case(kind, 2, 133, 133, same=True)
    K = _fill(c, in_dt, out_dt, jitter=jitter).cpu()
    s = c["sigma"].to(in_dt).to(out_dt)
    want = s * s + torch.tensor(jitter, dtype=out_dt) if kind != "distance" else torch.full((1,), jitter, dtype=out_dt)
    diag = torch.diagonal(K, dim1=-2, dim2=-1)
    assert torch.equal(diag, want[:, None].expand_as(diag)), f"{kind} {prec}"
    ref = E.kernel_value(c) + jitter * torch.eye(133, dtype=F64)
    _check_values(K, ref, in_dt, out_dt, f"{kind} {prec}")


@pytest.mark.parametrize("kind,L,G", E.FILL_SPLITS)
def test_fill_latent_splits(kind, L, G):
    """More latents than one launch holds (256; MGGP: 2048 / G^2 table entries): the later launches take their own slice of
    every per-latent parameter and of K.  All parameters are distinct per latent."""
    c = E.kernel_case(kind, 2, *E.SPLIT_SHAPE, L=L, G=max(G, 1))
    for in_dt, out_dt in ((F32, F32), (F64, F64)):
        _check_values(_fill(c, in_dt, out_dt), E.kernel_value(c), in_dt, out_dt, f"{kind} L={L} G={G}")


def _raw_fill(c, dtype, K, ldk, stride):
    """gpz_kfill through ctypes on the current stream; returns rc."""
    from gpzoo_amd import _lib, ops
    lib = _lib.load()
    keep = []
    d = ops._desc(_spec(c, dtype), dtype, keep)
    A, B = c["A"].to(dtype).cuda(), c["B"].to(dtype).cuda()
    g = _groups(c)
    rc = lib.gpz_kfill(C.byref(d), ops._ptr(A), c["nA"], ops._ptr(B), c["nB"], c["d"], ops._ptr(g.get("gA")), ops._ptr(g.get("gB")),
                       C.c_void_p(K.data_ptr()), ldk, stride, 0.0, ops._dt(K), ops._stream(A.device))
    torch.cuda.synchronize()
    return rc


def test_fill_refuses_more_than_45_groups_before_any_launch():
    from gpzoo_amd import _lib
    c = E.kernel_case("mggp", 2, *E.SPLIT_SHAPE, L=3, G=46)
    K = torch.full((3, 5, 9), -777.25, dtype=F32, device="cuda")
    rc = _raw_fill(c, F32, K, 9, 45)
    assert rc != 0 and b"n_groups=46 unsupported (max 45)" in _lib.load().gpz_last_error()
    assert bool((K == -777.25).all())
    from gpzoo_amd import ops
    with pytest.raises(RuntimeError, match="n_groups=46 unsupported"):
        ops.kfill(_spec(c, F32), c["A"].float().cuda(), c["B"].float().cuda(), **_groups(c))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_fill_c_abi_padded_window(dtype):
    """The C ABI's own arguments: a padded leading dimension, a latent stride beyond nA ldk and a base one element off a
    16-byte boundary -- the output window inside a sentinel-filled buffer is correct and nothing outside it is written."""
    sentinel = -777.25
    for nB in E.ABI_NB:
        c = E.kernel_case("rbf", 2, E.ABI_NA, nB, L=2, seed=nB)
        ref = E.kernel_value(c)
        for lp in E.ABI_LDK_PAD:
            for sp in E.ABI_STRIDE_PAD:
                for off in E.ABI_BASE:
                    ldk = nB + lp
                    stride = E.ABI_NA * ldk + sp
                    buf = torch.full((off + 2 * stride + 64,), sentinel, dtype=dtype, device="cuda")
                    assert buf.data_ptr() % 16 == 0
                    rc = _raw_fill(c, dtype, buf[off:], ldk, stride)
                    what = f"nB={nB} ldk={ldk} stride={stride} off={off}"
                    assert rc == 0, what
                    host = buf.cpu()
                    inside = torch.zeros(host.numel(), dtype=torch.bool)
                    win = torch.empty(2, E.ABI_NA, nB, dtype=dtype)
                    for l in range(2):
                        for i in range(E.ABI_NA):
                            a = off + l * stride + i * ldk
                            inside[a:a + nB] = True
                            win[l, i] = host[a:a + nB]
                    _check_values(win, ref, dtype, dtype, what)
                    assert bool((host[~inside] == sentinel).all()), what


def test_fill_more_than_65536_row_blocks():
    """kernel(X, Z) puts the N points on grid.y, four rows per block: 4 * 65536 + 1 rows, last row included."""
    c = E.kernel_case("rbf", 2, *E.TALL, L=1)
    K = _fill(c, F32, F32)
    _check_values(K, E.kernel_value(c), F32, F32, "tall")


# ---- gpz_kgrad ------------------------------------------------------------------------------------------------------

def _kgrad(c, dtype, Kbar, want_points=True):
    from gpzoo_amd import ops
    return ops.kgrad(_spec(c, dtype), c["A"].to(dtype).cuda(), c["B"].to(dtype).cuda(), Kbar.to(dtype).cuda(),
                     want_points=want_points, **_groups(c))


def _check_grads(c, dtype, what, ups=None):
    for un, up in (ups or E.upstreams(c)).items():
        ref = E.kernel_grads(c, up)
        gth, gA = _kgrad(c, dtype, up)
        assert gth.shape == (c["L"], 3) and gA.shape == (c["nA"], c["d"]) and gth.dtype == F64
        _close(gth, ref["theta"], dtype, f"{what} {un}: grad_theta")
        _close(gA, ref["A"], dtype, f"{what} {un}: grad_A")


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", E.GRAD_KINDS)
def test_grad_every_kind_dimension_and_precision(kind, d, dtype):
    """(5, 257): two row blocks, a second trip of one column; a dense and a probe upstream (non-zero only next to the
    64-column boundaries).  grad_theta = d/d(sigma, lengthscale, a), grad_A."""
    _check_grads(E.kernel_case(kind, d, *E.MAIN_GRAD), dtype, f"{kind} d={d}")


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("kind", E.GRAD_SWEEP_KINDS)
def test_grad_column_sweep(kind, dtype):
    """Every unroll slot as the last one of a trip, one to five trips, tails of one lane, 63 lanes and a full slot."""
    for nA in E.SWEEP_NA:
        for nB in E.GRAD_SWEEP_NB:
            _check_grads(E.kernel_case(kind, 2, nA, nB, seed=nA), dtype, f"{kind} {nA}x{nB}")


@pytest.mark.parametrize("nA,nB,L", E.FINISH_CASES)
def test_grad_finish_from_both_sides(nA, nB, L):
    """kgrad_finish sizes its grid by max(ceil(nA / 256), L): more row blocks than latents, and more latents than row blocks."""
    c = E.kernel_case("rbf", 2, nA, nB, L=L)
    for dtype in (F64, F32):
        _check_grads(c, dtype, f"finish {nA}x{nB} L={L}")


CLASSES = ("RBF", "NSF_RBF", "batched_RBF", "batched_Matern12", "batched_Matern32", "batched_Matern52", "MGGP_RBF",
           "MGGP_NSF_RBF", "batched_MGGP_RBF")
ORACLE_KIND = {"RBF": "rbf", "NSF_RBF": "nsf_rbf", "batched_RBF": "batched_rbf", "batched_Matern12": "matern12",
               "batched_Matern32": "matern32", "batched_Matern52": "matern52", "MGGP_RBF": "mggp_rbf",
               "MGGP_NSF_RBF": "mggp_nsf_rbf", "batched_MGGP_RBF": "batched_mggp_rbf"}


def _module(cls, d, dtype):
    """(module on the GPU, its parameters as fp64 CPU leaves in their own shapes, embedding)."""
    import gpzoo.kernels as K
    L = 3
    sig, ell, a = E.per_latent(E.SIG, L), E.per_latent(E.ELL, L), E.per_latent(E.GA, L)
    p = {}
    if cls in ("RBF", "MGGP_RBF"):
        p = dict(sigma=torch.tensor(1.2), lengthscale=torch.tensor(3.0))
    elif cls in ("NSF_RBF", "MGGP_NSF_RBF"):
        p = dict(sigma=sig.reshape(L, 1, 1), lengthscale=ell.reshape(L, 1, 1))
    elif cls == "batched_MGGP_RBF":
        p = dict(sigma=torch.tensor(1.1), lengthscale=torch.tensor(3.5))
    else:
        p = dict(sigma=sig, lengthscale=ell)
    mggp = "MGGP" in cls
    if cls == "MGGP_RBF":
        p["group_diff_param"] = torch.tensor(0.6)
    elif cls == "MGGP_NSF_RBF":
        p["group_diff_param"] = a.reshape(L, 1, 1)
    elif cls == "batched_MGGP_RBF":
        p["group_diff_param"] = torch.tensor(-0.6)          # |a|: the chain is sign(a)
    p = {n: E.r32(v.double()) for n, v in p.items()}
    k = getattr(K, cls)(n_groups=3, **({"L": L} if cls == "MGGP_NSF_RBF" else {})) if mggp else \
        (K.NSF_RBF(L=L) if cls == "NSF_RBF" else getattr(K, cls)())
    for n, v in p.items():
        setattr(k, n, nn.Parameter(v.clone()))
    k = k.to(dtype).cuda()
    emb = None
    if mggp:
        emb = E.r32(torch.randn(3, 2, generator=torch.Generator().manual_seed(5), dtype=F64) * 0.8)
        e = emb.to(dtype).cuda()
        k.embedding = nn.Parameter(e, requires_grad=False) if isinstance(k.embedding, nn.Parameter) else e
        k.input_dim = d
    return k, p, emb


def _module_ref(cls, d, p, X, Z, emb, gX, gZ, R):
    """fp64 oracle value and autograd gradients by leaf name; Z None: X in both slots (one leaf, the roles' gradients add)."""
    import matern_oracle as MO
    from oracle import svgp_oracle as O
    leaves = {n: v.clone().requires_grad_(True) for n, v in dict(p, X=X, **({} if Z is None else {"Z": Z})).items()}
    A, B = leaves["X"], leaves["X"] if Z is None else leaves["Z"]
    kind = ORACLE_KIND[cls]
    if "matern" in kind:
        K = MO.kernel_matrix(kind, A, B, leaves["sigma"], leaves["lengthscale"])
    elif emb is None:
        K = O.kernel_matrix(kind, A, B, leaves["sigma"], leaves["lengthscale"])
    else:
        K = O.kernel_matrix(kind, A, B, leaves["sigma"], leaves["lengthscale"], gA=gX, gB=gZ, embedding=emb,
                            group_diff=leaves["group_diff_param"], input_dim=d)
    (K * (R if K.dim() == 3 else R[0])).sum().backward()
    return K.detach(), {n: t.grad for n, t in leaves.items()}


def _module_case(cls, d, dtype, same):
    N, M = 257, 5
    g = torch.Generator().manual_seed(300 + d)
    X = E.r32((torch.rand(N, d, generator=g, dtype=F64) - 0.5) * 8)
    Z = None if same else E.r32((torch.rand(M, d, generator=g, dtype=F64) - 0.5) * 8)
    gX = torch.arange(N) % 3
    gZ = gX if same else torch.arange(M) % 3
    R = E.r32(torch.randn(3, N, N if same else M, generator=g, dtype=F64))
    k, p, emb = _module(cls, d, dtype)
    Kr, ref = _module_ref(cls, d, p, X, Z, emb, gX, gZ, R)
    Xg = X.to(dtype).cuda().requires_grad_(True)
    Zg = Xg if same else Z.to(dtype).cuda().requires_grad_(True)
    args = (gX.cuda(), gZ.cuda()) if emb is not None else ()
    Kg = k(Xg, Zg, *args)
    assert Kg.shape == Kr.shape
    _check_values(Kg.detach(), Kr, dtype, dtype, f"{cls} d={d} K")
    Rg = R.to(dtype).cuda()
    (Kg * (Rg if Kg.dim() == 3 else Rg[0])).sum().backward()
    got = {"X": Xg.grad, **{n: getattr(k, n).grad for n in p}}
    if not same:
        got["Z"] = Zg.grad
    for n, v in got.items():
        assert v is not None and v.shape == ref[n].shape, n
        _close(v, ref[n], dtype, f"{cls} d={d} same={same}: grad_{n}")


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("cls", CLASSES)
def test_module_gradients_to_points_and_parameters(cls, dtype):
    """k(X, Z) at N = 257, M = 5 with gradients to X, Z and every parameter (both roles of gpz_kgrad and the transposed
    call), and k(X, X) with one tensor in both slots."""
    _module_case(cls, 2, dtype, same=False)
    _module_case(cls, 2, dtype, same=True)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("cls", ["MGGP_RBF", "MGGP_NSF_RBF", "batched_MGGP_RBF"])
def test_mggp_modules_in_other_input_dimensions(cls, d):
    """group_pow = d / 2 in value and gradient, and the chain from the effective multiplier to group_diff_param (a, a^2, |a|)."""
    for dtype in (F64, F32):
        _module_case(cls, d, dtype, same=False)


@pytest.mark.parametrize("kind", E.GRAD_KINDS)
def test_grad_at_coincident_points(kind):
    """A holds exact copies of three of B's five points among its 257 (and the other way round): the gradients are finite and
    the oracle's (masked square root: zero from a coincident pair); an upstream on the coincident pairs alone gives exactly
    zero point gradients -- Matern-1/2's kink included -- and the oracle's parameter gradients."""
    c = E.kernel_case(kind, 2, 257, 5)
    rows = (0, 130, 256)
    for r, j in zip(rows, (4, 0, 2)):
        c["A"][r] = c["B"][j]
    t = dict(c, A=c["B"], B=c["A"], nA=5, nB=257)
    if kind == "mggp":
        t["gA"], t["gB"] = c["gB"], c["gA"]
    for case, pairs in ((c, [(r, j) for r, j in zip(rows, (4, 0, 2))]), (t, [(j, r) for r, j in zip(rows, (4, 0, 2))])):
        ups = E.upstreams(case)
        only = torch.zeros_like(ups["dense"])
        for i, j in pairs:
            only[:, i, j] = ups["dense"][:, i, j]
        for dtype in (F64, F32):
            _check_grads(case, dtype, f"{kind} coincident", ups=dict(dense=ups["dense"]))
            gth, gA = _kgrad(case, dtype, only)
            assert torch.isfinite(gth).all() and bool((gA == 0).all()), f"{kind}: point gradient from coincident pairs"
            _close(gth, E.kernel_grads(case, only)["theta"], dtype, f"{kind} coincident pairs: grad_theta")


def test_two_runs_give_equal_bits():
    for kind in ("rbf", "mggp"):
        c = E.kernel_case(kind, 3, 5, 1025)
        up = E.upstreams(c)["dense"]
        for dtype in (F64, F32):
            a = [t.clone() for t in _kgrad(c, dtype, up)]
            b = _kgrad(c, dtype, up)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            assert torch.equal(_fill(c, dtype, dtype), _fill(c, dtype, dtype))
