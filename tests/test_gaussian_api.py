"""CPU: the surface of the Gaussian factor models -- the two C entries and their host-side refusals, ``ops.gaussian_fa``,
the parameters of ``RSF`` and ``FA``, and the one change to the training loops (real loadings are not clamped)."""
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("gpz_gaussian_fa", "gpz_gaussian_fa_plan")
D, N, L = 7, 11, 3


def header():
    return open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()


def data(seed=0):
    g = torch.Generator().manual_seed(seed)
    return 3.0 + torch.randn(D, N, generator=g) * torch.linspace(0.5, 2.0, D)[:, None]


def rsf(y, **kw):
    import gpzoo.gp as G
    import gpzoo.kernels as K
    import gpzoo.likelihoods as li
    return li.RSF(G.WSVGP(K.NSF_RBF(L=L), dim=2, M=6), y, L=L, **kw)


def fa(y, **kw):
    import gpzoo.gp as G
    import gpzoo.likelihoods as li
    return li.FA(G.GaussianPrior(y, L=L), y, L=L, **kw)


def test_new_entries_are_declared_exported_and_bound():
    from gpzoo_amd import _lib, ops
    hdr = header()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    assert lib.gpz_version() == 212
    assert callable(ops.gaussian_fa) and callable(ops.gaussian_fa_plan)
    import gpzoo.likelihoods as li
    assert callable(li.gaussian_expected_loglik) and issubclass(li._GaussianFALogLik, torch.autograd.Function)
    assert issubclass(li.RSF, torch.nn.Module) and issubclass(li.FA, torch.nn.Module)
    assert li.GaussianScore._fields == ("loglik", "sse_per_gene", "mse_per_gene", "mse", "r2_per_gene", "r2")
    assert "gaussian.hip" in __import__("gpzoo_amd.build", fromlist=["SOURCES"]).SOURCES


def test_scratch_is_an_explicit_argument_named_partials():
    hdr = header()
    args = re.search(r"\bgpz_gaussian_fa\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in args.replace("\n", " ").split(",")]
    assert "ws" not in names and "partials" in names and "partials_bytes" in names
    assert "gpz_gaussian_fa_workspace_bytes" not in hdr
    import scratch_cases as S
    assert not {"gpz_gaussian_fa", "gpz_gaussian_fa_plan"} & S.header_entries_with_workspace(hdr)


def test_plan_query_answers_and_refuses_on_the_host():
    from gpzoo_amd import _lib, ops
    lib = _lib.load()
    p = ops.gaussian_fa_plan(100, 10, 20)
    assert p == dict(factors_padded=20, aligned_rows=True, gene_slices=1, spot_slices=1, partials_bytes=p["partials_bytes"])
    assert p["partials_bytes"] > 0
    assert lib.gpz_gaussian_fa_plan(100, 10, 65, None, None, None, None, None) < 0
    assert b"gpz_gaussian_fa: 65 factors unsupported" in lib.gpz_last_error()
    assert lib.gpz_gaussian_fa_plan(0, 10, 20, None, None, None, None, None) < 0
    assert b"gpz_gaussian_fa: bad extents" in lib.gpz_last_error()
    assert lib.gpz_gaussian_fa_plan(100, 1 << 31, 20, None, None, None, None, None) < 0
    assert b"gpz_gaussian_fa" in lib.gpz_last_error()
    with pytest.raises(ValueError, match="65 factors unsupported"):
        ops.gaussian_fa_plan(100, 10, 65)
    # nothing of D x N elements: at the Slide-seq mini-batch the partial sums take less than half the bytes of y
    big = ops.gaussian_fa_plan(7000, 17702, 20)
    assert big["gene_slices"] >= 2 and big["spot_slices"] >= 2
    assert big["partials_bytes"] < 0.5 * 4 * 7000 * 17702


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C
    from gpzoo_amd import _lib
    lib = _lib.load()
    rc = lib.gpz_gaussian_fa(None, None, None, None, None, None, 10, 4, 3, None, None, None, None, None, None, None, None, 0, None)
    assert rc < 0 and b"gpz_gaussian_fa: null pointer" in lib.gpz_last_error()
    # host memory stands in for device memory: every refusal below comes before the first launch
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    ok = [p(256 * i) for i in range(6)]
    rc = lib.gpz_gaussian_fa(*ok, 10, 4, 3, None, None, None, None, None, None, None, p(3072), 1 << 20, None)
    assert rc < 0 and b"null pointer" in lib.gpz_last_error()                   # loglik
    rc = lib.gpz_gaussian_fa(*ok, 10, 4, 3, p(2048), None, p(2304), None, None, None, None, p(3072), 1 << 20, None)
    assert rc < 0 and b"all null or all set" in lib.gpz_last_error()
    rc = lib.gpz_gaussian_fa(p(4), *ok[1:], 10, 4, 3, p(2048), None, None, None, None, None, None, p(3072), 1 << 20, None)
    assert rc < 0 and b"16-byte aligned" in lib.gpz_last_error()
    rc = lib.gpz_gaussian_fa(*ok, 10, 4, 65, p(2048), None, None, None, None, None, None, p(3072), 1 << 20, None)
    assert rc < 0 and b"65 factors unsupported" in lib.gpz_last_error()
    rc = lib.gpz_gaussian_fa(*ok, 0, 4, 3, p(2048), None, None, None, None, None, None, p(3072), 1 << 20, None)
    assert rc < 0 and b"bad extents" in lib.gpz_last_error()
    rc = lib.gpz_gaussian_fa(*ok, 10, 4, 3, p(2048), None, None, None, None, None, None, p(3072), 16, None)
    assert rc < 0 and b"partials too small" in lib.gpz_last_error()


@pytest.mark.parametrize("make", [rsf, fa])
def test_parameters_of_the_models(make):
    y = data()
    m = make(y)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    own = {k: v for k, v in sd.items() if "." not in k}
    assert own == {"W": (D, L), "b": (D,), "noise": (D,)}
    prefix = "gp." if make is rsf else "prior."
    assert {k for k in sd if "." in k} and all(k.startswith(prefix) for k in sd if "." in k)
    assert all(isinstance(getattr(m, k), torch.nn.Parameter) and getattr(m, k).requires_grad for k in own)
    assert m.signed_loadings is True and bool((m.W < 0).any())
    torch.testing.assert_close(m.b.detach(), y.mean(1))
    torch.testing.assert_close(torch.nn.functional.softplus(m.noise.detach()), y.std(1, unbiased=False), rtol=1e-4, atol=1e-5)
    flat = torch.cat([y[:1] * 0 + 2.0, y[1:]])                      # a constant gene: the floor of 1e-3
    assert float(torch.nn.functional.softplus(make(flat).noise.detach())[0]) == pytest.approx(1e-3, rel=2e-2)
    h = make(y, noise0=0.25)
    torch.testing.assert_close(torch.nn.functional.softplus(h.noise.detach()), torch.full((D,), 0.25), rtol=1e-4, atol=0)
    with pytest.raises(ValueError, match="noise0 must be positive"):
        make(y, noise0=0.0)


def test_forward_builds_a_normal_over_samples_genes_and_spots():
    from torch import distributions
    y = data()
    m = fa(y, noise0=0.5)
    pY, qF, pF = m(E=4)
    assert isinstance(pY, distributions.Normal) and pY.loc.shape == (4, D, N)
    assert pY.scale.shape == (4, D, N) and pY.log_prob(y).shape == (4, D, N)      # torch broadcasts the (D, 1) scale
    torch.testing.assert_close(pY.scale[2, :, 3], torch.nn.functional.softplus(m.noise))
    assert qF.mean.shape == (L, N) and pF.mean.shape == (L, N)
    pYb, qFb, _ = m.forward_batched(torch.tensor([1, 5, 6]), E=2)
    assert pYb.loc.shape == (2, D, 3) and qFb.mean.shape == (L, 3)
    r = rsf(y)
    qF = distributions.Normal(torch.zeros(L, N), torch.ones(L, N))
    pYr = r._pY(qF, 5)                                               # the CPU piece of RSF.forward: the GP itself needs a GPU
    assert isinstance(pYr, distributions.Normal) and pYr.loc.shape == (5, D, N)


def test_unknown_keywords_are_refused_and_the_noise_level_stays_in_range():
    import gpzoo.likelihoods as li
    y = data()
    m = fa(y)
    m(X=torch.zeros(N, 2), E=2)                                      # what the training loops pass
    with pytest.raises(TypeError, match="unexpected keyword.*lenghtscale"):
        m(E=2, lenghtscale=3.0)
    with pytest.raises(TypeError, match="unexpected keyword"):
        m.expected_loglik(None, y, groupsX=torch.zeros(N))
    r = rsf(y)
    with pytest.raises(TypeError, match="unexpected keyword.*verbos"):
        r.expected_loglik(torch.zeros(N, 2), y, verbos=True)         # refused before the GP is called
    lo, hi = li.NOISE_SD_RANGE
    sd = li._noise_sd(torch.tensor([-200.0, 0.0, 1e30]))
    assert float(sd[0]) == pytest.approx(lo) and float(sd[2]) == pytest.approx(hi) and float(sd[1]) == pytest.approx(0.6931472)
    assert bool(torch.isfinite(1.0 / (sd * sd)).all())               # what the spot pass forms, in fp32
    hdr = header()
    assert "1e-18 <= noise_sd[d] <= 1e18" in hdr


def test_real_loadings_are_not_clamped():
    from gpzoo_amd.utilities import _clamp_loadings
    import gpzoo.gp as G
    import gpzoo.kernels as K
    import gpzoo.likelihoods as li
    y = data()
    for m in (rsf(y), fa(y)):
        before = m.W.detach().clone()
        assert bool((before < 0).any())
        _clamp_loadings(m, ("W",))
        _clamp_loadings(m)
        assert torch.equal(m.W.detach(), before)
    nsf = li.NSF(G.WSVGP(K.NSF_RBF(L=L), dim=2, M=6), torch.ones(D, N), L=L)
    with torch.no_grad():
        nsf.W.copy_(torch.linspace(-1.0, 1.0, D * L).reshape(D, L))
    _clamp_loadings(nsf, ("W",))
    assert float(nsf.W.min()) == 0.0 and float(nsf.W.max()) == 1.0


def test_sparse_counts_are_refused():
    from gpzoo_amd import ops
    from gpzoo_amd.likelihoods import SparseCounts
    y = SparseCounts(torch.eye(D, N))
    z = torch.zeros(L, N)
    with pytest.raises(TypeError, match="dense real-valued data"):
        ops.gaussian_fa(z, z + 1, torch.ones(D, L), torch.zeros(D), torch.ones(D), y)


def test_cpu_tensors_fail_loudly():
    from gpzoo_amd import ops
    z = torch.zeros(L, N)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gaussian_fa(z, z + 1, torch.ones(D, L), torch.zeros(D), torch.ones(D), torch.zeros(D, N))
