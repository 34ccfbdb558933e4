"""GPU: the fused sparse Gaussian factor step (gpz_gaussian_fa_sparse, ops.gaussian_fa_sparse) against fp64 CPU autograd of
the dense closed form on ``z[:, idx] - offset`` -- every case of tests/sparse_gaussian_cases.py with
``gaussian_cases.check`` unchanged (value rel 5e-5 / abs 1e-3, gradients 1e-3 of their own row / column magnitude, sse rtol
1e-5) and ss to rtol 1e-9 -- bitwise reproducibility, poisoned scratch memory and outputs, the value-only form, misaligned
views, the batch forms and the dense entry on ``to_dense()``."""
import ctypes as C

import pytest
import torch

import gaussian_cases as GC
import sparse_gaussian_cases as S

pytestmark = pytest.mark.gpu

OUTS = ("loglik", "sse", "ss", "dmean", "dscale", "dW", "db", "dsd")
BITWISE = ("Lt5", "chunks", "batch_B137", "Lt64")


def same_bits(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert set(a[3]) == set(b[3])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def check_ss(ss, c, tag):
    want = S.null_ss(c)
    err = (ss.double().cpu() - want).abs()
    print(tag, "ss_per_gene: max relative error", float((err / want.clamp_min(1e-300)).max()))
    assert bool((err <= 1e-9 * want).all()), f"ss_per_gene {tag}"


@pytest.mark.parametrize("name", S.case_names())
def test_sparse_gaussian_cases(name):
    c, want = S.case(name), S.reference(name)
    ll, sse, ss, got = S.run(c)
    assert ll.dtype == sse.dtype == ss.dtype == torch.float64 and all(g.dtype == torch.float32 for g in got.values())
    GC.check(ll, sse, got, want, name)
    check_ss(ss, c, name)


@pytest.mark.parametrize("name", BITWISE)
def test_two_calls_agree_bit_for_bit(name):
    c = S.case(name)
    same_bits(S.run(c), S.run(c))


def raw_call(c, partials, poison, grads=True):
    """gpz_gaussian_fa_sparse through ctypes with the caller's ``partials``; with ``poison`` every output and all of
    ``partials`` are filled with 0xFF bytes (NaNs, -1 as an integer) first.  Returns the outputs by name."""
    from gpzoo_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = {k: c[k].cuda().contiguous() for k in ("mean", "scale", "W", "b", "sd")}
    e = S.expression(c, "cuda")
    view, base = e.values, e.values.base
    Lt, B = c["mean"].shape
    D, N = base.shape
    nnz = int(base.col_val.numel())
    need = ops.gaussian_fa_sparse_plan(N, B, D, Lt, nnz)["workspace_bytes"]
    assert partials.numel() >= need
    shapes = dict(loglik=((1,), torch.float64), sse=((D,), torch.float64), ss=((D,), torch.float64),
                  dmean=((Lt, B), torch.float32), dscale=((Lt, B), torch.float32), dW=((D, Lt), torch.float32),
                  db=((D,), torch.float32), dsd=((D,), torch.float32))
    out = {k: torch.zeros(s, dtype=dt, device=dev) for k, (s, dt) in shapes.items() if grads or k in OUTS[:3]}
    if poison:
        partials.fill_(255)
        for v in out.values():
            v.view(torch.uint8).fill_(255)
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    rc = lib.gpz_gaussian_fa_sparse(*(ptr(t[k]) for k in ("mean", "scale", "W", "b", "sd")), ptr(e.offset),
                                    *(ptr(getattr(base, k)) for k in base._PARTS), ptr(view.idx), ptr(view.pos),
                                    N, B, D, nnz, Lt, *(ptr(out.get(k)) for k in OUTS), ptr(partials), partials.numel(),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "gpz_gaussian_fa_sparse")
    torch.cuda.synchronize()
    return out


def test_poisoned_scratch_and_outputs_change_nothing():
    """The same call after the scratch memory and every output were filled with 0xFF bytes gives identical bits: the small
    whole-data case, then the chunk case and a batch view of it on the same (larger) buffer, which then holds the earlier
    calls' sums and NaNs; the value-only form on poisoned memory as well."""
    from gpzoo_amd import ops
    names = ("Lt20", "chunks", "batch_B137", "empties")
    sizes = []
    for n in names:
        c = S.case(n)
        sizes.append(ops.gaussian_fa_sparse_plan(c["N"], c["B"], c["z"].shape[0], c["mean"].shape[0],
                                                 int((c["z"] != 0).sum()))["workspace_bytes"])
    assert sizes[1] > sizes[0]
    partials = torch.zeros(max(sizes) + 64, dtype=torch.uint8, device="cuda")
    for n in names:
        c, want = S.case(n), S.reference(n)
        clean = raw_call(c, torch.zeros_like(partials), poison=False)
        dirty = raw_call(c, partials, poison=True)
        for k in OUTS:
            assert bool(torch.isfinite(dirty[k]).all()), (n, k)
            assert torch.equal(clean[k], dirty[k]), (n, k)
        assert float(dirty["loglik"][0]) == pytest.approx(want.value, rel=5e-5, abs=1e-3)
        v = raw_call(c, partials, poison=True, grads=False)
        for k in OUTS[:3]:
            assert torch.equal(v[k], clean[k]), (n, k)


@pytest.mark.parametrize("name", BITWISE + ("batch_B1", "D1"))
def test_value_only_call_returns_the_same_bits(name):
    c, want = S.case(name), S.reference(name)
    full = S.run(c)
    out = S.run(c, grads=False)
    assert len(out[3]) == 0
    assert torch.equal(out[0], full[0]) and torch.equal(out[1], full[1]) and torch.equal(out[2], full[2])
    assert float(out[0]) == pytest.approx(want.value, rel=5e-5, abs=1e-3)


@pytest.mark.parametrize("name", ["Lt5", "Lt20", "batch_B137"])
def test_misaligned_views_give_the_aligned_bits(name):
    c = S.case(name)
    same_bits(S.run(c), S.run(c, shift=1))


@pytest.mark.parametrize("name", ["batch_B137", "batch_B1", "descending"])
def test_idx_argument_equals_the_view(name):
    from gpzoo_amd import ops
    c = S.case(name)
    whole = S.expression({k: v for k, v in c.items() if k != "idx"}, "cuda")
    p = [c[k].cuda() for k in ("mean", "scale", "W", "b", "sd")]
    idx = c["idx"].cuda()
    a = ops.gaussian_fa_sparse(*p, whole, idx=idx)
    b = ops.gaussian_fa_sparse(*p, whole[:, idx])
    i32 = ops.gaussian_fa_sparse(*p, whole, idx=idx.to(torch.int32))
    for x, y, z in zip(a, b, i32):
        assert torch.equal(x, y) and torch.equal(x, z)
    for form in (dict(idx=idx), {}):
        v = ops.gaussian_fa_sparse(*p, whole if form else whole[:, idx], grads=False, **form)
        assert len(v) == 3 and all(torch.equal(x, y) for x, y in zip(v, a[:3]))


@pytest.mark.parametrize("name", ["Lt20", "chunks"])
def test_identity_view_of_all_spots_gives_the_whole_data_bits(name):
    from gpzoo_amd import ops
    c = S.case(name)
    e = S.expression(c, "cuda")
    p = [c[k].cuda() for k in ("mean", "scale", "W", "b", "sd")]
    a = ops.gaussian_fa_sparse(*p, e)
    b = ops.gaussian_fa_sparse(*p, e[:, torch.arange(c["N"], device="cuda")])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["Lt20", "batch_B137", "center_false"])
def test_dense_entry_on_to_dense_agrees(name):
    """``ops.gaussian_fa`` on ``expr.to_dense()`` (the fp32 rounding of z - offset) against the same oracle and tolerances."""
    from gpzoo_amd import ops
    c, want = S.case(name), S.reference(name)
    e = S.expression(c, "cuda")
    p = [c[k].cuda() for k in ("mean", "scale", "W", "b", "sd")]
    out = ops.gaussian_fa(*p, e.to_dense())
    GC.check(out[0], out[1], dict(zip(S.GRADS, out[2:])), want, name + " dense")
    sp = ops.gaussian_fa_sparse(*p, e)
    assert float(sp[0]) == pytest.approx(float(out[0]), rel=1e-4, abs=2e-3)


def test_refusals_reach_python():
    from gpzoo_amd import ops
    c = S.case("Lt64")
    e = S.expression(c, "cuda")
    D, N = e.shape
    z = torch.zeros(65, N).cuda()
    with pytest.raises(ValueError, match="gpz_gaussian_fa_sparse: 65 factors unsupported"):
        ops.gaussian_fa_sparse(z, z + 1, torch.ones(D, 65).cuda(), torch.zeros(D).cuda(), torch.ones(D).cuda(), e)
    with pytest.raises(ValueError, match="do not fit together"):
        ops.gaussian_fa_sparse(z[:3], z[:3] + 1, torch.ones(D, 3).cuda(), torch.zeros(D + 1).cuda(), torch.ones(D).cuda(), e)
    with pytest.raises(ValueError, match="do not fit together"):
        ops.gaussian_fa_sparse(z[:3, :7], z[:3, :7] + 1, torch.ones(D, 3).cuda(), torch.zeros(D).cuda(), torch.ones(D).cuda(), e)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        ops.gaussian_fa_sparse(z[:3], z[:3] + 1, torch.ones(D, 3).cuda(), torch.zeros(D).cuda(), torch.ones(D).cuda(), e.cpu())
    with pytest.raises(TypeError, match="gaussian_fa_sparse"):
        ops.gaussian_fa(z[:3], z[:3] + 1, torch.ones(D, 3).cuda(), torch.zeros(D).cuda(), torch.ones(D).cuda(), e)
