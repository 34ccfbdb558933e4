"""GPU: the fused Gaussian factor step (gpz_gaussian_fa, ops.gaussian_fa) against fp64 CPU autograd of the closed form --
every kernel instance, tile edge, alignment path and slice count (tests/gaussian_cases.py) -- bitwise reproducibility,
stale scratch memory and outputs, the value-only form and misaligned views.  Tolerances are nb_cases.check's."""
import ctypes as C

import pytest
import torch

import gaussian_cases as GC

pytestmark = pytest.mark.gpu

ONE_SLICE, MULTI_SLICE = 9, 28          # rows of GC.SWEEP: (130, 500, 20) and (600, 600, 20)
OUTS = ("loglik", "sse", "dmean", "dscale", "dW", "db", "dsd")


@pytest.mark.parametrize("i", range(len(GC.SWEEP)))
def test_gaussian_sweep(i):
    D, N, Lt, why = GC.SWEEP[i]
    c, want = GC.case(i)
    ll, sse, got = GC.run(c)
    GC.check(ll, sse, got, want, dict(D=D, N=N, Lt=Lt, why=why))


def test_two_calls_agree_bit_for_bit():
    c, _ = GC.case(MULTI_SLICE)
    a, b = GC.run(c), GC.run(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def raw_call(c, partials, poison, grads=True):
    """gpz_gaussian_fa through ctypes with the caller's ``partials``; with ``poison`` every output and all of
    ``partials`` are filled with 0xFF bytes (NaNs) first.  Returns the outputs by name."""
    from gpzoo_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = {k: c[k].cuda().contiguous() for k in ("mean", "scale", "W", "b", "sd", "y")}
    Lt, N = c["mean"].shape
    D = c["y"].shape[0]
    need = ops.gaussian_fa_plan(N, D, Lt)["partials_bytes"]
    assert partials.numel() >= need
    shapes = dict(loglik=((1,), torch.float64), sse=((D,), torch.float64), dmean=((Lt, N), torch.float32),
                  dscale=((Lt, N), torch.float32), dW=((D, Lt), torch.float32), db=((D,), torch.float32),
                  dsd=((D,), torch.float32))
    out = {k: torch.zeros(s, dtype=dt, device=dev) for k, (s, dt) in shapes.items() if grads or k in ("loglik", "sse")}
    if poison:
        partials.fill_(255)
        for v in out.values():
            v.view(torch.uint8).fill_(255)
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    rc = lib.gpz_gaussian_fa(*(ptr(t[k]) for k in ("mean", "scale", "W", "b", "sd", "y")), N, D, Lt,
                             *(ptr(out.get(k)) for k in OUTS), ptr(partials), partials.numel(),
                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "gpz_gaussian_fa")
    torch.cuda.synchronize()
    return out


def test_stale_partials_and_outputs_change_nothing():
    """The same call after ``partials`` and every output were filled with 0xFF bytes gives identical bits: a one-slice
    shape, then a multi-slice shape on the same (larger) buffer, which then holds the first call's sums and NaNs."""
    from gpzoo_amd import ops
    cases = [GC.case(ONE_SLICE)[0], GC.case(MULTI_SLICE)[0]]
    plans = [ops.gaussian_fa_plan(c["y"].shape[1], c["y"].shape[0], c["mean"].shape[0]) for c in cases]
    assert plans[0]["gene_slices"] == plans[0]["spot_slices"] == 1
    assert plans[1]["gene_slices"] >= 2 and plans[1]["spot_slices"] >= 2
    assert plans[1]["partials_bytes"] > plans[0]["partials_bytes"]
    partials = torch.zeros(plans[1]["partials_bytes"] + 64, dtype=torch.uint8, device="cuda")
    for c, want in zip(cases, (GC.case(ONE_SLICE)[1], GC.case(MULTI_SLICE)[1])):
        clean = raw_call(c, torch.zeros_like(partials), poison=False)
        dirty = raw_call(c, partials, poison=True)
        for k in OUTS:
            assert bool(torch.isfinite(dirty[k]).all()), k
            assert torch.equal(clean[k], dirty[k]), k
        assert float(dirty["loglik"][0]) == pytest.approx(want.value, rel=5e-5, abs=1e-3)
        # value-only on poisoned memory as well
        v = raw_call(c, partials, poison=True, grads=False)
        assert torch.equal(v["loglik"], clean["loglik"]) and torch.equal(v["sse"], clean["sse"])


@pytest.mark.parametrize("i", [1, ONE_SLICE, 27, MULTI_SLICE, 29])
def test_value_only_call_returns_the_same_bits(i):
    c, want = GC.case(i)
    ll, sse, _ = GC.run(c)
    out = GC.run(c, grads=False)
    assert len(out[2]) == 0
    assert torch.equal(out[0], ll) and torch.equal(out[1], sse)
    assert float(out[0]) == pytest.approx(want.value, rel=5e-5, abs=1e-3)


@pytest.mark.parametrize("i", [3, ONE_SLICE, 29])
def test_misaligned_views_give_the_aligned_bits(i):
    c, _ = GC.case(i)
    a = GC.run(c)
    b = GC.run(c, shift=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_refusals_reach_python():
    from gpzoo_amd import ops
    Lt, N, D = 65, 10, 4
    z = torch.zeros(Lt, N).cuda()
    with pytest.raises((RuntimeError, ValueError), match="65 factors unsupported"):
        ops.gaussian_fa(z, z + 1, torch.ones(D, Lt).cuda(), torch.zeros(D).cuda(), torch.ones(D).cuda(), torch.ones(D, N).cuda())
    with pytest.raises(ValueError, match="do not fit together"):
        ops.gaussian_fa(z[:3], z[:3] + 1, torch.ones(D, 3).cuda(), torch.zeros(D + 1).cuda(), torch.ones(D).cuda(),
                        torch.ones(D, N).cuda())
