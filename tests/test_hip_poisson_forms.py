"""GPU: every kernel instance, tile edge and plan branch of the fused Poisson step (gpz_poisson_nsf, csrc/poisson.hip)
against the fp64 torch autograd evaluation of the same formula (tests/poisson_cases.py; tests/test_poisson_cases.py
checks the case lists, the probes and that reference on the CPU).

Bounds, the ones tests/test_hip_poisson.py::test_random_poisson_shapes already puts on this kernel:

  ll          pytest.approx(ref, rel=5e-5, abs=1e-3)
  gradients   assert_close(rtol=1e-3, atol=1e-3 max|ref|)

They are not tightened here.  What makes them sufficient at the plan branches is the probe counts: every element next
to a slice, group, tile or vector-group boundary holds a count whose share of each output it feeds is at least ten
times that output's tolerance (asserted on the CPU), so one element dropped or counted twice fails the comparison.
The exception is (64, 16385, 5, 1), sharp in ll with the lgamma term and in dW only (see the CPU test).

Every comparison prints its figures (err / tolerance per output) before it asserts; with GPZ_TEST_RECORD_DIR set they
are also appended to poisson_forms.jsonl there."""
import ctypes as C

import pytest
import torch

import poisson_cases as PC
from helpers import record

pytestmark = pytest.mark.gpu

NAMES = ("ll",) + PC.OUTPUTS


def _dev(c):
    return [c[k].float().cuda() for k in ("mean", "scale", "eps", "W", "V", "y")]


def run(c, with_lgamma, args=None):
    """ops.poisson_nsf on the case: (ll, dmean, dscale, dW, dV), device tensors."""
    from gpzoo_amd import ops
    out = ops.poisson_nsf(*(args or _dev(c)), with_lgamma)
    assert out[0].dtype == torch.float64 and all(t.dtype == torch.float32 for t in out[1:])
    return out


def check(c, got, with_lgamma, tag):
    ref = PC.reference(c, with_lgamma)
    ll = float(got[0])
    fig = {"ll": abs(ll - ref["ll"]) / float(PC.tolerance(ref, "ll"))}
    for nm, t in zip(PC.OUTPUTS, got[1:]):
        assert t.shape == ref[nm].shape and bool(torch.isfinite(t).all()), (nm, tag)
        fig[nm] = float(((t.double().cpu() - ref[nm]).abs() / PC.tolerance(ref, nm)).max())
    print(tag, "with_lgamma" if with_lgamma else "no_lgamma", "err/tol", {k: f"{v:.3g}" for k, v in fig.items()})
    record("poisson_forms.jsonl", dict(case=str(tag), with_lgamma=with_lgamma, err_over_tol=fig), append=True)
    assert ll == pytest.approx(ref["ll"], rel=PC.LL_REL, abs=PC.LL_ABS), tag
    for nm, t in zip(PC.OUTPUTS, got[1:]):
        torch.testing.assert_close(t.double().cpu(), ref[nm], rtol=PC.G_RTOL, atol=PC.G_ATOL * float(ref[nm].abs().max()),
                                   msg=lambda m: f"{nm} {tag}: {m}")


def _id(shape):
    return "N{}-D{}-Lt{}-E{}".format(*shape)


# --- a. every factor count -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", PC.FACTOR_SWEEP, ids=_id)
def test_every_factor_count(shape):
    """Lt = 1 .. 64 at one full tile plus 6 spots (N % 4 != 0: scalar loads and stores) and two gene groups plus 5
    genes: all 13 instances of both passes, every tail length of pass B, the padded k-steps of KS = 12, 14 and 16."""
    c = PC.make_case(*shape)
    with_lgamma = bool(shape[2] % 2)
    check(c, run(c, with_lgamma), with_lgamma, shape)


@pytest.mark.parametrize("shape", PC.INSTANCE_ENDS, ids=_id)
def test_interior_path_of_each_instance(shape):
    """N = 128, D = 64: every group and tile is whole and rows are 16-byte aligned, so both passes take their
    branch-free interior forms, where the padded factor slots are read through a clamped index."""
    c = PC.make_case(*shape)
    with_lgamma = not shape[2] % 2
    check(c, run(c, with_lgamma), with_lgamma, shape)


# --- b. tile edges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", PC.TILE_EDGES, ids=_id)
def test_tile_edges(shape):
    """Spot counts around the 64-spot tile and the 4-spot vector group, gene counts around the 16-gene group and the
    64-gene block, with (Lt = 20) and without (Lt = 8) pass B's vector tail; three samples.  Dense inputs: at these
    sizes one element is more than 0.5 % of any sum it enters."""
    c = PC.make_case(*shape)
    with_lgamma = bool((shape[0] + shape[1]) % 2)
    check(c, run(c, with_lgamma), with_lgamma, shape)


# --- c. plan branches, d. host split ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", PC.PLAN_CASES + [PC.HOST_SPLIT], ids=_id)
def test_plan_branches_with_probe_counts(shape):
    """Gene slices whose boundaries are no multiple of 16, the S = 32 and SN = 16 caps (the latter with an empty last
    spot slice, which must still write a zero slab), an odd number of sample groups over several tiles, the host's
    split of 65 samples into 32 + 32 + 1 -- each with sharp probe counts at every boundary, with and without the
    lgamma term (counted once however many calls the host makes); the gradients do not depend on the term, bit for bit."""
    c = PC.make_probe_case(*shape)
    args = _dev(c)
    plain, full = run(c, False, args), run(c, True, args)
    check(c, plain, False, shape)
    check(c, full, True, shape)
    for nm, a, b in zip(PC.OUTPUTS, plain[1:], full[1:]):
        assert torch.equal(a, b), nm


# --- e. counts -------------------------------------------------------------------------------------------------------

def test_counts_beyond_the_table_and_empty_rows():
    """y with 0, 255, 256, 257, 12 345, 2.5 and 300.25 (lgamma_sum_kernel's table ends at 255: lgammaf for the rest), a
    gene without counts and a spot without counts."""
    c = PC.make_counts_case()
    args = _dev(c)
    for with_lgamma in (True, False):
        check(c, run(c, with_lgamma, args), with_lgamma, "counts")
    lg = float(torch.lgamma(c["y"] + 1.0).sum())
    d = float(run(c, False, args)[0]) - float(run(c, True, args)[0])
    print("lgamma sum", d, "reference", lg)
    # lgamma_sum_kernel adds up to 64 terms in fp32 before it goes to fp64: 64 * 2^-24 = 3.8e-6 of the sum at worst,
    # plus a few fp32 ulp (6e-8 each) of lgammaf per term
    assert d == pytest.approx(lg, rel=1e-5)


# --- f. reproducibility and workspace reuse --------------------------------------------------------------------------

def test_bitwise_reproducible_across_workspace_reuse():
    """The workspace is shared by consecutive calls and never cleared.  A small shape on a fresh workspace, then after
    a large shape has filled it, then after the whole buffer was overwritten with NaN bit patterns: the small shape's
    five outputs are the same bits each time (a read of a slab entry this call did not write would differ), and so
    are the large shape's."""
    from gpzoo_amd import ops
    big, small = PC.make_probe_case(*PC.LARGE), PC.make_case(*PC.SMALL)
    ab, asm = _dev(big), _dev(small)
    ops.release_workspaces()
    s0 = run(small, True, asm)
    b1 = run(big, True, ab)
    s1 = run(small, True, asm)
    b2 = run(big, True, ab)
    s2 = run(small, True, asm)
    torch.cuda.synchronize()
    assert ops._workspaces and all(w.numel() >= PC.workspace_bytes(*PC.LARGE) for w in ops._workspaces.values())
    for w in ops._workspaces.values():
        w.fill_(0xFF)
    s3 = run(small, True, asm)
    b3 = run(big, True, ab)
    for nm, *ts in zip(NAMES, s0, s1, s2, s3):
        assert all(torch.equal(ts[0], t) for t in ts[1:]), ("small", nm)
    for nm, *ts in zip(NAMES, b1, b2, b3):
        assert all(torch.equal(ts[0], t) for t in ts[1:]), ("large", nm)
    check(small, s3, True, PC.SMALL)
    check(big, b3, True, PC.LARGE)


# --- g. argument checks, the alignment contract ----------------------------------------------------------------------

SENTINEL = -777.0


class Direct:
    """gpz_poisson_nsf through ctypes with the tensors of a small case; outputs pre-filled with a sentinel."""

    def __init__(self, shape=(68, 37, 20, 3)):
        from gpzoo_amd import _lib
        self.lib = _lib.load()
        self.N, self.D, self.Lt, self.E = shape
        self.c = PC.make_case(*shape)
        self.args = _dev(self.c)
        dev = self.args[0].device
        full = lambda *s, dt=torch.float32: torch.full(s, SENTINEL, dtype=dt, device=dev)   # noqa: E731
        self.out = [full(2, dt=torch.float64), full(self.Lt, self.N), full(self.Lt, self.N), full(self.D, self.Lt), full(self.N)]
        self.nbytes = self.lib.gpz_poisson_nsf_workspace_bytes(self.N, self.D, self.Lt, self.E)
        self.ws = torch.empty(self.nbytes + 256, dtype=torch.uint8, device=dev)

    def call(self, args=None, N=None, D=None, Lt=None, E=None, ws_bytes=None, ws_ptr=None):
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        a = args or self.args
        pick = lambda v, d: d if v is None else v   # noqa: E731
        rc = self.lib.gpz_poisson_nsf(*[p(t) for t in a], pick(N, self.N), pick(D, self.D), pick(Lt, self.Lt), pick(E, self.E),
                                      1, *[p(t) for t in self.out], C.c_void_p(pick(ws_ptr, self.ws.data_ptr())),
                                      pick(ws_bytes, self.nbytes), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, self.lib.gpz_last_error().decode("utf-8", "replace")

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.out)


def test_argument_errors_are_refused_before_any_launch():
    d = Direct()
    assert d.nbytes == PC.workspace_bytes(d.N, d.D, d.Lt, d.E)
    for kw, msg in ((dict(E=33), "33 samples per call unsupported (1..32)"),
                    (dict(E=0), "0 samples per call unsupported (1..32)"),
                    (dict(ws_bytes=d.nbytes - 1), "workspace too small"),
                    # E Lt N * 4 bytes = 2^31 exactly, with ws_bytes = 16: even without the guard the workspace check refuses
                    (dict(E=32, Lt=64, N=1 << 18, ws_bytes=16), "exceed the 2 GiB a call can address"),
                    (dict(E=32, Lt=64, N=(1 << 18) - 1, ws_bytes=16), "workspace too small"),     # one spot fewer: past the guard
                    (dict(Lt=65), "65 factors unsupported"),
                    (dict(N=0), "bad extents"),
                    (dict(ws_ptr=d.ws.data_ptr() + 4), "16-byte aligned")):
        rc, err = d.call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
        assert d.untouched(), kw
    rc, err = d.call()                            # the same arguments unchanged: accepted, and the sentinels are gone
    assert rc == 0, err
    assert not d.untouched()
    got = [d.out[0][0] - d.out[0][1]] + d.out[1:]
    check(d.c, got, True, "direct")


def _shifted(t):
    """The same values as a contiguous view one element into a larger storage (4 bytes past a 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("shape", [(68, 37, 20, 3), (128, 64, 8, 2)], ids=_id)
def test_misaligned_inputs(shape):
    """N % 4 == 0, where both passes read y 16 bytes at a time: y, W and mean handed over as views at a one-element
    storage offset give the bits of aligned copies through ops.poisson_nsf (which copies them), and the C entry
    refuses each such pointer."""
    d = Direct(shape)
    want = run(d.c, True, d.args)
    moved = list(d.args)
    for i in (0, 3, 5):                           # mean, W, y
        moved[i] = _shifted(d.args[i])
    got = run(d.c, True, moved)
    for nm, a, b in zip(NAMES, want, got):
        assert torch.equal(a, b), nm
    check(d.c, got, True, shape)
    for i in range(6):
        one = list(d.args)
        one[i] = _shifted(d.args[i])
        rc, err = d.call(args=one)
        assert rc != 0 and "16-byte aligned" in err, (i, rc, err)
        assert d.untouched(), i
