"""GPU: every form and tile path of the fused SVGP backward (gpz_svgp_backward) against fp64 torch autograd through the
oracle (tests/backward_forms_cases.py; tests/test_backward_forms_cases.py checks that reference on the CPU).

Each test is one problem with one whitening; inside it every requested (precision, tile kernel, form) variant runs on
the dense random upstream and on the edge-column probes, with g_kl always and g_chol whenever kernel gradients are
asked for.  Bounds:

  fp64   |got - ref| <= 1e-6 (max|ref| + |ref|)                      (tests/test_hip_backward.py's bound)
  fp32   the same with 2e-3 whitened, 5e-3 un-whitened               (tests/test_hip_fuzz.py's ceilings); a quantity
         beyond its ceiling is allowed 4 x the deviation of the SAME oracle evaluated in fp32 torch from its fp64
         evaluation (the factor covers another order of summation) -- never a bound taken from the kernel's output
  fp32 variants of one problem agree with the first of them to 1e-4 (tests/test_hip_wide.py's bound)

Measured on one MI355X (worst max|got - ref| / max|ref| over all cases and quantities of this file; per case in
backward_forms.jsonl under $GPZ_TEST_RECORD_DIR, by (precision, form, whitening) in DESIGN.md section 5):
  fp64   3.0e-12  (dLoss/dZ, shape D in chunks under the whitened clamp recipe, both forms)
  fp32   5.6e-6   (dLoss/dZ, shape H, classic); un-whitened 3.8e-6 (dLoss/dsigma, shape E under the clamp recipe, classic)
No fp32 quantity went beyond its ceiling, so the fp32 evaluation of the oracle was never consulted.
"""
import pytest
import torch

import backward_forms_cases as BC
from helpers import record

pytestmark = pytest.mark.gpu

# tag: (N, M, L) -- the smallest shapes that reach each branch
SHAPES = {
    "tiny1": (1, 1, 1),        # a single point and a single inducing point (d = 1): 127 padded rows and columns
    "tiny5": (5, 2, 1),        # a single row of blocks, 126 padded rows
    "B": (300, 129, 2),        # Mp = 256 with 127 padded rows; ncp = 384: one and a half wide tiles; the library picks classic
    "C": (129, 300, 3),        # N < M: three blocks, the 128-row A B^T kernel, two column tiles (one of a single column)
    "D": (2100, 200, 2),       # ncp = 2176 = 17 * 128: the k extent cut in 2 pieces of 1088 (no multiple of 128); with
                               # chunk = 1024 three chunks, the last a single ragged tile
    "E": (700, 640, 2),        # nblk = 5: the 256-row A B^T kernel with a ragged last row tile, 5 row tiles in the wide product
    "F": (900, 700, 1),        # nblk = 6 and one latent (8 strips wanted from one latent)
    "G": (400, 1100, 2),       # Mp = 1152: 9 blocks, more than 1024 rows in the rank-1 update (fp64 un-whitened only)
    "H": (11008, 640, 16),     # the paired wide schedule with an odd count of row tiles (fp32 whitened only)
}
ALL3 = ("f64", "f32", "f32n")          # fp64 (generic kernel), fp32 wide tiles, fp32 narrow_tiles=True
CEIL32 = {True: 2e-3, False: 5e-3}     # by whitened


def _cases():
    out = []

    def add(tag, kind="nsf_rbf", d=2, recipe=None, whitened=True, kg=True, chunk=0, retain=False, variants=ALL3):
        N, M, L = SHAPES[tag]
        if kind == "rbf_scalar":
            L = 1
        name = f"{tag}-{kind}-d{d}-{'w' if whitened else 'u'}-{'all' if kg else 'muLu'}" + \
               (f"-chunk{chunk}" if chunk else "") + (f"-{recipe}" if recipe else "")
        out.append(pytest.param(dict(tag=tag, N=N, M=M, L=L, kind=kind, d=d, recipe=recipe, whitened=whitened, kg=kg,
                                     chunk=chunk, retain=retain, variants=variants), id=name))

    for wh in (True, False):
        for kg in (False, True):
            for tag in "BCDEF":
                add(tag, whitened=wh, kg=kg, retain=tag in "DE")      # D and E also with the forward's retained Wt
            add("D", whitened=wh, kg=kg, chunk=1024, retain=True)
        for kind in ("rbf_scalar", "matern12", "matern32", "matern52", "mggp_nsf_rbf"):
            add("C", kind=kind, d=1 if kind == "rbf_scalar" else 2, whitened=wh, variants=("f64", "f32"))
            add("D", kind=kind, d=3 if kind == "matern52" else 2, whitened=wh, variants=("f64", "f32"))
        add("tiny1", d=1, whitened=wh, variants=("f64",))
        add("tiny5", whitened=wh, variants=("f64",))
    add("G", whitened=False, variants=("f64",))
    # columns at the clamps, on both sides of them in every latent
    add("B", recipe="whitened_clamp", whitened=True)
    add("D", recipe="whitened_clamp", whitened=True, chunk=1024)     # the third chunk holds no clamped column: Hd's gate both ways
    for tag in "BDE":
        add(tag, recipe="unwhitened_clamp", whitened=False)
    return out


def _spec(c, dt):
    from gpzoo_amd import _lib
    from gpzoo_amd.ops import KernelSpec
    cu = lambda t: t.to(dt).cuda()   # noqa: E731
    kid = {"nsf_rbf": _lib.KERNEL_RBF, "rbf_scalar": _lib.KERNEL_RBF, "matern12": _lib.KERNEL_MATERN12,
           "matern32": _lib.KERNEL_MATERN32, "matern52": _lib.KERNEL_MATERN52, "mggp_nsf_rbf": _lib.KERNEL_MGGP_RBF}[c["kind"]]
    if c["kind"] == "mggp_nsf_rbf":
        emb = BC.embedding_of(c)
        r2 = ((emb[:, None, :] - emb[None, :, :]) ** 2).sum(-1)
        return KernelSpec(kid, cu(c["sigma"]), cu(c["lengthscale"]), True, cu(c["group_diff"] ** 2), cu(r2), 1.0), \
            dict(gX=c["gX"].cuda(), gZ=c["gZ"].cuda())
    return KernelSpec(kid, cu(c["sigma"]), cu(c["lengthscale"]), c["kind"] != "rbf_scalar"), {}


class _Problem:
    """One case on the device in one precision: the forward pass (scale, retained Wt) is shared by its backward runs."""

    def __init__(self, c, whitened, dt, chunk, retain):
        from gpzoo_amd import ops
        self.c, self.whitened, self.dt, self.chunk = c, whitened, dt, chunk
        self.spec, self.extra = _spec(c, dt)
        cu = lambda t: t.to(dt).cuda()   # noqa: E731
        self.args = (self.spec, cu(c["X"]), cu(c["Z"]), cu(c["mu"]), cu(c["Lu_raw"]), c["jitter"], whitened)
        self.kw = dict(clamp_min=c["clamp_min"], chunk=chunk, **self.extra)
        self.fwd = ops.svgp_forward(*self.args, want_Lu=False, retain_wt=0.5 if retain else 0.0, **self.kw)
        assert not retain or "wt_cache" in self.fwd

    def backward(self, up, kg, form, narrow=False, use_wt=False):
        from gpzoo_amd import ops
        cu = lambda t: t.to(self.dt).cuda()   # noqa: E731
        res = ops.svgp_backward(*self.args, cu(up["gm"]), cu(up["gs"]), self.fwd["scale"], kernel_grads=kg,
                                g_chol=cu(up["gc"]) if kg else None, g_kl=up["w"].cuda(), narrow_tiles=narrow, form=form,
                                wt_cache=self.fwd["wt_cache"] if use_wt else None, **self.kw)
        out = {"mu": res[0], "Lu_raw": res[1]}
        if kg:
            out.update(sigma=res[2][:, 0], lengthscale=res[2][:, 1], Z=res[3])
            if "group_diff" in self.c:      # the library differentiates w.r.t. the effective multiplier a^2: chain rule 2a
                out["group_diff"] = res[2][:, 2] * 2 * self.c["group_diff"].cuda()
        return {k: v.double().cpu() for k, v in out.items()}


def _rel(got, ref):
    return float((got.reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _within(got, ref, rt):
    """|got - ref| <= rt (max|ref| + |ref|): torch.testing.assert_close(rtol=rt, atol=rt * max|ref|)."""
    return bool(((got.reshape(ref.shape) - ref).abs() <= rt * (max(float(ref.abs().max()), 1e-30) + ref.abs())).all())


def _check_against_oracle(got, ref, f32, whitened, what, ref32):
    """Every quantity finite and inside its bound; returns {name: relative error}.  ``ref32``: a callable giving the
    same oracle's fp32 evaluation, asked for only when an fp32 quantity is beyond its ceiling."""
    errs = {}
    for name, g in got.items():
        r = ref[name]
        assert torch.isfinite(g).all(), f"{what}: {name} is not finite"
        errs[name] = _rel(g, r)
        print(f"{what}: {name} {errs[name]:.3e}")
        if not f32:
            assert _within(g, r, 1e-6), f"{what}: {name} off by {errs[name]:.3e} of max|ref| (fp64 bound 1e-6)"
        elif not _within(g, r, CEIL32[whitened]):
            dev = _rel(ref32()[name], r)
            print(f"{what}: {name} beyond the ceiling {CEIL32[whitened]:.0e}; the fp32 oracle deviates by {dev:.3e}")
            assert errs[name] <= 4 * dev, (f"{what}: {name} off by {errs[name]:.3e} of max|ref|; ceiling "
                                           f"{CEIL32[whitened]:.0e}, fp32 evaluation of the oracle off by {dev:.3e}")
    return errs


def _run_case(p, oracle_device="cpu"):
    c = BC.make_case(p["N"], p["M"], p["L"], kind=p["kind"], d=p["d"], recipe=p["recipe"])
    wh, kg, chunk = p["whitened"], p["kg"], p["chunk"]
    problems = {}
    for v in p["variants"]:
        dt = torch.float64 if v == "f64" else torch.float32
        if dt not in problems:
            problems[dt] = _Problem(c, wh, dt, chunk, p["retain"])
    worst = {}
    for which in ("dense", "probe"):
        up = BC.make_upstream(c, wh, which, chunk, device=oracle_device)
        ref = BC.oracle_grads(c, wh, which, chunk, device=oracle_device)
        ref32 = lambda: BC.oracle_grads(c, wh, which, chunk, device=oracle_device, dtype=torch.float32)   # noqa: E731
        first32 = None
        for v in p["variants"]:
            f32 = v != "f64"
            prob = problems[torch.float32 if f32 else torch.float64]
            for form in ("classic", "algebra"):
                for use_wt in ((False, True) if p["retain"] else (False,)):
                    what = f"{which} {v} {form}" + (" retained-Wt" if use_wt else "")
                    got = prob.backward(up, kg, form, narrow=v == "f32n", use_wt=use_wt)
                    errs = _check_against_oracle(got, ref, f32, wh, what, ref32)
                    for k, e in errs.items():
                        key = f"{'f32' if f32 else 'f64'}/{form}/{k}"
                        worst[key] = max(worst.get(key, 0.0), e)
                    if f32 and first32 is None:
                        first32 = (what, got)
                    elif f32:
                        for k, g in got.items():
                            assert _within(g, first32[1][k], 1e-4), \
                                f"{what} against {first32[0]}: {k} differs by {_rel(g, first32[1][k]):.3e} (bound 1e-4)"
    record("backward_forms.jsonl", dict(tag=p["tag"], N=p["N"], M=p["M"], L=p["L"], kind=p["kind"], d=p["d"],
                                        recipe=p["recipe"], whitened=wh, kernel_grads=kg, chunk=chunk, worst=worst), append=True)


@pytest.mark.parametrize("p", _cases())
def test_backward_forms_against_fp64_autograd(p):
    """Both forms x the requested precisions / tile kernels (x retained Wt where asked) on the dense and the probe
    upstream, every gradient against the CPU oracle's autograd."""
    _run_case(p)


def test_paired_schedule_with_an_odd_row_tile_count():
    """Shape H (N=11008, M=640, L=16, fp32 whitened): every wide product of the pass on the paired schedule.  Rechecked
    against wide_product_launch_t (csrc/gemmw.hip): ncp = 11008 = 43 column tiles of 256 -> ceil(43 / 16) = 3 strips (8
    units are already there with 16 latents), W = ceil(43 / 3) = 15; mtw = 640 / 128 = 5 row tiles; units = 16 * 3 = 48;
    paired = 48 * ceil(5 / 2) * 15 = 2160 >= 4 * 512, so pair = colmajor = 1 with an ODD count of row tiles (the last
    pair of every column is half empty).  The A B^T accumulations: 11 tile slots * 16 = 176 tiles -> 2 pieces of 5504.
    The oracle runs in torch fp64 on the GPU (rocBLAS, nothing of this library)."""
    N, M, L = SHAPES["H"]
    _run_case(dict(tag="H", N=N, M=M, L=L, kind="nsf_rbf", d=2, recipe=None, whitened=True, kg=True, chunk=0,
                   retain=False, variants=("f32",)), oracle_device="cuda")


@pytest.mark.parametrize("tag", list(SHAPES))
def test_library_choice_is_the_documented_rule(tag):
    """form=None gives, bit for bit, the forced form that the rule in backward_algebra's comment selects
    (all parameters: N >= 2.2 Mp, un-whitened fp32 N >= 4.4 Mp; mu / Lu only: N >= 0.75 Mp)."""
    N, M, L = SHAPES[tag]
    f32 = tag not in ("tiny1", "tiny5", "G")
    c = BC.make_case(N, M, L, d=1 if tag == "tiny1" else 2)
    for wh in ((True,) if tag == "H" else (False,) if tag == "G" else (True, False)):
        up = BC.make_upstream(c, wh, "dense", device="cuda" if tag == "H" else "cpu")
        prob = _Problem(c, wh, torch.float32 if f32 else torch.float64, 0, False)
        for kg in (True, False):
            rule = "algebra" if BC.library_picks_algebra(N, M, kg, f32, wh) else "classic"
            own, forced = prob.backward(up, kg, None), prob.backward(up, kg, rule)
            other = prob.backward(up, kg, "classic" if rule == "algebra" else "algebra")
            for k in own:
                assert torch.equal(own[k], forced[k]), f"{tag} whitened={wh} kernel_grads={kg}: {k} is not the {rule} form's"
            if M > 128:             # the comparison tells the forms apart: they differ in at least one bit somewhere
                assert any(not torch.equal(own[k], other[k]) for k in own), (tag, wh, kg)
