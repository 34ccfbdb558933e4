"""GPU: the eight fused entries that score counts -- poisson_nsf, nb_nsf, poisson_deviance, nb_deviance and their sparse
siblings -- across rate levels 1e-6 .. 1e4, theta 1e-2 .. 1e6, a narrow and a wide latent spread, and a mixed case whose
16-gene tiles each hold eight regimes (tests/range_cases.py; tests/test_range_cases.py checks the cases, the classification
and the bounds on the CPU).  The other suites cover these entries for shape; this one covers them for value range.

Oracles and tolerances are the existing ones (nb_cases.oracle, poisson_cases.reference, deviance_cases.oracle,
nb_deviance_cases.oracle; LL_REL, LL_ABS, G_RTOL, G_ATOL).  Per output:

  * every value is finite;
  * an output of the case's floor, or one the plain fp32 evaluation classifies as in domain, meets its bound --
    dtheta G_RTOL |ref| + G_ATOL C_d (the sum of the absolute values of its summands), the per-gene outputs of the mixed
    case with max|ref| over the genes of the same regime, the value with the lgamma term LL_REL (|value without it| +
    sum lgamma(y + 1)) + LL_ABS, an entry whose oracle value and bound are both 0 exactly 0;
  * an output out of domain meets max(bound, 4 x the error of the plain fp32 evaluation), element-wise;
  * the sparse entries (SparseCounts of the whole data set, idx = None; empty at level 1e-6) meet the same bounds.

Every comparison prints its figures before it asserts; with GPZ_TEST_RECORD_DIR set one line per case, family and entry is
appended to count_range.jsonl there."""
import pytest
import torch

import range_cases as R
from helpers import record

pytestmark = pytest.mark.gpu


def _gpu(c, *keys):
    return [c[k].float().cuda() for k in keys]


def _counts(y):
    from gpzoo_amd.likelihoods import SparseCounts
    return SparseCounts(y.float()).cuda()


def _step(c, family, entry):
    """[(names, tensors)] of a step, once without and once with the lgamma(y + 1) term."""
    from gpzoo_amd import ops
    nb = family == "nb_step"
    y = c["y"] if nb else c["yp"]
    par = _gpu(c, "mean", "scale", "eps", "W", "V") + (_gpu(c, "theta") if nb else [])
    data = y.float().cuda() if entry == "dense" else _counts(y)
    names = R.STEP_GRADS + (("dtheta",) if nb else ())
    runs = []
    for flag, value in ((False, "ll"), (True, "ll_lgamma")):
        if entry == "dense":
            out = (ops.nb_nsf if nb else ops.poisson_nsf)(*par, data, flag)
        else:
            out = (ops.nb_nsf_sparse if nb else ops.poisson_nsf_sparse)(*par, data, None, flag)
        assert out[0].dtype == torch.float64 and len(out) == 1 + len(names)
        runs.append(dict(zip((value,) + names, out)))
    return runs


def _deviance(c, family, entry):
    from gpzoo_amd import ops
    nb = family == "nb_deviance"
    y = c["y"] if nb else c["yp"]
    par = _gpu(c, "mean", "scale", "W", "V") + (_gpu(c, "theta") if nb else [])
    if entry == "dense":
        out = (ops.nb_deviance if nb else ops.poisson_deviance)(*par, y.float().cuda(), True)
    else:
        out = (ops.nb_deviance_sparse if nb else ops.poisson_deviance_sparse)(*par, _counts(y), None, True)
    assert set(out) == set(R.OUTPUTS[family])
    return [out]


def check(cid, family):
    c = R.lookup(cid)
    ev, dom, f32 = R.evaluation(c, family), R.in_domain(c, family), R.f32_figures(c, family)
    strict = set(R.floor(c, family))
    failed = []
    for entry in ("dense", "sparse"):
        runs = (_step if family.endswith("step") else _deviance)(c, family, entry)
        rec = {}
        for got in runs:
            for k, t in got.items():
                assert t.shape == ev["ref"][k].shape, (cid, family, entry, k)
                fig = R.figure(t, ev["ref"][k], ev["bound"][k])
                held = R.figure(t, ev["ref"][k], R.allowed(c, family, k))
                if k in rec:                           # a gradient, run with either flag: the worse of the two
                    fig, held = max(fig, rec[k]["figure"]), max(held, rec[k]["of_allowed"])
                rec[k] = dict(figure=fig, of_allowed=held, in_domain=bool(dom[k] or k in strict), f32_figure=f32[k])
        print(cid, family, entry, {k: f"{v['figure']:.3g}" + ("" if v["in_domain"] else f" (out of domain: fp32 {v['f32_figure']:.3g},"
                                                                                      f" {v['of_allowed']:.3g} of allowed)")
                                   for k, v in rec.items()})
        record("count_range.jsonl", dict(case=cid, level=c["level"], theta=c["theta_all"], spread=c["spread"], family=family,
                                         entry=entry, outputs=rec), append=True)
        failed += [(entry, k, v) for k, v in rec.items() if not v["of_allowed"] <= 1.0]
    assert not failed, (cid, family, failed)


@pytest.mark.parametrize("cid", R.POISSON_IDS)
def test_poisson_step(cid):
    check(cid, "poisson_step")


@pytest.mark.parametrize("cid", R.NB_IDS)
def test_nb_step(cid):
    check(cid, "nb_step")


@pytest.mark.parametrize("cid", R.POISSON_IDS)
def test_poisson_deviance(cid):
    check(cid, "poisson_deviance")


@pytest.mark.parametrize("cid", R.NB_IDS)
def test_nb_deviance(cid):
    check(cid, "nb_deviance")
