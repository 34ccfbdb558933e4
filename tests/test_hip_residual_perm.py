"""GPU: Geary's C, the kurtosis and the permutation null of the residual entries (csrc/residual.hip over the wide and the
permutation column passes of csrc/spatial_stats.hip) against tests/residual_perm_cases.py -- every stage against the fp64
oracle of the entry's own residuals, the bits the entries share, the counts inside their bracket, all 5040 relabellings of
seven spots against the randomisation moments, C end to end, the planted structure through the permutation p-values, and
the model method."""
import functools

import numpy as np
import pytest
import torch

import geary_cases as Y
import residual_cases as R
import residual_perm_cases as Q
import test_hip_residual_autocorr as TR

pytestmark = pytest.mark.gpu

COMBOS = TR.COMBOS
STATS = ("moran", "geary")
STAT_FIELDS = ("I", "C", "residual_mean", "residual_var", "kurtosis")
PERM_FIELDS = ("value", "n_ge", "n_le", "sim_mean", "sim_m2", "sims")
_t = TR._t


def _stats(d, kind, family, nbr, y=None, **kw):
    from gpzoo_amd import ops
    a, th = TR._args(d, family, y)
    r = ops.residual_spatial_stats(*a, nbr, theta_pos=th, kind=kind, **kw)
    assert tuple(r) == STAT_FIELDS and all(t.dtype == torch.float64 and t.is_cuda for t in r.values())
    return r


def _perm(d, kind, family, nbr, perms, stat, y=None, **kw):
    from gpzoo_amd import ops
    a, th = TR._args(d, family, y)
    r, mom = ops.residual_autocorr_perm(*a, nbr, perms, theta_pos=th, kind=kind, stat=stat, return_sims=True, **kw)
    assert r.stat == stat and r.n_ge.dtype == r.n_le.dtype == torch.int32 and tuple(mom) == STAT_FIELDS[2:]
    return r, mom


def _all_bits(r, mom):
    return [TR._bits(getattr(r, f)) for f in PERM_FIELDS] + [TR._bits(t) for t in mom.values()]


def _same_bits(a, b, msg):
    for x, z in zip(a, b):
        np.testing.assert_array_equal(x, z, err_msg=msg)


@functools.lru_cache(maxsize=None)
def _rows600():
    """D = 6, B = 600 (three row chunks, a partial column tile), dense and stored: _sparse_case's construction."""
    return TR._sparse_case("rows")


# --- 1. every stage against the oracle of the entry's own residuals, and 3. the counts ----------------------------------------

def _check_stage(d, nbr_np, slab_genes, what):
    B = nbr_np.shape[0]
    nbr, perms_np = _t(nbr_np, torch.int64), Q.perms_of(B)
    perms = _t(perms_np, torch.int32)
    assert perms_np.shape[0] == Q.P == 19
    for kind, family in COMBOS:
        res = TR._residuals(d, kind, family).T.double().cpu().numpy()
        want = Q.stats(res, nbr_np)
        got = _stats(d, kind, family, nbr, slab_genes=slab_genes)
        for f, w in zip(STAT_FIELDS[:4], ("I", "C", "mean", "var")):
            TR._close(got[f].cpu().numpy(), want[w], f"{what} {kind} {family} {f}")
        kerr = np.abs(got["kurtosis"].cpu().numpy() / want["kurtosis"] - 1.0).max()
        print(what, kind, family, "kurtosis: max relative error", kerr)
        assert kerr <= Y.KURTOSIS_RTOL
        sims_want = dict(zip(STATS, Q.perm_stats(res, nbr_np, perms_np)))
        for stat in STATS:
            r, mom = _perm(d, kind, family, nbr, perms, stat, slab_genes=slab_genes)
            sims = r.sims.cpu().numpy()
            err = np.abs(sims - sims_want[stat]).max()
            print(what, kind, family, stat, "max |sims - oracle|", err)
            assert sims.shape == sims_want[stat].shape and err <= Q.MORAN_ATOL
            # the running mean and M2 against the device's own simulated values (the bound of tests/test_hip_geary.py)
            e = Q.MORAN_ATOL
            np.testing.assert_allclose(r.sim_mean.cpu().numpy(), sims.mean(axis=1), rtol=0, atol=e)
            np.testing.assert_array_less(np.abs((r.sim_m2 / Q.P).cpu().numpy() - sims.var(axis=1)),
                                         2 * sims.std(axis=1) * e + e ** 2 + 1e-15)
            # 3. the counts inside the bracket around the oracle
            observed = want["I" if stat == "moran" else "C"]
            ge, le, band = Q.counts_bracket(observed, sims_want[stat])
            n_ge, n_le = r.n_ge.cpu().numpy(), r.n_le.cpu().numpy()
            assert (ge <= n_ge).all() and (n_ge <= ge + band).all(), (what, kind, family, stat)
            assert (le <= n_le).all() and (n_le <= le + band).all(), (what, kind, family, stat)
            assert (n_ge + n_le >= Q.P).all() and (band >= 1).all()        # the identity row is inside every band


@pytest.mark.parametrize("K", [1, 6, 32])
def test_stages_at_three_slabs_against_the_oracle_of_the_own_residuals(K):
    """two_blocks (130 x 130) at slab_genes = 64: three slabs, the last one two genes wide (other thread slots)."""
    from gpzoo_amd import ops
    plan = ops.residual_autocorr_perm_plan(130, 130, 8, K, Q.P, 0, 64)
    assert (plan["n_slabs"], plan["perm_batch"], plan["batches"]) == (3, 16, 2)
    _check_stage(TR._dev("two_blocks"), R.random_table(130, K, seed=K), 64, f"two_blocks K={K}")


@pytest.mark.parametrize("name", ["long_rows", "one_past"])
def test_stages_at_a_second_row_chunk_and_one_past_a_tile(name):
    """long_rows (B = 257): a second 256-row chunk holding one spot.  one_past (65 x 65): two column tiles."""
    c = R.make_case(name)
    _check_stage(TR._dev(name), R.case_table(c), 0, name)


def test_stages_at_three_row_chunks_and_a_partial_column_tile():
    d, _ = _rows600()
    _check_stage(d, R.random_table(600, 6, seed=6), 0, "rows600")


# --- 2. bits -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,slab_genes", [("two_blocks", 64), ("long_rows", 0)])
def test_the_bits_the_entries_share(name, slab_genes):
    """The stats entry's I, mean and variance are residual_morans_i's; the permutation entry's value is the stats entry's I or
    C; an identity row reproduces it and counts on both sides."""
    c, d = R.make_case(name), TR._dev(name)
    nbr = _t(R.case_table(c), torch.int64)
    perms = _t(Q.perms_of(c["B"]), torch.int32)
    for kind, family in COMBOS:
        narrow = TR._moran(d, kind, family, nbr, slab_genes=slab_genes)
        wide = _stats(d, kind, family, nbr, slab_genes=slab_genes)
        for f in ("I", "residual_mean", "residual_var"):
            assert torch.equal(narrow[f], wide[f]), (kind, family, f)
        for stat in STATS:
            r, mom = _perm(d, kind, family, nbr, perms, stat, slab_genes=slab_genes)
            assert torch.equal(r.value, wide["I" if stat == "moran" else "C"]), (kind, family, stat)
            assert torch.equal(r.sims[:, 0], r.value)
            assert all(torch.equal(mom[f], wide[f]) for f in mom)
            without = _perm(d, kind, family, nbr, perms[1:], stat, slab_genes=slab_genes)[0]
            assert torch.equal(r.n_ge, without.n_ge + 1) and torch.equal(r.n_le, without.n_le + 1)
            assert torch.equal(r.sims[:, 1:], without.sims)


def test_nothing_depends_on_the_batch_size():
    d = TR._dev("two_blocks")
    nbr = _t(R.case_table(R.make_case("two_blocks")), torch.int64)
    perms = _t(Q.perms_of(130), torch.int32)
    for kind, family in (("pearson", "nb"), ("deviance", "poisson")):
        for stat in STATS:
            first = _all_bits(*_perm(d, kind, family, nbr, perms, stat, slab_genes=64, perm_batch=1))
            for pb in (3, 0, 32):
                _same_bits(first, _all_bits(*_perm(d, kind, family, nbr, perms, stat, slab_genes=64, perm_batch=pb)), f"{stat} {pb}")


def test_the_same_bits_on_poisoned_and_stale_scratch():
    """No region of the scratch is read before this call has written it: the slab, the wide pass's partials, the relabelled
    tables and their `written` words, the permutations' partials and the observed sums."""
    from gpzoo_amd import ops
    d, sc = TR._sparse_case("holes")
    nbr, perms = _t(R.random_table(130, 6, seed=2), torch.int64), _t(Q.perms_of(130), torch.int32)
    other, other_nbr = TR._dev("long_rows"), _t(R.random_table(257, 3, seed=2), torch.int64)

    def run():
        out = []
        for y in (None, sc):
            out += [TR._bits(t) for t in _stats(d, "deviance", "nb", nbr, y=y, slab_genes=64).values()]
            out += _all_bits(*_perm(d, "deviance", "nb", nbr, perms, "geary", y=y, slab_genes=64, perm_batch=3))
        return out
    first = run()
    ws = ops._workspace(torch.device("cuda", torch.cuda.current_device()), 1)
    assert ws.numel() >= ops.residual_autocorr_perm_plan(130, 130, 8, 6, Q.P, sc.nnz, 64, 3)["partials_bytes"]
    ws.fill_(0xFF)
    poisoned = run()
    _perm(other, "pearson", "poisson", other_nbr, _t(Q.perms_of(257), torch.int32), "moran")      # the leftovers of another shape
    _same_bits(first, poisoned, "poisoned")
    _same_bits(first, run(), "stale")


@pytest.mark.parametrize("which", ["holes", "rows"])
def test_the_sparse_entries_give_the_dense_entries_bits(which):
    d, sc = TR._sparse_case(which)
    B = d["y"].shape[1]
    nbr = _t(R.random_table(B, 6, seed=3), torch.int64)
    perms = _t(Q.perms_of(B), torch.int32)
    for kind, family in COMBOS:
        a, b = _stats(d, kind, family, nbr, y=sc, slab_genes=64), _stats(d, kind, family, nbr, slab_genes=64)
        assert all(torch.equal(a[k], b[k]) for k in a)
        for stat in STATS:
            _same_bits(_all_bits(*_perm(d, kind, family, nbr, perms, stat, y=sc, slab_genes=64)),
                       _all_bits(*_perm(d, kind, family, nbr, perms, stat, slab_genes=64)), f"{which} {kind} {family} {stat}")


def test_three_slabs_against_one_slab():
    """Values agree to 1e-10 and the counts lie within the bracket, not bit for bit: a slab of two columns is summed by other
    thread slots than one of 130 (test_hip_residual_autocorr.test_three_slabs_give_what_one_slab_gives)."""
    c, d = R.make_case("two_blocks"), TR._dev("two_blocks")
    nbr_np = R.case_table(c)
    nbr, perms = _t(nbr_np, torch.int64), _t(Q.perms_of(130), torch.int32)
    for kind, family in COMBOS:
        for stat in STATS:
            three, m3 = _perm(d, kind, family, nbr, perms, stat, slab_genes=64)
            one, m1 = _perm(d, kind, family, nbr, perms, stat, slab_genes=192)
            for f in ("value", "sims", "sim_mean"):
                TR._close(getattr(three, f).cpu().numpy(), getattr(one, f).cpu().numpy(), f"{kind} {family} {stat} {f}")
            for f in m3:
                TR._close(m3[f].cpu().numpy(), m1[f].cpu().numpy(), f"{kind} {family} {stat} {f}")
            ge, le, band = Q.counts_bracket(one.value.cpu().numpy(), one.sims.cpu().numpy())
            n_ge, n_le = three.n_ge.cpu().numpy(), three.n_le.cpu().numpy()
            assert (ge <= n_ge).all() and (n_ge <= ge + band).all() and (le <= n_le).all() and (n_le <= le + band).all()


@pytest.mark.parametrize("bad", ["table", "repeat", "range"])
def test_device_side_findings_raise(bad):
    d = TR._dev("one_past")
    nbr = _t(R.case_table(R.make_case("one_past")), torch.int64).clone()
    perms = _t(Q.perms_of(65), torch.int32).clone()
    if bad == "table":
        nbr[40, 2] = 40
        match = "naming its own row"
    else:
        perms[18, 7] = perms[18, 8] if bad == "repeat" else 65
        match = "not a permutation"
    with pytest.raises(ValueError, match=match):
        _perm(d, "pearson", "poisson", nbr, perms, "geary")
    if bad == "table":
        with pytest.raises(ValueError, match=match):
            _stats(d, "pearson", "poisson", nbr)


# --- 4. enumeration ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", sorted(Y.ENUM_TABLES))
def test_all_5040_relabellings_give_the_randomisation_moments(table):
    """mean_sim and var_sim of I and C over every relabelling of seven spots are the analytic randomisation moments at the
    device's own kurtosis; the normality variance is visibly another number."""
    from gpzoo_amd.utilities import _autocorr_moments
    c = Q.enum_case()
    d = {k: _t(c[k]) for k in ("mean", "scale", "W", "V", "y", "theta")}
    nbr_np = Y.ENUM_TABLES[table]
    nbr, perms = _t(nbr_np, torch.int64), _t(Y.enum_perms(), torch.int32)
    enum = Q.enum_moments(TR._residuals(d, "pearson", "poisson").T.double().cpu().numpy(), nbr_np)   # of the entry's own residuals
    for stat, E, V in (("moran", "EI", "VI"), ("geary", "EC", "VC")):
        r, mom = _perm(d, "pearson", "poisson", nbr, perms, stat)
        m = _autocorr_moments(nbr, mom["kurtosis"])
        mean, var = r.sim_mean.cpu().numpy(), (r.sim_m2 / 5040).cpu().numpy()
        print(table, stat, mean / float(m[E]) - 1, var / m[V + "_rand"].cpu().numpy() - 1)
        np.testing.assert_allclose(mean, float(m[E]), rtol=Y.ENUM_RTOL, atol=0)
        np.testing.assert_allclose(var, m[V + "_rand"].cpu().numpy(), rtol=Y.ENUM_RTOL, atol=0)
        # from the CPU oracle: which gene's randomisation variance is furthest from the normality variance, and by how much
        gap = enum[V] / float(m[V + "_norm"]) - 1.0
        g = int(np.abs(gap).argmax())
        assert abs(gap[g]) >= 0.05, (table, stat, gap)
        dev_gap = var / float(m[V + "_norm"]) - 1.0
        assert int(np.abs(dev_gap).argmax()) == g and abs(dev_gap[g] - gap[g]) <= Y.ENUM_RTOL * (1.0 + abs(gap[g]))


# --- 5. end to end --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TR.CASES)
def test_i_and_c_end_to_end_against_the_oracle(name):
    c, d = R.make_case(name), TR._dev(name)
    nbr = R.case_table(c)
    for kind, family in COMBOS:
        ref = R.oracle_residuals(c, kind, family)
        got = _stats(d, kind, family, _t(nbr, torch.int64))
        ei = np.abs(got["I"].cpu().numpy() - R.morans_i(ref, nbr)[0]).max()
        ec = np.abs(got["C"].cpu().numpy() - Q.geary_c(ref, nbr)).max()
        print(name, kind, family, "max |I - oracle|", ei, "of", R.I_ATOL, "max |C - oracle|", ec, "of", Q.C_ATOL)
        assert ei <= R.I_ATOL and ec <= Q.C_ATOL


# --- 6. planted structure ----------------------------------------------------------------------------------------------------------

def test_planted_structure_has_the_smallest_p_values():
    from gpzoo.likelihoods import ResidualAutocorrPerm, ResidualGearyPerm, residual_autocorr
    from gpzoo.utilities import fdr_bh
    from torch.distributions import Normal
    c = R.planted_case()
    d = {k: _t(c[k]) for k in ("mean", "scale", "W", "V", "y", "theta")}
    nbr, perms = _t(c["nbr"], torch.int64), _t(Q.planted_perms(), torch.int32)
    planted = c["planted"]
    for kind, family in COMBOS:
        for mode, cls in (("moran", ResidualAutocorrPerm), ("geary", ResidualGearyPerm)):
            r = residual_autocorr([Normal(d["mean"], d["scale"])], [d["W"]], d["V"], d["y"], nbr,
                                  theta_pos=d["theta"] if family == "nb" else None, kind=kind, mode=mode, perms=perms)
            assert isinstance(r, cls) and r.n_perms == 199 and r.sims is None
            count, p = (r.n_ge, r.pval_greater) if mode == "moran" else (r.n_le, r.pval_less)
            count, p = count.cpu().numpy(), p.cpu().numpy()
            print(kind, family, mode, "planted p", p[planted], "smallest null p", p[~planted].min())
            assert (count[planted] == 0).all() and (p[planted] == 0.005).all()
            assert (p[~planted] >= 0.02).all()
            want = Q.planted_oracle(kind, family, mode)
            selected = np.flatnonzero((fdr_bh(torch.as_tensor(p)) <= 0.05).numpy())
            np.testing.assert_array_equal(selected, want["selected"])
            assert set(selected) >= set(np.flatnonzero(planted))


# --- 7. the model method ---------------------------------------------------------------------------------------------------------------

def test_the_model_method_with_the_new_keywords():
    """A small NSF over WSVGP, the construction of tests/test_residual_api._nsf with the variational parameters it leaves
    unset filled in as tests/test_hip_residual_autocorr._gp fills them, on the device (80 genes, 130 spots, 3 factors)."""
    from gpzoo.likelihoods import NSF, ResidualAutocorr, ResidualAutocorrPerm, ResidualGeary, ResidualGearyPerm
    g, X, y = TR._model_data()
    model = NSF(TR._gp(g, X), y.cpu(), L=TR.L_M)
    model.W = torch.nn.Parameter(torch.rand(TR.D_M, TR.L_M, generator=g))
    model = model.cuda()
    Dm = TR.D_M
    plain = model.residual_autocorr(X, y)
    assert isinstance(plain, ResidualAutocorr)
    r = model.residual_autocorr(X, y, n_perms=7, seed=3)
    assert isinstance(r, ResidualAutocorrPerm) and r.n_perms == 7 and r.sims is None
    assert r._fields[:6] == ResidualAutocorr._fields and all(torch.equal(a, b) for a, b in zip(r[:6], plain))
    again = model.residual_autocorr(X, y, n_perms=7, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(r[:7], again[:7])) and all(torch.equal(a, b) for a, b in zip(r[8:17], again[8:17]))
    assert ((r.n_ge + r.n_le) >= 7).all() and ((r.pval_sim > 0) & (r.pval_sim <= 1)).all()
    other = model.residual_autocorr(X, y, n_perms=7, seed=4)
    assert torch.equal(other.I, r.I) and not torch.equal(other.mean_sim, r.mean_sim)
    gy = model.residual_autocorr(X, y, n_perms=7, seed=3, mode="geary", return_sims=True)
    assert isinstance(gy, ResidualGearyPerm) and gy.sims.shape == (Dm, 7) and float(gy.expected) == 1.0
    assert torch.equal(gy.residual_mean, plain.residual_mean) and torch.equal(gy.residual_var, plain.residual_var)
    g0 = model.residual_autocorr(X, y, mode="geary")
    assert isinstance(g0, ResidualGeary) and torch.equal(g0.C, gy.C) and g0.variance.dim() == 0
    rnd = model.residual_autocorr(X, y, assumption="randomisation")
    assert isinstance(rnd, ResidualAutocorr) and rnd.variance.shape == rnd.z.shape == (Dm,) and torch.equal(rnd.I, plain.I)
    assert not torch.equal(rnd.variance, plain.variance.expand(Dm))
    both = model.residual_autocorr(X, y, mode="geary", assumption="randomisation", n_perms=7, seed=3)
    assert isinstance(both, ResidualGearyPerm) and both.variance.shape == (Dm,) and torch.equal(both.n_le, gy.n_le)
