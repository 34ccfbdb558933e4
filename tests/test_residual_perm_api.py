"""CPU: the surface of the residual statistics and permutation entries -- the C entries' declarations, bindings and host-side
refusals, the plan query and what its scratch holds, the new keywords of ``residual_autocorr`` on every count model, the
result types and their re-exports, and the refusals that need no device."""
import ctypes as C
import inspect

import pytest
import torch

import test_residual_api as TA

ENTRIES = ("gpz_residual_spatial_stats", "gpz_residual_spatial_stats_sparse", "gpz_residual_autocorr_perm",
           "gpz_residual_autocorr_perm_sparse")
NEW_SYMBOLS = ENTRIES + ("gpz_residual_autocorr_perm_plan",)
_args = TA._args


def test_new_entries_are_declared_exported_and_bound():
    from gpzoo_amd import _lib, build, ops
    hdr = TA.header()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][1]) == len(_args(name)), name
    assert lib.gpz_version() == 212 and "#define GPZ_VERSION 212" in hdr
    comment = hdr[hdr.index("Additions under version 212"):hdr.index("#ifndef GPZOO_HIP_H")]
    assert all(n in comment for n in NEW_SYMBOLS)
    assert "geary_expr.h" not in hdr                                       # the header that no longer exists is not named
    assert all(callable(getattr(ops, n)) for n in ("residual_spatial_stats", "residual_autocorr_perm", "residual_autocorr_perm_plan"))
    # the passes are spatial_stats.hip's, reached through moran_pass.h; the relabel kernel stays in moran_perm.hip, once
    stats = open(build.CSRC + "/spatial_stats.hip").read()
    perm = open(build.CSRC + "/moran_perm.hip").read()
    resid = open(build.CSRC + "/residual.hip").read()
    assert "void rp_rows" in stats and "void rp_rows" not in resid and "moran_slab_perm_run" in resid
    assert "void mp_relabel_kernel" in perm and "mp_relabel_kernel" not in stats and "mp_relabel_kernel" not in resid
    assert '#include "moran_pass.h"' in perm and "relabel_tables" in stats
    assert "atomicAdd" not in stats and "atomicAdd" not in resid           # no floating-point atomics (none at all there)
    assert build.SOURCE_FLAGS["spatial_stats.hip"] == ["-ffp-contract=off"] == build.SOURCE_FLAGS["moran_perm.hip"]


def test_the_arguments_are_those_of_the_moran_entries_plus_the_new_ones():
    hdr = TA.header()
    for name in ENTRIES:
        a = _args(name)
        assert a[-3:] == ["partials", "partials_bytes", "stream"] and "ws" not in a and "ws_bytes" not in a
        assert f"{name}_workspace_bytes" not in hdr
    moran, moran_s = _args("gpz_residual_morans_i"), _args("gpz_residual_morans_i_sparse")
    cut = moran.index("I")
    assert _args("gpz_residual_spatial_stats") == moran[:cut] + ["I", "C", "res_mean", "res_var", "kurtosis", "info"] + moran[-3:]
    assert (_args("gpz_residual_spatial_stats_sparse")
            == moran_s[:moran_s.index("I")] + ["I", "C", "res_mean", "res_var", "kurtosis", "info"] + moran_s[-3:])
    tail = ["P", "stat", "perm_batch", "value", "n_ge", "n_le", "sim_mean", "sim_m2", "sims", "res_mean", "res_var", "kurtosis",
            "info", "partials", "partials_bytes", "stream"]
    for name, base in (("gpz_residual_autocorr_perm", moran), ("gpz_residual_autocorr_perm_sparse", moran_s)):
        a, k = _args(name), base.index("nbr") + 1
        assert a[:k] == base[:k] and a[k] == "perms" and a[k + 1:a.index("P")] == base[k:base.index("I")] and a[a.index("P"):] == tail
    assert _args("gpz_residual_autocorr_perm_plan") == ["B", "D", "Lt", "K", "P", "nnz", "slab_genes_wanted", "perm_batch_wanted",
                                                        "slab_genes", "n_slabs", "perm_batch", "batches", "partials_bytes"]
    import scratch_cases as S
    assert not set(NEW_SYMBOLS) & S.header_entries_with_workspace(hdr)


def test_plan_query_needs_no_device_and_bounds_its_scratch():
    from gpzoo_amd import ops
    p = ops.residual_autocorr_perm_plan(39694, 17702, 20, 6, 100)
    assert set(p) == {"slab_genes", "n_slabs", "perm_batch", "batches", "partials_bytes"}
    for B, D, K, P in ((39694, 17702, 6, 100), (7000, 17702, 6, 100), (4099, 3000, 32, 19), (600, 130, 6, 5), (7, 5, 2, 5040),
                       (2_000_000, 500, 32, 100)):
        base = ops.residual_autocorr_plan(B, D, 20)
        for want in (0, 1, 3, 32):
            p = ops.residual_autocorr_perm_plan(B, D, 20, K, P, 0, 0, want)
            sg, pb, chunks = p["slab_genes"], p["perm_batch"], -(-B // 256)
            assert (sg, p["n_slabs"]) == (base["slab_genes"], base["n_slabs"])       # the slabs of the Moran entries
            if want:
                assert pb == min(want, P)
            else:
                assert 1 <= pb <= min(32, P) and (pb == 1 or 4 * B * K * pb <= 256 << 20)   # a batch's tables within 256 MiB
                assert pb == min(16, P, max(1, (256 << 20) // (4 * B * K)))
            assert p["batches"] == -(-P // pb)
            # the slab, plus O(B Lt) factors, 40 bytes per (chunk, column) of the wide pass and its means, plus per
            # permutation of a batch 4 B (K + 1) table bytes and 8 bytes per (chunk, column); nothing of D x B or P x D
            fixed = 4 * B * sg + 4 * 21 * (B + 64) + (40 * chunks + 8 + 24) * sg
            assert 4 * B * sg <= p["partials_bytes"] <= fixed + pb * (4 * B * (K + 1) + 8 * chunks * sg) + 16384
        assert ops.residual_autocorr_perm_plan(B, D, 20, K, P, 10 ** 9)["partials_bytes"] == ops.residual_autocorr_perm_plan(B, D, 20, K, P)["partials_bytes"]
    assert ops.residual_autocorr_perm_plan(600, 130, 5, 6, 19, 0, 64)["n_slabs"] == 3
    # P = 0: what the stats entries need -- no tables, no permutations' partial sums
    for B, D in ((39694, 17702), (600, 130), (7, 5)):
        p0, p1 = ops.residual_autocorr_perm_plan(B, D, 20, 2, 0), ops.residual_autocorr_perm_plan(B, D, 20, 2, 1)
        assert (p0["perm_batch"], p0["batches"]) == (0, 0) and p0["slab_genes"] == p1["slab_genes"]
        sg, chunks = p0["slab_genes"], -(-B // 256)
        assert ops.residual_autocorr_plan(B, D, 20)["partials_bytes"] < p0["partials_bytes"] < p1["partials_bytes"]
        assert p0["partials_bytes"] <= 4 * B * sg + 4 * 21 * (B + 64) + (40 * chunks + 8) * sg + 8192
    # gpz_residual_morans_i_plan is as it was: the new scratch is asked of the new query alone
    assert ops.residual_autocorr_plan(600, 130, 5)["partials_bytes"] < ops.residual_autocorr_perm_plan(600, 130, 5, 6, 1)["partials_bytes"]
    for bad in ((0, 1, 1, 1, 1), (5, 0, 1, 1, 1), (5, 1, 0, 1, 1), (5, 1, 65, 1, 1), (5, 1, 1, 0, 1), (5, 1, 1, 33, 1), (5, 1, 1, 5, 1),
                (5, 1, 1, 1, -1), (5, 1, 1, 1, 1 << 31), (5, 1, 1, 1, 1, -1), (5, 1, 1, 1, 1, 0, 32), (5, 1, 1, 1, 1, 0, 0, 33),
                (5, 1, 1, 1, 1, 0, 0, -1)):
        with pytest.raises(ValueError):
            ops.residual_autocorr_perm_plan(*bad)


def test_bad_arguments_are_refused_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 32768)()                       # host memory stands in for device memory: nothing is launched
    base = (C.addressof(buf) + 15) & ~15
    p = lambda off=0: C.c_void_p(base + off)  # noqa: E731
    inp = [p(256 * i) for i in range(9)]             # mean, scale, W, V, theta, y, genes, nbr, perms
    souts = [p(4096 + 256 * i) for i in range(6)]    # I, C, res_mean, res_var, kurtosis, info
    pouts = [p(8192 + 256 * i) for i in range(10)]   # value, n_ge, n_le, sim_mean, sim_m2, sims, res_mean, res_var, kurtosis, info
    rows = [p(12288 + 256 * i) for i in range(4)]
    scratch = p(16384)

    def stats(inp=inp, B=10, K=2, slab=0, outs=souts, scratch=scratch, nbytes=1 << 30, kind=0):
        return lib.gpz_residual_spatial_stats(*inp[:8], B, 4, 4, 3, K, 1, kind, 1, slab, *outs, scratch, nbytes, None)

    def perm(inp=inp, B=10, K=2, slab=0, P=5, stat=0, pb=0, outs=pouts, scratch=scratch, nbytes=1 << 30):
        return lib.gpz_residual_autocorr_perm(*inp, B, 4, 4, 3, K, 1, 0, 1, slab, P, stat, pb, *outs, scratch, nbytes, None)

    def perm_sparse(rows=rows, nnz=5, stat=1, P=5):
        return lib.gpz_residual_autocorr_perm_sparse(*inp[:5], *rows, *inp[6:], 10, 4, nnz, 4, 3, 2, 1, 0, 1, 0, P, stat, 0, *pouts, scratch,
                                                     1 << 30, None)

    def stats_sparse(rows=rows, nnz=5):
        return lib.gpz_residual_spatial_stats_sparse(*inp[:5], *rows, inp[6], inp[7], 10, 4, nnz, 4, 3, 2, 1, 0, 1, 0, *souts, scratch, 1 << 30,
                                                     None)
    err = lib.gpz_last_error
    for run, who, n_in, outs, key in ((stats, b"gpz_residual_spatial_stats: ", 8, souts, "outs"),
                                      (perm, b"gpz_residual_autocorr_perm: ", 9, pouts, "outs")):
        for i in [j for j in range(n_in) if j not in (4, 6)]:                    # theta and genes have refusals of their own
            assert run(inp=inp[:i] + [None] + inp[i + 1:]) < 0 and who + b"null pointer" in err(), (who, i)
        for i in range(len(outs)):
            if outs is pouts and i == 5:
                continue                                                         # sims may be NULL
            assert run(**{key: outs[:i] + [None] + outs[i + 1:]}) < 0 and who + b"null pointer" in err(), (who, i)
        assert run(scratch=None) < 0 and who + b"null pointer" in err()
        for K in (0, -1, 33, 10):
            assert run(K=K) < 0 and who in err() and b"neighbours" in err(), K
        assert run(B=3, K=3) < 0 and b"neighbours" in err()
        for slab in (1, 63, 100, -64):
            assert run(slab=slab) < 0 and who in err() and b"multiple of 64" in err()
        assert run(scratch=p(16388)) < 0 and b"16-byte aligned" in err()
        assert run(nbytes=8) < 0 and who in err() and b"partials too small" in err()
        assert run(inp=inp[:4] + [None] + inp[5:]) < 0 and b"needs theta" in err()
    assert stats(kind=2) < 0 and b"kind 2 unknown" in err()
    who = b"gpz_residual_autocorr_perm: "
    for P in (0, -3, 1 << 31):
        assert perm(P=P) < 0 and who in err() and b"permutations unsupported" in err()
    for stat in (-1, 2):
        assert perm(stat=stat) < 0 and who in err() and b"stat" in err() and b"unknown" in err()
    for pb in (-1, 33):
        assert perm(pb=pb) < 0 and who in err() and b"perm_batch" in err()
    assert perm(outs=pouts[:5] + [None] + pouts[6:], nbytes=8) < 0 and b"partials too small" in err()     # sims NULL passes the checks
    who = b"gpz_residual_autocorr_perm_sparse: "
    assert perm_sparse(rows=[None] + rows[1:]) < 0 and who + b"null pointer (counts)" in err()
    assert perm_sparse(rows=[rows[0], None] + rows[2:]) < 0 and who + b"null pointer (non-zeros)" in err()
    assert perm_sparse(nnz=1 << 31) < 0 and b"32 bits" in err()
    assert perm_sparse(stat=2) < 0 and who in err() and b"unknown" in err()
    assert perm_sparse(P=0) < 0 and who in err()
    assert stats_sparse(rows=[None] + rows[1:]) < 0 and b"gpz_residual_spatial_stats_sparse: null pointer (counts)" in err()
    assert stats_sparse(nnz=-1) < 0 and b"bad extents" in err()


def test_ops_refusals_come_before_any_device_work():
    from gpzoo.likelihoods import SparseCounts
    from gpzoo_amd import ops
    c = TA._case()
    a = (c["mean"], c["scale"], c["W"], c["V"])
    nbr = torch.stack([(torch.arange(13) + k + 1) % 13 for k in range(3)], dim=1)
    perms = torch.stack([torch.randperm(13) for _ in range(4)])
    sc = SparseCounts(c["y"])
    for bad, match in ((sc[:, torch.tensor([0, 2, 5])], "a view"), (sc.T, "obs x feat")):
        with pytest.raises(TypeError, match=match):
            ops.residual_spatial_stats(*a, bad, nbr)
        with pytest.raises(TypeError, match=match):
            ops.residual_autocorr_perm(*a, bad, nbr, perms)
    for stat in ("getis", 0, None):
        with pytest.raises(ValueError, match="stat"):
            ops.residual_autocorr_perm(*a, c["y"], nbr, perms, stat=stat)
    for bad in (perms[:, :12], perms.float(), perms[:0], perms[0], perms.bool()):
        with pytest.raises(ValueError, match="perms must be"):
            ops.residual_autocorr_perm(*a, c["y"], nbr, bad)
    for pb in (-1, 1.5, True, 33):
        with pytest.raises(ValueError, match="perm_batch"):
            ops.residual_autocorr_perm(*a, c["y"], nbr, perms, perm_batch=pb)
    for call in (lambda n, **k: ops.residual_spatial_stats(*a, c["y"], n, **k), lambda n, **k: ops.residual_autocorr_perm(*a, c["y"], n, perms, **k)):
        with pytest.raises(ValueError, match="nbr"):
            call(nbr[:12])
        with pytest.raises(ValueError, match="nbr"):
            call(nbr.float())
        with pytest.raises(ValueError, match="neighbours"):
            call(torch.zeros(13, 33, dtype=torch.int64))
        with pytest.raises(ValueError, match="neighbours"):
            call(torch.zeros(13, 13, dtype=torch.int64))
        with pytest.raises(ValueError, match="kind"):
            call(nbr, kind="anscombe")
        for slab in (1, 100, -64, 64.5):
            with pytest.raises(ValueError, match="slab_genes"):
                call(nbr, slab_genes=slab)
    # whole CPU inputs pass every check and stop at the device
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.residual_spatial_stats(*a, sc, nbr, kind="deviance", slab_genes=64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.residual_autocorr_perm(*a, c["y"], nbr, perms, theta_pos=c["theta"], stat="geary", return_sims=True, perm_batch=3)
    sig = inspect.signature(ops.residual_autocorr_perm)
    for k, default in (("stat", "moran"), ("return_sims", False), ("perm_batch", 0), ("slab_genes", 0)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == default
    assert list(inspect.signature(ops.residual_spatial_stats).parameters) == list(inspect.signature(ops.residual_morans_i).parameters)
    assert list(inspect.signature(ops.residual_autocorr_perm_plan).parameters) == ["B", "D", "Lt", "K", "P", "nnz", "slab_genes", "perm_batch"]


NEW_KEYWORDS = (("mode", "moran"), ("assumption", "normality"), ("n_perms", None), ("seed", 0), ("perms", None), ("return_sims", False))


def test_keywords_result_types_and_reexports():
    import gpzoo.likelihoods as li
    import gpzoo.utilities as ut
    import gpzoo_amd.likelihoods as ali
    for name in ("ResidualGeary", "ResidualAutocorrPerm", "ResidualGearyPerm", "ResidualAutocorr", "residual_autocorr"):
        assert getattr(li, name) is getattr(ali, name)
    base = ("expected", "variance", "z", "residual_mean", "residual_var")
    assert li.ResidualAutocorr._fields == ("I",) + base                                     # the six fields, as before
    assert li.ResidualGeary._fields == ("C",) + base + ("residual_kurtosis",)
    eleven = ut.GeneAutocorrPerm._fields[4:]
    assert len(eleven) == 11 and eleven == ut.GeneGearyPerm._fields[4:]
    assert li.ResidualAutocorrPerm._fields == ("I",) + base + ("residual_kurtosis",) + eleven
    assert li.ResidualGearyPerm._fields == li.ResidualGeary._fields + eleven
    sigs = [inspect.signature(li.residual_autocorr)]
    for cls in (li.NSF2, li.NSF, li.MGGP_NSF, li.Hybrid_NSF2, li.Hybrid_NSF_Exact, li.Hybrid_NSF):
        sigs.append(inspect.signature(cls.residual_autocorr))
        doc = " ".join(cls.residual_autocorr.__doc__.split())
        assert "standardised by the model's own variance" in doc and "n_perms" in doc
    for s in sigs:
        for k, default in NEW_KEYWORDS:
            assert s.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and s.parameters[k].default == default
    for cls in (li.PNMF, li.RSF, li.FA):
        assert not hasattr(cls, "residual_autocorr")
    doc = " ".join(li.residual_autocorr.__doc__.split())
    for phrase in ("normal approximation", "degrees of freedom", "not a calibrated test", "exact for exchangeable residuals",
                   "approximately exchangeable", "still ignores the degrees of freedom", "a mathematical tie may fall either way",
                   "for Geary ``pval_less``"):
        assert phrase in doc, phrase
    # the helpers are utilities', not copies
    src = inspect.getsource(ali)
    assert "def _perm_fields" not in src and "def _autocorr_perms" not in src and "def _autocorr_moments" not in src


def test_the_refusals_of_the_new_keywords_need_no_device():
    from torch.distributions import Normal
    import gpzoo.likelihoods as li
    c = TA._case()
    qF, W = [Normal(c["mean"], c["scale"] + 0.1)], [c["W"]]
    nbr = torch.stack([(torch.arange(13) + k + 1) % 13 for k in range(3)], dim=1)
    perms = torch.stack([torch.randperm(13) for _ in range(4)])
    model, X, y = TA._nsf()

    def free(**kw):
        return li.residual_autocorr(qF, W, c["V"], c["y"], nbr, **kw)

    def method(**kw):
        return model.residual_autocorr(X, y, **kw)
    for call in (free, method):
        with pytest.raises(ValueError, match="n_perms and perms exclude each other"):
            call(n_perms=3, perms=perms)
        for bad in ("getis", None, 0):
            with pytest.raises(ValueError, match="mode"):
                call(mode=bad)
        for bad in ("normal", None):
            with pytest.raises(ValueError, match="assumption"):
                call(assumption=bad)
        for bad in (0, -2, 2.5, True):
            with pytest.raises(ValueError, match="n_perms"):
                call(n_perms=bad)
        with pytest.raises(ValueError, match="perms must be"):
            call(perms=perms[:, :12])
    small = torch.tensor([[1, 2], [2, 0], [0, 1]])
    with pytest.raises(ValueError, match="needs B >= 4"):
        li.residual_autocorr([Normal(c["mean"][:, :3], c["scale"][:, :3] + 0.1)], W, c["V"][:3], c["y"][:, :3], small[:, :1],
                             assumption="randomisation")
    with pytest.raises(ValueError, match="needs B >= 4"):
        model.residual_autocorr(X[:3], y[:, :3], idx=torch.arange(3), assumption="randomisation")
