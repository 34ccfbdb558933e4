"""CPU: the cases, probes and fp64 oracle of tests/sparse_poisson_cases.py, SparseCounts on CPU tensors, and the host-side
contract of gpz_poisson_nsf_sparse (symbols, plan query, argument errors) -- nothing here needs a GPU."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import poisson_cases as PC
import sparse_poisson_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = SC.all_cases()
ENTRIES = ("gpz_poisson_nsf_sparse", "gpz_poisson_nsf_sparse_workspace_bytes", "gpz_poisson_nsf_sparse_plan")


# --- oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_sparse_oracle_equals_dense_reference(name, c):
    """The sparse formulas in fp64 against fp64 autograd of the dense formula: 1e-9 of the GPU tolerances."""
    for with_lgamma in (False, True):
        ref, got = SC.reference(c, with_lgamma), SC.sparse_reference(c, with_lgamma)
        assert abs(got["ll"] - ref["ll"]) <= 1e-9 * float(PC.tolerance(ref, "ll")), name
        for nm in PC.OUTPUTS:
            assert got[nm].shape == ref[nm].shape
            assert float(((got[nm] - ref[nm]).abs() / PC.tolerance(ref, nm)).max()) <= 1e-9, (name, nm)


def test_sparse_formulas_in_fp32_sit_far_inside_the_tolerances():
    """Why the project's Poisson tolerances need no loosening: plain fp32 torch on the same formulas."""
    c = SC.chunk_case()
    ref, got = SC.reference(c, True), SC.sparse_reference(c, True, dtype=torch.float32)
    assert abs(got["ll"] - ref["ll"]) <= 0.05 * float(PC.tolerance(ref, "ll"))
    for nm in PC.OUTPUTS:
        assert float(((got[nm] - ref[nm]).abs() / PC.tolerance(ref, nm)).max()) <= 0.05, nm


# --- probes and case list --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,c", [(n, c) for n, c in CASES if c["probes"]], ids=[n for n, c in CASES if c["probes"]])
def test_probes_are_sharp(name, c):
    v = SC.dense_view(c)
    assert len(v["probes"]) >= 1
    for (d, n, cnt), s in zip(v["probes"], PC.sharpness(v)):
        assert v["y"][d, n] == cnt
        assert min(s.values()) >= PC.SHARP_NEED, (name, d, n, cnt, s)


def test_case_list_contains_each_boundary():
    C_ = SC.chunk_length()
    assert C_ >= 2 and SC.plan(1037, 1037, 80, 20, 3)["spot_chunk"] == 0          # columns are not split
    c = SC.chunk_case()
    lens = {k: int((c["y"][g] != 0).sum()) for k, g in SC.CHUNK_GENES.items()}
    assert lens == {"C-1": C_ - 1, "C": C_, "C+1": C_ + 1, "2C+1": 2 * C_ + 1, "full": 1037}
    probes = {(d, n) for d, n, _ in c["probes"]}
    for g in SC.CHUNK_GENES.values():
        spots = torch.nonzero(c["y"][g]).reshape(-1).tolist()
        for lo in range(0, len(spots), C_):
            assert (g, spots[lo]) in probes and (g, spots[min(lo + C_, len(spots)) - 1]) in probes
    assert {(0, 0), (79, 1036)} <= probes
    col = SC.dense_column_case()
    assert SC.DENSE_COLUMN_SHAPE[1] == 2100 and bool((col["y"][:, SC.DENSE_COLUMN] != 0).all())
    # factor counts: both ends of a kernel instance and the largest; samples beyond the group the spot pass holds on chip
    pads = {s[2]: SC.plan(s[0], s[0], s[1], s[2], s[3])["factors_padded"] for s in SC.FACTOR_SHAPES}
    assert sorted(pads) == [1, 4, 5, 20, 63, 64] and pads[4] == 4 and pads[5] > 5 and pads[20] == 20 and pads[63] == pads[64] == 64
    assert [s[3] for s in SC.SAMPLE_SHAPES] == [1, 2, 20, 33]
    assert SC.plan(130, 130, 80, 7, 33)["samples_per_group"] < 33
    e = SC.empties_case()["y"]
    assert all(not e[d].any() for d in (0, 41, 79)) and all(not e[:, n].any() for n in (0, 66, 67, 129))
    assert int((SC.no_counts_case()["y"] != 0).sum()) == 0 and int((SC.one_count_case()["y"] != 0).sum()) == 1
    assert SC.single_case()["y"].shape == (1, 1)
    vals = SC.values_case()["y"]
    assert bool((vals >= 256).any()) and bool((vals != vals.round()).any())
    idx = SC.batch_indices()
    assert len(idx["B1"]) == 1 and len(idx["B70"]) == 70 and sorted(idx["perm"]) == list(range(1037))
    assert idx["B70"] != sorted(idx["B70"])
    for k, v in idx.items():
        assert len(set(v)) == len(v), k
    ye = SC.batch_case("empty_cols")
    assert all(not ye["y"][:, n].any() for n in SC.BATCH_EMPTY_COLS) and set(SC.BATCH_EMPTY_COLS) <= set(idx["empty_cols"])
    yh = SC.batch_case("hidden_gene")
    assert bool(yh["y"][SC.BATCH_HIDDEN_GENE].any()) and not SC.batch_dense(yh)[SC.BATCH_HIDDEN_GENE].any()
    for _, c in CASES:
        dens = float((c["y"] != 0).double().mean())
        assert dens <= 0.2 or c["y"].numel() == 1, dens


# --- SparseCounts on CPU tensors -------------------------------------------------------------------------------------

def _structure(s):
    return [getattr(s, k) for k in s._PARTS]


def _same(a, b):
    return a.shape == b.shape and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(_structure(a), _structure(b)))


def _dense():
    return SC.empties_case()["y"].float()


def test_sparse_counts_constructions_agree():
    from gpzoo_amd.likelihoods import SparseCounts
    y = _dense()
    D, N = y.shape
    ref = SparseCounts(y)
    assert ref.shape == (D, N) and ref.nnz == int((y != 0).sum()) and ref.device == y.device
    assert ref.col_ptr.dtype == torch.int64 and ref.col_gene.dtype == torch.int32 and ref.col_val.dtype == torch.float32
    assert ref.row_ptr.dtype == torch.int64 and ref.row_spot.dtype == torch.int32
    assert _same(ref, SparseCounts(y.to_sparse_csr())) and _same(ref, SparseCounts(y.to_sparse_csc()))
    assert _same(ref, SparseCounts(y.to_sparse())) and _same(ref, SparseCounts(ref))
    # COO with duplicates (a count split in two), explicit zeros and an unsorted order
    g, n = torch.nonzero(y, as_tuple=True)
    v = y[g, n]
    half = torch.floor(v / 2)
    ind = torch.cat([torch.stack([g, n]), torch.stack([g, n]), torch.tensor([[0, 5], [0, 7]])], dim=1)
    val = torch.cat([half, v - half, torch.zeros(2)])
    shuffle = torch.randperm(ind.shape[1], generator=torch.Generator().manual_seed(3))
    coo = torch.sparse_coo_tensor(ind[:, shuffle], val[shuffle], (D, N))
    assert _same(ref, SparseCounts(coo))
    # duck-typed CSR / CSC: what adata.X is, without scipy
    csr = y.to_sparse_csr()
    duck = types.SimpleNamespace(indptr=csr.crow_indices().numpy(), indices=csr.col_indices().numpy().astype("int32"),
                                 data=csr.values().numpy(), shape=(D, N), format="csr")
    assert _same(ref, SparseCounts(duck))
    csc = y.to_sparse_csc()
    duck = types.SimpleNamespace(indptr=csc.ccol_indices().tolist(), indices=csc.row_indices().tolist(),
                                 data=csc.values().tolist(), shape=(D, N), format="csc")
    assert _same(ref, SparseCounts(duck))
    with pytest.raises(TypeError):
        SparseCounts(types.SimpleNamespace(shape=(D, N), format="coo"))
    with pytest.raises(IndexError):
        SparseCounts(types.SimpleNamespace(indptr=[0, 1] + [1] * (D - 1), indices=[N], data=[1.0], shape=(D, N), format="csr"))


def test_sparse_counts_orders_and_round_trip():
    from gpzoo_amd.likelihoods import SparseCounts
    y = _dense()
    D, N = y.shape
    s = SparseCounts(y)
    assert torch.equal(s.to_dense(), y)
    spot = torch.repeat_interleave(torch.arange(N), torch.diff(s.col_ptr))
    gene = torch.repeat_interleave(torch.arange(D), torch.diff(s.row_ptr))
    assert int(s.col_ptr[-1]) == int(s.row_ptr[-1]) == s.nnz
    assert torch.equal(y[s.col_gene.long(), spot], s.col_val) and bool((s.col_val != 0).all())
    # by spot: genes ascending inside a spot; by gene: spots ascending inside a gene; row_perm maps one order onto the other
    key = spot * D + s.col_gene
    assert bool((key[1:] > key[:-1]).all())
    rkey = gene * N + s.row_spot
    assert bool((rkey[1:] > rkey[:-1]).all())
    perm = s.row_perm.long()
    assert sorted(perm.tolist()) == list(range(s.nnz))
    assert torch.equal(s.col_gene[perm].long(), gene) and torch.equal(spot[perm], s.row_spot.long())
    assert torch.equal(s.col_val[perm], y[gene, s.row_spot.long()])


def test_sparse_counts_batch_view():
    from gpzoo_amd.likelihoods import SparseCounts
    y = _dense()
    s = SparseCounts(y)
    idx = torch.tensor([129, 3, 66, 0, 77, 12])
    v = s[:, idx]
    assert v.shape == (y.shape[0], 6) and v.base is s and v.device == s.device
    assert torch.equal(v.to_dense(), y[:, idx]) and v.nnz == int((y[:, idx] != 0).sum())
    assert torch.equal(v.idx.long(), idx) and v.pos.dtype == torch.int32
    assert torch.equal(v.pos.long()[idx], torch.arange(6)) and int((v.pos >= 0).sum()) == 6
    assert torch.equal(s[:, torch.tensor([-1, 2], dtype=torch.int32)].to_dense(), y[:, [-1, 2]])
    for bad in (3, slice(None), (slice(None), 3), (slice(None), [1, 2]), (slice(0, 4), idx), (idx, slice(None)),
                (slice(None), idx.float()), (slice(None), idx.reshape(2, 3))):
        with pytest.raises(TypeError):
            s[bad]
    with pytest.raises(TypeError):
        v[:, torch.tensor([0])]
    for bad in (torch.tensor([1, 2, 1]), torch.tensor([0, 130]), torch.tensor([-131])):
        with pytest.raises(IndexError):
            s[:, bad]
    # inside a deferred_info block the check waits for the block's end
    from gpzoo_amd import ops
    with pytest.raises(IndexError):
        with ops.deferred_info():
            w = s[:, torch.tensor([5, 5])]
            assert w.shape == (y.shape[0], 2)


def test_non_fused_route_names_fused():
    from gpzoo_amd import utilities
    from gpzoo_amd.likelihoods import SparseCounts
    s = SparseCounts(_dense())
    model = types.SimpleNamespace(expected_loglik=None)
    for loop in (utilities.train, utilities.train_batched, utilities.train_hybrid, utilities.train_hybrid_batched):
        with pytest.raises(TypeError, match="fused=True"):
            loop(model, None, torch.zeros(130, 2), s, steps=1, fused=False)
    with pytest.raises(TypeError, match="fused=True"):
        utilities.train(types.SimpleNamespace(), None, torch.zeros(130, 2), s, steps=1)


# --- ABI -------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_and_bound():
    from gpzoo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpzoo_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.exported_symbols() and getattr(lib, name)
    assert lib.gpz_version() == 212


def test_plan_query():
    from gpzoo_amd import ops
    p = ops.poisson_nsf_sparse_plan(39694, 7000, 17702, 20, 3, 35_000_000)
    assert p["gene_chunk"] > 0 and p["factors_padded"] == 20 and p["samples_per_group"] == 3
    assert p["n_gene_chunks"] >= 17702 + 35_000_000 // p["gene_chunk"]
    # O(nnz E Lt + E Lt B + D Lt): nothing of D x B elements
    assert 0 < p["workspace_bytes"] < 4 * 17702 * 7000 // 20
    assert ops.poisson_nsf_sparse_plan(130, 130, 80, 64, 100, 0)["samples_per_group"] < 100
    for bad in ((0, 0, 80, 20, 3, 0), (130, 131, 80, 20, 3, 0), (130, 130, 0, 20, 3, 0), (130, 130, 80, 65, 3, 0),
                (130, 130, 80, 0, 3, 0), (130, 130, 80, 20, 0, 0), (130, 130, 80, 20, 3, -1), (-5, -5, 80, 20, 3, 0)):
        with pytest.raises(ValueError, match="gpz_poisson_nsf_sparse_plan"):
            ops.poisson_nsf_sparse_plan(*bad)


def _call(lib, over=None, ws_bytes=None, **shape):
    """gpz_poisson_nsf_sparse with host buffers as stand-ins: every case here must be refused before any launch."""
    s = dict(N=130, B=130, D=80, nnz=50, Lt=20, E=3)
    s.update(shape)
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)
    names = ("mean", "scale", "eps", "W", "V", "col_ptr", "col_gene", "col_val", "row_ptr", "row_spot", "row_perm", "idx", "pos")
    outs = ("loglik", "dmean", "dscale", "dW", "dV", "ws")
    a = {k: p for k in names + outs}
    a["idx"] = a["pos"] = None
    a.update(over or {})
    need = lib.gpz_poisson_nsf_sparse_workspace_bytes(s["N"], s["B"], s["D"], s["nnz"], s["Lt"], s["E"])
    rc = lib.gpz_poisson_nsf_sparse(*[a[k] for k in names], s["N"], s["B"], s["D"], s["nnz"], s["Lt"], s["E"], 1,
                                    *[a[k] for k in outs], need if ws_bytes is None else ws_bytes, None)
    return rc, lib.gpz_last_error().decode()


def test_argument_errors_before_any_launch():
    from gpzoo_amd import _lib
    lib = _lib.load()
    assert lib.gpz_poisson_nsf_sparse_workspace_bytes(130, 130, 80, 50, 20, 3) > 0
    for bad in ((130, 130, 80, 50, 65, 3), (130, 130, 80, 50, 0, 3), (-1, 130, 80, 50, 20, 3), (130, 130, -80, 50, 20, 3),
                (130, 130, 80, -1, 20, 3), (130, 0, 80, 50, 20, 3), (130, 130, 80, 50, 20, 0), (130, 200, 80, 50, 20, 3)):
        assert lib.gpz_poisson_nsf_sparse_workspace_bytes(*bad) == 0, bad
    refused = [dict(Lt=65), dict(Lt=0), dict(N=-1), dict(D=-80), dict(nnz=-1), dict(E=0), dict(B=0), dict(B=131),
               dict(B=70),                                            # a batch without idx / pos
               dict(ws_bytes=1024)]
    refused += [dict(over={k: None}) for k in ("mean", "scale", "eps", "W", "V", "col_ptr", "col_gene", "col_val", "row_ptr",
                                               "row_spot", "row_perm", "loglik", "dmean", "dscale", "dW", "dV", "ws")]
    buf = (C.c_char * 256)()
    odd = C.c_void_p((C.addressof(buf) + 63) // 64 * 64 + 4)
    refused += [dict(over={"W": odd}), dict(over={"ws": odd}), dict(over={"idx": odd}), dict(over={"pos": odd})]
    for kw in refused:
        rc, msg = _call(lib, **kw)
        assert rc < 0 and msg.startswith("gpz_poisson_nsf_sparse:"), (kw, rc, msg)
