#!/usr/bin/env python3
"""Time the permutation null of the residual autocorrelation (ops.residual_autocorr_perm) on one MI355X next to what could
be composed before it existed, on the same inputs in the same process: the arms alternate round by round, device events, the
median of 30 rounds after warm-up.  Synthetic counts with D = 17 702 genes, Lt = 20 factors, K = 6 neighbours, P = 100
permutations, Pearson residuals, the Poisson family, at B = 7000 and B = 39 694 spots, dense counts and a SparseCounts at
5 % density.

The yardstick is the composition, not the code under test: P calls of ``ops.residual_morans_i`` over tables relabelled with
torch indexing (T[pi] = pi[nbr]), which give the same statistic.  Each call forms the residuals again and rereads every
slab four times.  Timed in the same rounds: ``ops.residual_spatial_stats`` (the residual pass and the observed statistics,
which the entry runs once), so that the permutation pass alone is the entry minus it, and ``ops.morans_i`` on one ready slab
(times n_slabs: the README's figure for one Moran pass over all slabs).

    python tools/residual_perm_step.py [--json FILE] [--quick] [--rounds N] [--side-rounds N] [--perm-batches 4,8,32] [--existing]

``--quick`` runs B = 7000 only.  Geary's C and, with ``--perm-batches``, the entry at other batch sizes (dense counts) are
timed beside the main arms over ``--side-rounds`` rounds (5) of their own.  ``--existing`` times only the entries that existed before (``residual_morans_i``, ``gene_autocorr_perm_sparse``),
for a comparison of two builds of the library."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402

D, LT, K, P = 17702, 20, 6, 100
DENSITY = 0.05


def alternating_ms(fns: dict, rounds: int, warm: int = 1) -> dict:
    """Median milliseconds per candidate over ``rounds`` rounds, each round running every candidate once in turn."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in times.items()}


def synthetic_counts(D, N, density, dev, seed):
    """(D, N) fp32 counts on the device, built in column blocks so that no temporary is larger than the result."""
    g = torch.Generator(device=dev).manual_seed(seed)
    y = torch.empty((D, N), dtype=torch.float32, device=dev)
    for n0 in range(0, N, 4096):
        n1 = min(N, n0 + 4096)
        keep = torch.rand((D, n1 - n0), generator=g, device=dev) < density
        y[:, n0:n1] = (torch.poisson(torch.full((D, n1 - n0), 2.0, device=dev), generator=g) + 1.0) * keep
    return y


def params(n, dev):
    g = torch.Generator().manual_seed(1)
    return ((0.3 * torch.randn(LT, n, generator=g)).to(dev), (0.2 + 0.3 * torch.rand(LT, n, generator=g)).to(dev),
            (torch.rand(D, LT, generator=g) + 0.05).to(dev), (0.5 + torch.rand(n, generator=g)).to(dev))


def relabelled(nbr, pi):
    T = torch.empty_like(nbr)
    T[pi] = pi[nbr]
    return T


def yardstick(p, y, nbr, perms):
    """P calls of the entry that existed, each over a relabelled table; (D, P) simulated I."""
    return torch.stack([ops.residual_morans_i(*p, y, relabelled(nbr, pi))["I"] for pi in perms], dim=1)


def option(args, name, default=None):
    if name not in args:
        return default
    i = args.index(name)
    v = args[i + 1]
    del args[i:i + 2]
    return v


def main():
    args = sys.argv[1:]
    out = option(args, "--json")
    rounds = int(option(args, "--rounds", 30))
    side_rounds = int(option(args, "--side-rounds", 5))
    batches = [int(v) for v in option(args, "--perm-batches", "").split(",") if v]
    quick, existing = "--quick" in args, "--existing" in args
    dev = torch.device("cuda")
    rows = []
    g = torch.Generator().manual_seed(2)
    for B in ((7000,) if quick else (7000, 39694)):
        p = params(B, dev)
        nbr = ops.spatial_knn(torch.rand(B, 2, generator=g, dtype=torch.float64).to(dev), K)
        gp = torch.Generator(device=dev).manual_seed(4)
        perms = torch.stack([torch.randperm(B, generator=gp, device=dev) for _ in range(P)])
        y = synthetic_counts(D, B, DENSITY, dev, seed=int(1000 * DENSITY))
        s = SparseCounts(y)
        if existing:
            rec = dict(B=B, D=D, Lt=LT, K=K, P=P, density=DENSITY, nnz=s.nnz, arms="existing")
            rec.update(alternating_ms({
                "residual_morans_i_dense_ms": lambda: ops.residual_morans_i(*p, y, nbr),
                "residual_morans_i_sparse_ms": lambda: ops.residual_morans_i(*p, s, nbr),
                "gene_autocorr_perm_sparse_moran_ms": lambda: ops.gene_autocorr_perm_sparse(s, nbr, perms, stat="moran"),
                "gene_autocorr_perm_sparse_geary_ms": lambda: ops.gene_autocorr_perm_sparse(s, nbr, perms, stat="geary"),
            }, rounds))
            rows.append(rec)
            print(json.dumps(rec), flush=True)
            continue
        plan = ops.residual_autocorr_perm_plan(B, D, LT, K, P)
        slab = torch.randn(B, plan["slab_genes"], generator=torch.Generator(device=dev).manual_seed(3), device=dev)
        for counts, name in ((y, "dense"), (s, "sparse")):
            rec = dict(B=B, D=D, Lt=LT, K=K, P=P, counts=name, density=DENSITY, nnz=s.nnz, family="poisson", kind="pearson",
                       partials_MiB=plan["partials_bytes"] / 2 ** 20, **{k: plan[k] for k in ("slab_genes", "n_slabs", "perm_batch", "batches")})
            fns = {
                "entry_moran_ms": lambda c=counts: ops.residual_autocorr_perm(*p, c, nbr, perms),
                "yardstick_ms": lambda c=counts: yardstick(p, c, nbr, perms),
                "stats_ms": lambda c=counts: ops.residual_spatial_stats(*p, c, nbr),
                "residual_morans_i_ms": lambda c=counts: ops.residual_morans_i(*p, c, nbr),
                "morans_i_one_slab_ms": lambda: ops.morans_i(slab, nbr),
            }
            ms = alternating_ms(fns, rounds)
            # beside them, over ``--side-rounds`` rounds: Geary's C, and the entry at other batch sizes (dense counts)
            side = {"entry_geary_ms": lambda c=counts: ops.residual_autocorr_perm(*p, c, nbr, perms, stat="geary")}
            if name == "dense":
                for pb in batches:
                    side[f"entry_moran_batch{pb}_ms"] = lambda c=counts, pb=pb: ops.residual_autocorr_perm(*p, c, nbr, perms, perm_batch=pb)
            rec.update(alternating_ms(side, side_rounds))
            rec["side_rounds"] = side_rounds
            rec.update(ms)
            rec["ratio_entry_over_yardstick"] = ms["entry_moran_ms"] / ms["yardstick_ms"]
            rec["perm_pass_per_permutation_ms"] = (ms["entry_moran_ms"] - ms["stats_ms"]) / P
            rec["morans_i_all_slabs_ms"] = ms["morans_i_one_slab_ms"] * plan["n_slabs"]
            r, _ = ops.residual_autocorr_perm(*p, counts, nbr, perms, return_sims=True)
            ref = yardstick(p, counts, nbr, perms)
            rec["max_abs_sims_minus_yardstick"] = float((r.sims - ref).abs().max())
            rows.append(rec)
            print(json.dumps(rec), flush=True)
            del r, ref
        del y, s, slab
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
