#!/usr/bin/env python3
"""Time the Gaussian residual autocorrelation entries (ops.gaussian_residual_stats, ops.gaussian_residual_autocorr_perm) on one
MI355X next to what could be composed before they existed, on the same inputs in the same process: the arms alternate round
by round, device events, the median over the rounds after warm-up.  Synthetic log-normalised expression with D = 17 702
genes, Lt = 20 factors, K = 6 neighbours at B = 7000 and B = 39 694 spots; the data dense, and a whole SparseExpression at
1 / 5 / 20 % density; kinds "pearson" and "predictive"; without permutations and with P = 100.

The yardstick is the composition, not the code under test: per chunk of the plan's ``slab_genes`` genes
``((y - b[:, None] - W @ m) / den).T.contiguous()`` in torch and ``ops.spatial_stats`` on the chunk; with permutations, P
more such passes per chunk over tables relabelled with torch indexing (T[pi] = pi[nbr]).  It needs the dense array (the
5 % data densified: the library had no way to form residuals from a SparseExpression), so the sparse arms are set against
the same dense yardstick.  Its peak temporaries are ``torch.cuda.max_memory_allocated`` over one pass, above what was
allocated before it.

    python tools/gaussian_residual_step.py [--json FILE] [--quick] [--rounds N] [--perm-rounds N] [--densities 0.01,0.05,0.2]
                                           [--count-entries]

``--quick`` runs B = 7000 only.  The permutation arms run ``--perm-rounds`` rounds (3): one round of the yardstick is P
passes.  ``--count-entries`` times only ``ops.residual_morans_i`` on dense counts, for a comparison of two builds of the
library (the count kernels are not meant to move)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts, SparseExpression  # noqa: E402

D, LT, K, P = 17702, 20, 6, 100


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


def synthetic_values(D, N, density, dev, seed):
    """(D, N) fp32 log1p of counts on the device with about ``density`` of the entries non-zero, built in column blocks."""
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.empty((D, N), dtype=torch.float32, device=dev)
    for n0 in range(0, N, 4096):
        n1 = min(N, n0 + 4096)
        keep = torch.rand((D, n1 - n0), generator=g, device=dev) < density
        v[:, n0:n1] = torch.log1p(torch.poisson(torch.full((D, n1 - n0), 2.0, device=dev), generator=g) + 1.0) * keep
    return v


def expression(density, B, dev):
    v = synthetic_values(D, B, density, dev, seed=int(1000 * density))
    expr = SparseExpression(SparseCounts(v), v.double().mean(dim=1))
    del v
    return expr


def params(n, dev):
    g = torch.Generator().manual_seed(1)
    return ((0.3 * torch.randn(LT, n, generator=g)).to(dev), (0.2 + 0.3 * torch.rand(LT, n, generator=g)).to(dev),
            (0.3 * torch.randn(D, LT, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev),
            (0.2 + 0.8 * torch.rand(D, generator=g)).to(dev))


def relabelled(nbr, pi):
    T = torch.empty_like(nbr)
    T[pi] = pi[nbr]
    return T


def yardstick(p, y, nbr, kind, slab_genes, perms=None):
    """What could be composed before: (I (D,), simulated I (D, P) or None)."""
    mean, scale, W, b, sd = p
    obs, sims = [], []
    for g0 in range(0, D, slab_genes):
        g1 = min(D, g0 + slab_genes)
        den = sd[g0:g1, None] if kind == "pearson" else torch.sqrt(sd[g0:g1, None] ** 2 + (W[g0:g1] ** 2) @ (scale ** 2))
        r = ((y[g0:g1] - b[g0:g1, None] - W[g0:g1] @ mean) / den).T.contiguous()
        obs.append(ops.spatial_stats(r, nbr).I)
        if perms is not None:
            sims.append(torch.stack([ops.spatial_stats(r, relabelled(nbr, pi)).I for pi in perms], dim=1))
    return torch.cat(obs), (torch.cat(sims) if sims else None)


def peak_temporaries_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def option(args, name, default=None):
    if name not in args:
        return default
    i = args.index(name)
    v = args[i + 1]
    del args[i:i + 2]
    return v


def count_entries(B, dev, rounds, nbr):
    """``ops.residual_morans_i`` on dense counts: the entry whose kernels the Gaussian family must not move."""
    g = torch.Generator().manual_seed(1)
    p = ((0.3 * torch.randn(LT, B, generator=g)).to(dev), (0.2 + 0.3 * torch.rand(LT, B, generator=g)).to(dev),
         (torch.rand(D, LT, generator=g) + 0.05).to(dev), (0.5 + torch.rand(B, generator=g)).to(dev))
    y = torch.expm1(synthetic_values(D, B, 0.05, dev, seed=50)).round()
    rec = dict(B=B, D=D, Lt=LT, K=K, arms="count entries")
    rec.update(alternating_ms({"residual_morans_i_dense_ms": lambda: ops.residual_morans_i(*p, y, nbr)}, rounds, warm=3))
    return rec


def main():
    args = sys.argv[1:]
    out = option(args, "--json")
    rounds = int(option(args, "--rounds", 30))
    perm_rounds = int(option(args, "--perm-rounds", 3))
    densities = [float(v) for v in option(args, "--densities", "0.01,0.05,0.2").split(",") if v]
    quick, counts_only = "--quick" in args, "--count-entries" in args
    dev = torch.device("cuda")
    rows = []
    g = torch.Generator().manual_seed(2)
    for B in ((7000,) if quick else (7000, 39694)):
        nbr = ops.spatial_knn(torch.rand(B, 2, generator=g, dtype=torch.float64).to(dev), K)
        if counts_only:
            rows.append(count_entries(B, dev, rounds, nbr))
            print(json.dumps(rows[-1]), flush=True)
            continue
        p = params(B, dev)
        gp = torch.Generator(device=dev).manual_seed(4)
        perms = torch.stack([torch.randperm(B, generator=gp, device=dev) for _ in range(P)])
        plan = ops.gaussian_residual_plan(B, D, LT, K, P)
        dense = expression(0.05, B, dev).to_dense()
        for kind in ("pearson", "predictive"):
            base = dict(B=B, D=D, Lt=LT, K=K, P=P, kind=kind, partials_MiB=plan["partials_bytes"] / 2 ** 20,
                        **{k: plan[k] for k in ("slab_genes", "n_slabs", "perm_batch", "batches")})
            ref_I, ref_sims = yardstick(p, dense, nbr, kind, plan["slab_genes"], perms[:3])
            for name, density in [("dense", None)] + [(f"sparse {100 * d:g} %", d) for d in densities]:
                data = dense if density is None else expression(density, B, dev)
                rec = dict(base, data=name, nnz=None if density is None else data.nnz)
                fns = {"entry_stats_ms": lambda: ops.gaussian_residual_stats(*p, data, nbr, kind=kind)}
                if density is None:
                    fns["yardstick_stats_ms"] = lambda: yardstick(p, dense, nbr, kind, plan["slab_genes"])
                rec.update(alternating_ms(fns, rounds))
                fns = {"entry_perm_ms": lambda: ops.gaussian_residual_autocorr_perm(*p, data, nbr, perms, kind=kind)}
                if density is None:
                    fns["yardstick_perm_ms"] = lambda: yardstick(p, dense, nbr, kind, plan["slab_genes"], perms)
                    rec["yardstick_peak_temporaries_MiB"] = peak_temporaries_mib(fns["yardstick_perm_ms"])
                rec.update(alternating_ms(fns, perm_rounds))
                rec["perm_rounds"], rec["rounds"] = perm_rounds, rounds
                if density is None or density == 0.05:         # the same data: against the composition's numbers
                    got = ops.gaussian_residual_stats(*p, data, nbr, kind=kind)["I"]
                    r, _ = ops.gaussian_residual_autocorr_perm(*p, data, nbr, perms[:3], kind=kind, return_sims=True)
                    rec["max_abs_I_minus_yardstick"] = float((got - ref_I).abs().max())
                    rec["max_abs_sims_minus_yardstick"] = float((r.sims - ref_sims).abs().max())
                rows.append(rec)
                print(json.dumps(rec), flush=True)
                del data
                torch.cuda.empty_cache()
        del dense
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
