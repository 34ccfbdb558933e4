#!/usr/bin/env python3
"""Time the residual autocorrelation entry (ops.residual_morans_i) on one MI355X next to the torch composition a user would
write, on the same inputs in the same process: the median of 30 rounds that alternate the candidates, after warm-up, on
synthetic counts with D = 17 702 genes, Lt = 20 factors, K = 6 neighbours, Pearson residuals, both families, at B = 7000 and
B = 39 694 spots, for dense counts and for a SparseCounts at 1 / 5 / 20 % density.

The yardstick is the composition, not the code under test.  It runs over gene chunks of the plan's ``slab_genes``:
``V * (W @ m)``, the residual, ``.T.contiguous()``, ``ops.morans_i`` -- on the dense counts, also where the entry reads the
SparseCounts.  Two parts are timed in the same rounds to show which bounds the entry: the residual pass alone
(``ops.count_residuals`` of all genes into one (B, D) array) and ``ops.morans_i`` alone on one ready slab (times n_slabs).

    python tools/residual_autocorr_step.py [--json FILE] [--quick]

``--quick`` runs B = 7000 at 5 % only."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402

D, LT, K = 17702, 20, 6
ROUNDS, WARM = 30, 2


def alternating_ms(fns: dict, rounds=ROUNDS, warm=WARM) -> dict:
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


def torch_composition(mean, scale, W, V, theta, y, nbr, chunk):
    """What a user composes: per gene chunk the (chunk, B) rate, the Pearson residual, its transpose, ops.morans_i."""
    m = torch.exp(mean + 0.5 * scale * scale)
    out = []
    for d0 in range(0, y.shape[0], chunk):
        mu = V * torch.matmul(W[d0:d0 + chunk], m)
        var = mu if theta is None else mu * (1.0 + mu / theta[d0:d0 + chunk, None])
        r = (y[d0:d0 + chunk] - mu) / torch.sqrt(var)
        out.append(ops.morans_i(r.T.contiguous(), nbr))
    return torch.cat(out)


def params(n, dev):
    g = torch.Generator().manual_seed(1)
    return ((0.3 * torch.randn(LT, n, generator=g)).to(dev), (0.2 + 0.3 * torch.rand(LT, n, generator=g)).to(dev),
            (torch.rand(D, LT, generator=g) + 0.05).to(dev), (0.5 + torch.rand(n, generator=g)).to(dev))


def main():
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    quick = "--quick" in args
    dev = torch.device("cuda")
    rows = []
    g = torch.Generator().manual_seed(2)
    theta = (0.5 + 20.0 * torch.rand(D, generator=g)).to(dev)
    for B in ((7000,) if quick else (7000, 39694)):
        p = params(B, dev)
        nbr = ops.spatial_knn(torch.rand(B, 2, generator=g, dtype=torch.float64).to(dev), K)
        plan = ops.residual_autocorr_plan(B, D, LT)
        slab = torch.randn(B, plan["slab_genes"], generator=torch.Generator(device=dev).manual_seed(3), device=dev)
        for density in ((0.05,) if quick else (0.01, 0.05, 0.20)):
            y = synthetic_counts(D, B, density, dev, seed=int(1000 * density))
            s = SparseCounts(y)
            for family, th in (("poisson", None), ("nb", theta)):
                rec = dict(B=B, D=D, Lt=LT, K=K, density=density, nnz=s.nnz, family=family, kind="pearson",
                           slab_genes=plan["slab_genes"], n_slabs=plan["n_slabs"], partials_MiB=plan["partials_bytes"] / 2 ** 20)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                ref = torch_composition(*p, th, y, nbr, plan["slab_genes"])
                torch.cuda.synchronize()
                rec["torch_peak_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                ms = alternating_ms({
                    "dense_ms": lambda: ops.residual_morans_i(*p, y, nbr, theta_pos=th),
                    "sparse_ms": lambda: ops.residual_morans_i(*p, s, nbr, theta_pos=th),
                    "torch_ms": lambda: torch_composition(*p, th, y, nbr, plan["slab_genes"]),
                    "residual_pass_dense_ms": lambda: ops.count_residuals(*p, y, theta_pos=th),
                    "residual_pass_sparse_ms": lambda: ops.count_residuals(*p, s, theta_pos=th),
                    "morans_i_one_slab_ms": lambda: ops.morans_i(slab, nbr),
                })
                rec.update(ms)
                rec["morans_i_all_slabs_ms"] = ms["morans_i_one_slab_ms"] * plan["n_slabs"]
                a = ops.residual_morans_i(*p, y, nbr, theta_pos=th)["I"]
                b = ops.residual_morans_i(*p, s, nbr, theta_pos=th)["I"]
                rec["max_abs_I_dense_minus_torch"] = float((a - ref).abs().max())
                rec["dense_equals_sparse_bits"] = bool(torch.equal(a, b))
                rows.append(rec)
                print(json.dumps(rec), flush=True)
            del y, s
            torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
