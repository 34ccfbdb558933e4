#!/usr/bin/env python3
"""Time the sparse-count KL NMF iteration (gpz_nmf_kl_sparse_update) next to the dense one (gpz_nmf_kl_update) on the same
matrix in the same process, fp32, one GPU:

  iteration   X 40 000 x 2 000, L = 20, at 1 %, 5 % and 20 % non-zeros: the two entries are called in alternation, 30 timed
              calls of 20 iterations each after warm-up, device events, the median over the calls divided by 20; a call of
              ONE iteration (which carries the sparse entry's per-call transpose of H and chunk list) is reported beside it
  slideseq    the sparse iteration alone at 39 694 x 17 702, L = 20, 5 % (the dense X would be 2.8 GB and is never built:
              the counts are drawn block by block and kept as their non-zeros)
  end_to_end  regularized_nmf(init='nndsvd', max_iter=200, tol=0) at the first shape from a dense CUDA tensor and from
              counts.T: wall time up to the returned numpy arrays, how much of it is initialize_nmf, the bytes each form
              of the counts holds on the device and the peak device memory of each run

    python tools/sparse_nmf_step.py [iteration] [slideseq] [end_to_end] [--json FILE] [--once DENSITY]

``--once`` runs 20 sparse and 20 dense iterations at one density of the first shape and nothing else (for a profiler)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpzoo_amd import _lib, nmf, ops  # noqa: E402
from gpzoo_amd.likelihoods import SparseCounts  # noqa: E402

N1, D1, L = 40_000, 2_000, 20
NS, DS = 39_694, 17_702
DENSITIES = (0.01, 0.05, 0.20)
REPS, WARM, ITERS = 30, 3, 20


def sparse_counts(D, N, density, dev, seed, dense=False):
    """SparseCounts (D, N) of Poisson(2) + 1 where a uniform draw falls below ``density``, drawn in blocks of 2048 spots so
    that nothing of D x N elements exists unless ``dense`` asks for the array as well."""
    g = torch.Generator(device=dev).manual_seed(seed)
    gene, spot, val = [], [], []
    y = torch.empty((D, N), dtype=torch.float32, device=dev) if dense else None
    for n0 in range(0, N, 2048):
        n1 = min(N, n0 + 2048)
        keep = torch.rand((D, n1 - n0), generator=g, device=dev) < density
        block = (torch.poisson(torch.full((D, n1 - n0), 2.0, device=dev), generator=g) + 1.0) * keep
        d, n = torch.nonzero(block, as_tuple=True)
        gene.append(d); spot.append(n + n0); val.append(block[d, n])
        if dense:
            y[:, n0:n1] = block
    coo = torch.sparse_coo_tensor(torch.stack([torch.cat(gene), torch.cat(spot)]), torch.cat(val), (D, N))
    return SparseCounts(coo), y


def held_bytes(s):
    return sum(getattr(s, k).numel() * getattr(s, k).element_size() for k in s._PARTS)


def start(N, D, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N, L, generator=g) + 0.05).to(dev), (torch.rand(L, D, generator=g) + 0.05).to(dev)


class Entries:
    """The two library entries on preallocated factors (no clone, no Python between the call and the launch)."""

    def __init__(self, counts, X, dev):
        self.lib, self.c, self.X, self.dev = _lib.load(), counts, X, dev
        self.D, self.N = counts.shape
        self.ptrs = [C.c_void_p(getattr(counts, k).data_ptr()) for k in counts._PARTS]
        self.nb_s = self.lib.gpz_nmf_kl_sparse_workspace_bytes(self.N, self.D, counts.nnz, L, _lib.GPZ_F32)
        self.ws_s = torch.empty(self.nb_s, dtype=torch.uint8, device=dev)
        if X is not None:
            self.nb_d = self.lib.gpz_nmf_kl_workspace_bytes(self.N, self.D, L, _lib.GPZ_F32)
            self.ws_d = torch.empty(self.nb_d, dtype=torch.uint8, device=dev)
        self.reset()

    def reset(self):
        self.Ws, self.Hs = start(self.N, self.D, self.dev)
        self.Wd, self.Hd = self.Ws.clone(), self.Hs.clone()

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def sparse(self, iters):
        rc = self.lib.gpz_nmf_kl_sparse_update(*self.ptrs, C.c_void_p(self.Ws.data_ptr()), C.c_void_p(self.Hs.data_ptr()), self.N,
                                               self.D, self.c.nnz, L, _lib.GPZ_F32, iters, C.c_void_p(self.ws_s.data_ptr()),
                                               self.nb_s, self.stream())
        _lib.check(rc, "gpz_nmf_kl_sparse_update")

    def dense(self, iters):
        rc = self.lib.gpz_nmf_kl_update(C.c_void_p(self.X.data_ptr()), C.c_void_p(self.Wd.data_ptr()), C.c_void_p(self.Hd.data_ptr()),
                                        self.N, self.D, L, _lib.GPZ_F32, iters, C.c_void_p(self.ws_d.data_ptr()), self.nb_d,
                                        self.stream())
        _lib.check(rc, "gpz_nmf_kl_update")


def alternating_ms(fns, iters):
    """Median milliseconds per call of each function, the functions called in turn inside every repetition."""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(REPS)]
    for _ in range(WARM):
        for fn in fns:
            fn(iters)
    torch.cuda.synchronize()
    for row in ev:
        for fn, (a, b) in zip(fns, row):
            a.record(); fn(iters); b.record()
    torch.cuda.synchronize()
    return [statistics.median(row[i][0].elapsed_time(row[i][1]) for row in ev) for i in range(len(fns))]


def iteration_point(density, dev):
    counts, y = sparse_counts(D1, N1, density, dev, seed=int(1000 * density), dense=True)
    X = y.T.contiguous()
    del y
    e = Entries(counts, X, dev)
    e.sparse(1); e.dense(1)
    agree = max(float((e.Ws - e.Wd).abs().max() / e.Wd.abs().max()), float((e.Hs - e.Hd).abs().max() / e.Hd.abs().max()))
    e.reset()
    s20, d20 = alternating_ms([e.sparse, e.dense], ITERS)
    e.reset()
    s1, d1 = alternating_ms([e.sparse, e.dense], 1)
    return dict(what="iteration", N=N1, D=D1, L=L, density=density, nnz=counts.nnz, sparse_iter_ms=s20 / ITERS,
                dense_iter_ms=d20 / ITERS, sparse_call1_ms=s1, dense_call1_ms=d1, rel_diff_after_1=agree,
                x_dense_bytes=X.numel() * 4, x_sparse_bytes=held_bytes(counts), sparse_ws_bytes=e.nb_s, dense_ws_bytes=e.nb_d)


def slideseq_point(dev):
    counts, _ = sparse_counts(DS, NS, 0.05, dev, seed=50)
    e = Entries(counts, None, dev)
    s20, = alternating_ms([e.sparse], ITERS)
    e.reset()
    s1, = alternating_ms([e.sparse], 1)
    return dict(what="slideseq", N=NS, D=DS, L=L, density=0.05, nnz=counts.nnz, sparse_iter_ms=s20 / ITERS, sparse_call1_ms=s1,
                x_dense_bytes=NS * DS * 4, x_sparse_bytes=held_bytes(counts), sparse_ws_bytes=e.nb_s)


def wall_ms(fn, reps=3):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), torch.cuda.max_memory_allocated()


def end_to_end_point(density, dev):
    from gpzoo_amd.utilities import regularized_nmf
    kw = dict(solver="mu", beta_loss="kullback-leibler", init="nndsvd", max_iter=200, tol=0)
    counts, y = sparse_counts(D1, N1, density, dev, seed=int(1000 * density), dense=True)
    X = y.T.contiguous()
    del y
    rec = dict(what="end_to_end", N=N1, D=D1, L=L, density=density, nnz=counts.nnz, x_dense_bytes=X.numel() * 4,
               x_sparse_bytes=held_bytes(counts))
    rec["dense_init_ms"], _ = wall_ms(lambda: nmf.initialize_nmf(X, L, init="nndsvd"))
    rec["dense_total_ms"], rec["dense_peak_bytes"] = wall_ms(lambda: regularized_nmf(X, L, **kw))
    del X
    ops.release_workspaces()
    torch.cuda.empty_cache()
    rec["sparse_init_ms"], _ = wall_ms(lambda: nmf.initialize_nmf(counts.T, L, init="nndsvd"))
    rec["sparse_total_ms"], rec["sparse_peak_bytes"] = wall_ms(lambda: regularized_nmf(counts.T, L, **kw))
    return rec


def show(r):
    mib = lambda b: f"{b / 2 ** 20:8.1f} MiB"
    if r["what"] == "iteration":
        print(f"iteration  {r['N']} x {r['D']} L {r['L']} density {r['density']:4.2f} nnz {r['nnz']:>9d}: dense {r['dense_iter_ms']:.3f} ms, "
              f"sparse {r['sparse_iter_ms']:.3f} ms per iteration ({r['dense_iter_ms'] / r['sparse_iter_ms']:.2f}x); a call of one: dense "
              f"{r['dense_call1_ms']:.3f}, sparse {r['sparse_call1_ms']:.3f} ms; X {mib(r['x_dense_bytes'])} dense, {mib(r['x_sparse_bytes'])} "
              f"sparse; workspace {mib(r['dense_ws_bytes'])} / {mib(r['sparse_ws_bytes'])}; rel diff after 1 {r['rel_diff_after_1']:.1e}", flush=True)
    elif r["what"] == "slideseq":
        print(f"slideseq   {r['N']} x {r['D']} L {r['L']} density {r['density']:4.2f} nnz {r['nnz']:>9d}: sparse {r['sparse_iter_ms']:.3f} ms per "
              f"iteration, a call of one {r['sparse_call1_ms']:.3f} ms; X would be {mib(r['x_dense_bytes'])} dense, is {mib(r['x_sparse_bytes'])} "
              f"sparse; workspace {mib(r['sparse_ws_bytes'])}", flush=True)
    else:
        print(f"end_to_end {r['N']} x {r['D']} L {r['L']} density {r['density']:4.2f}: dense {r['dense_total_ms']:.1f} ms (init "
              f"{r['dense_init_ms']:.1f}), sparse {r['sparse_total_ms']:.1f} ms (init {r['sparse_init_ms']:.1f}); peak device memory "
              f"{mib(r['dense_peak_bytes'])} dense, {mib(r['sparse_peak_bytes'])} sparse", flush=True)


def main():
    args = sys.argv[1:]
    dev = torch.device("cuda")
    if "--once" in args:
        density = float(args[args.index("--once") + 1])
        counts, y = sparse_counts(D1, N1, density, dev, seed=int(1000 * density), dense=True)
        e = Entries(counts, y.T.contiguous(), dev)
        e.sparse(ITERS); e.dense(ITERS)
        torch.cuda.synchronize()
        print(f"once: density {density}, nnz {counts.nnz}, {ITERS} iterations of each entry")
        return
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    parts = args or ["iteration", "slideseq", "end_to_end"]
    rows = []
    for part in parts:
        points = {"iteration": [lambda d=d: iteration_point(d, dev) for d in DENSITIES], "slideseq": [lambda: slideseq_point(dev)],
                  "end_to_end": [lambda d=d: end_to_end_point(d, dev) for d in DENSITIES]}[part]
        for p in points:
            r = p()
            rows.append(r)
            show(r)
            ops.release_workspaces()
            torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
