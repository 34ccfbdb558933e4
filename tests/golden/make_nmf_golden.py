#!/usr/bin/env python3
"""Generate the regularized_nmf golden vectors by running the REFERENCE and sklearn (build container, CPU only).

    MPLBACKEND=Agg python tests/golden/make_nmf_golden.py

Imports luisdiaz1997/GPzoo from /root/reference like make_golden.py (read-only, never copied, never shipped) and writes
tests/golden/extra_nmf_<case>.npz -- the ``extra_`` prefix keeps them out of conftest.golden_cases(), which lists SVGP
parity cases.  Data only.  Per case, on a planted count matrix Y = Poisson(6 F W / L), F ~ Gamma(0.6), W ~ Gamma(0.5):

  Y (integer counts), kwargs (JSON), sz;  sklearn's starting values W0, H0 (fp64 input);
  F64, W64: the reference's regularized_nmf for Y in float64;  F32, W32: the same for Y cast to float32;
  nmfW64, nmfH64, nmfW32, nmfH32: the raw factorisations behind them (sklearn's NMF with the same keywords);
  n_iter64, n_iter32.

A fixture is only written when it meets what the tests rely on:
  (a) sklearn's (W0, H0) and the same routine fed scipy's exact SVD agree to 1e-8 absolute and share their zero pattern
      (the triplets are converged: any accurate SVD gives these starting values);
  (b) no entry of the unclipped NNDSVD lies within 1e-7 of the 1e-6 clipping threshold;
  (c) the float32 and float64 runs stop at the same iteration.
"""
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, "/root/reference")

import numpy as np
import scipy.linalg
import sklearn.decomposition._nmf as sk_nmf
from sklearn.decomposition import NMF

from gpzoo.utilities import regularized_nmf  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from nmf_oracle import planted_counts  # noqa: E402

CASES = {
    # name: (N, D, L, seed, NMF keywords, shrinkage, size factors?); seeds whose matrix meets (a)-(c) -- at D = 80 the
    # singular gap of many draws leaves sklearn's randomized SVD 1e-8 .. 1e-5 from the exact one
    "nndsvdar_600x150": (600, 150, 4, 11, dict(max_iter=200, init="nndsvdar", random_state=997), 0.3, False),
    "nndsvda_1037x80_tol0": (1037, 80, 4, 24, dict(max_iter=200, init="nndsvda", tol=0.0, random_state=997), 0.2, False),
    "nndsvd_600x150_sz": (600, 150, 4, 30, dict(max_iter=30, init="nndsvd", random_state=997), 0.3, True),
    "random_600x150": (600, 150, 4, 14, dict(max_iter=100, init="random", random_state=5), 0.3, False),
}


def exact_svd(M, n_components, **_):
    U, S, Vt = scipy.linalg.svd(M, full_matrices=False)
    return U[:, :n_components], S[:n_components], Vt[:n_components]


def init_conditions(Y, L, init, random_state):
    W0, H0 = sk_nmf._initialize_nmf(Y, L, init=init, random_state=random_state)
    if init == "random":
        return W0, H0
    keep = sk_nmf._randomized_svd
    sk_nmf._randomized_svd = exact_svd
    try:
        We, He = sk_nmf._initialize_nmf(Y, L, init=init, random_state=random_state)
        Wr, Hr = sk_nmf._initialize_nmf(Y, L, init="nndsvd", eps=0.0, random_state=random_state)
    finally:
        sk_nmf._randomized_svd = keep
    Wz, Hz = sk_nmf._initialize_nmf(Y, L, init="nndsvd", random_state=random_state)
    Wze, Hze = np.where(Wr < 1e-6, 0.0, Wr), np.where(Hr < 1e-6, 0.0, Hr)
    gap = max(np.abs(W0 - We).max(), np.abs(H0 - He).max())
    assert gap < 1e-8, f"(a) randomized vs exact SVD starting values differ by {gap:.2e}"
    assert ((Wz == 0) == (Wze == 0)).all() and ((Hz == 0) == (Hze == 0)).all(), "(a) zero patterns differ"
    for M in (Wr, Hr):
        near = np.abs(M - 1e-6) < 1e-7
        assert not near.any(), f"(b) {int(near.sum())} entries within 1e-7 of the clipping threshold"
    print(f"    (a) {gap:.1e}   (b) none")
    return W0, H0


def main():
    for name, (N, D, L, seed, kw, shrinkage, with_sz) in CASES.items():
        print(name)
        Y = planted_counts(N, D, L, seed)
        assert Y.max() < 2 ** 15
        kw = dict(kw, solver="mu", beta_loss="kullback-leibler")
        sz = 1
        if with_sz:
            tot = Y.sum(axis=1, keepdims=True)
            assert (tot > 0).all(), "size factors need a Y without empty rows"
            sz = tot / np.median(tot)
        W0, H0 = init_conditions(Y, L, kw["init"], kw["random_state"])
        out = {}
        for tag, dt in (("64", np.float64), ("32", np.float32)):
            Yd = Y.astype(dt)
            model = NMF(L, **kw)
            eF = model.fit_transform(Yd)
            F, W = regularized_nmf(Yd, L, sz=sz, shrinkage=shrinkage, **kw)
            out["F" + tag], out["W" + tag] = F, W
            out["nmfW" + tag], out["nmfH" + tag], out["n_iter" + tag] = eF, model.components_, model.n_iter_
            print(f"    float{tag}: n_iter {model.n_iter_}, F {F.dtype}, W {W.dtype}")
        assert out["n_iter64"] == out["n_iter32"], "(c) the float32 and float64 runs stop at different iterations"
        dF = np.abs(out["F32"] - out["F64"]).max()
        dW = np.abs(out["nmfW32"] - out["nmfW64"]).max() / np.abs(out["nmfW64"]).max()
        dH = np.abs(out["nmfH32"] - out["nmfH64"]).max() / np.abs(out["nmfH64"]).max()
        print(f"    float32 vs float64: F {dF:.1e} abs, nmf W {dW:.1e} rel, nmf H {dH:.1e} rel")
        path = os.path.join(HERE, f"extra_nmf_{name}.npz")
        np.savez_compressed(path, Y=Y.astype(np.int16), kwargs=json.dumps(kw), L=L, shrinkage=shrinkage,
                            sz=np.asarray(sz, dtype=np.float64), W0=W0, H0=H0, **out)
        assert os.path.getsize(path) < 512 * 1024, os.path.getsize(path)
        print(f"    {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
