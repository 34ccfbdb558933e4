#!/usr/bin/env python3
"""Golden vectors of the train / validation split, by running the REFERENCE's anndata_to_train_val itself (build
container only).

    MPLBACKEND=Agg python tests/golden/make_trainval_golden.py

Imports luisdiaz1997/GPzoo from /root/reference (read-only, never copied, never shipped) and runs its
``anndata_to_train_val`` on a small duck-typed stand-in for an AnnData object (N = 97 spots, D = 23 genes; ``X`` with a
``toarray`` method, ``obsm['spatial']``, ``shape``, ``layers``) for train_frac 0.8 and 1.0 and the three ``sz`` modes.
Stores the inputs (the UNRESCALED coordinates and the counts, spots x genes as the reference holds them) and the outputs
(each split's Y, sz and, where the reference sets it, idx) as extra_trainval_*.npz next to this script.  The reference
rescales the coordinates inside the function; tests/test_deviance_api.py compares rows of X by index only.  Data only."""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, "/root/reference")

import numpy as np

from gpzoo.utilities import anndata_to_train_val  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
N, D = 97, 23


class _Counts:
    """What ``ad.X`` needs for the reference: ``toarray()``."""

    def __init__(self, a):
        self.a = a

    def toarray(self):
        return self.a.copy()


class _AnnData:
    def __init__(self, Y, coords):
        self.X, self.obsm, self.layers, self.shape = _Counts(Y), {"spatial": coords}, {}, Y.shape


def main():
    rng = np.random.default_rng(20240)
    depth = np.exp(0.6 * rng.standard_normal((N, 1)))
    Y = rng.poisson(depth * rng.gamma(0.7, 2.0, size=(1, D))).astype(np.float64)
    Y[rng.random((N, D)) < 0.4] = 0.0
    Y[5, :] = 0.0                                   # a spot without counts
    Y[:, 7] = 0.0                                   # a gene without counts
    coords = rng.uniform(0.0, 3000.0, size=(N, 2))
    for frac in (0.8, 1.0):
        for sz in ("constant", "mean", "scanpy"):
            Dtr, Dval = anndata_to_train_val(_AnnData(Y, coords.copy()), train_frac=frac, sz=sz)
            out = dict(coords=coords, Y=Y, train_frac=np.float64(frac), has_val=np.int64(Dval is not None))
            for tag, d in (("tr", Dtr), ("val", Dval)):
                if d is None:
                    continue
                out[f"{tag}_Y"], out[f"{tag}_sz"] = d["Y"], d["sz"]
                if "idx" in d:
                    out[f"{tag}_idx"] = d["idx"]
            name = f"extra_trainval_{sz}_frac{int(round(100 * frac))}.npz"
            np.savez_compressed(os.path.join(HERE, name), **out)
            print(name, {k: getattr(v, "shape", v) for k, v in out.items()})


if __name__ == "__main__":
    main()
