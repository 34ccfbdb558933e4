#!/usr/bin/env python3
"""Record the bits of every spatial-autocorrelation entry (needs a GPU and the built library).

    python tests/golden/make_autocorr_bits_golden.py

Writes tests/golden/extra_autocorr_bits.npz: outputs only, as tests/autocorr_bits_cases.py lays them out (fp64 as int64 views,
integers as they are, the plan queries' values).  The inputs are regenerated from the seeded case modules by the test.
Recorded from the commit before the gene pass and the column pass were each made one template; a change of these kernels
that keeps the file passing has kept every entry's numbers."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import autocorr_bits_cases as A  # noqa: E402


def main():
    out = A.plans()
    for name, group in A.GROUPS.items():
        got = group()
        print(f"{name}: {len(got)} arrays", flush=True)
        out.update(got)
    np.savez_compressed(A.PATH, **out)
    size = os.path.getsize(A.PATH)
    assert size < 1000 * 1000, size
    print(f"{len(out)} arrays, {size} bytes -> {A.PATH}")


if __name__ == "__main__":
    main()
