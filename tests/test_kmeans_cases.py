"""CPU: the shapes of tests/kmeans_cases.py are what tests/test_hip_kmeans.py takes them for -- the constants are the
``constexpr`` values of csrc/kmeans.hip, the edge list reaches every tile edge, dimension and dtype, the path list reaches
both assignment paths on both sides of each switch, and the built data sets have the clusters, ties and empty clusters
they claim (checked with the numpy oracle)."""
import os
import re

import numpy as np

import kmeans_cases as K
import kmeans_oracle as O
from conftest import ROOT


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "gpzoo_amd", "csrc", "kmeans.hip")).read()
    found = {n: int(v) for n, v in re.findall(r"^constexpr int KMS_(\w+) = (\d+);", src, flags=re.M)}
    assert found["T_C"] == K.T_C and found["B_N"] == K.B_N and found["S"] == K.S and found["SPLIT_WGS"] == K.SPLIT_WGS
    assert K.S == 64                                  # one lane of a wave per residue
    assert found["MAX_T"] >= O.n_trials(2 ** 31 - 1)


def test_edge_list_reaches_every_edge_dimension_and_dtype():
    cases = K.edge_cases()
    assert {M for _, M, _, _ in cases} == set(K.EDGE_M) == {1, K.T_C - 1, K.T_C, K.T_C + 1, 2 * K.T_C + 1}
    for M in K.EDGE_M:
        assert {N for N, m, _, _ in cases if m == M} >= {n for n in (M, K.B_N - 1, K.B_N, K.B_N + 1, 2 * K.B_N + 3) if n >= M}
    assert all(M <= N <= 5000 for N, M, _, _ in cases)
    assert {(d, t) for _, _, d, t in cases} == {(d, t) for d in (1, 2, 3, 4) for t in ("f64", "f32")}
    for N, M, d, t in cases:
        X, C0 = K.random_case(N, M, d, t)
        assert X.shape == (N, d) and X.dtype == K.dtype_of(t) and C0.shape == (M, d) and C0.dtype == np.float64
    assert len(cases) <= 32


def test_path_list_reaches_both_paths_on_both_sides_of_each_switch():
    plans = [K.split_plan(N, M) for N, M, _ in K.PATH_CASES]
    assert all(1 <= M <= N for N, M, _ in K.PATH_CASES)
    assert [p["splits"] for p in plans] == [1, 2, 3, 2, 2, 1]
    assert [p["tiles_per_split"] for p in plans] == [1, 1, 1, 2, 1, 2]
    assert plans[4]["tiles"] == K.SPLIT_WGS - 1 and plans[5]["tiles"] == K.SPLIT_WGS
    assert plans[3]["ctiles"] == 3                    # splits of two and of one centre tiles
    # the notebook's shape and the small-N shape of tools/kmeans_step.py are split, the large one is not needed to be
    assert K.split_plan(39694, 3000)["splits"] > 1 and K.split_plan(7000, 3000)["splits"] > 1
    for N, M, _ in K.PATH_CASES:                      # never more workgroups than the target, but for one rounding up
        p = K.split_plan(N, M)
        assert p["splits"] * p["tiles_per_split"] >= p["ctiles"] > (p["splits"] - 1) * p["tiles_per_split"]


def test_blob_case_has_the_cluster_sizes():
    X, C0, sizes = K.blob_case()
    assert sizes == [1, K.S - 1, K.S, K.S + 1, 2 * K.S + 1]
    labels, _ = O.assign(X, C0)
    assert np.bincount(labels, minlength=len(sizes)).tolist() == sizes
    assert not np.array_equal(labels, np.sort(labels))           # shuffled: members are not contiguous


def test_tie_case_ties_across_tiles_and_leaves_the_higher_duplicate_empty():
    X, C0 = K.tie_case()
    M = len(C0)
    assert M - 1 >= K.T_C and len(X) >= M
    D = O.d2_matrix(X, C0)
    assert (D[:10, 3] == D[:10, M - 1]).all() and (D[:10, 3] == D[:10].min(axis=1)).all()
    assert (D[10:20, 5] == D[10:20, 9]).all() and (D[10:20, 5] == D[10:20].min(axis=1)).all()
    labels, _ = O.assign(X, C0)
    assert (labels[:10] == 3).all() and (labels[10:20] == 5).all()
    counts = np.bincount(labels, minlength=M)
    assert counts[9] == 0 and counts[M - 1] == 0 and (np.delete(counts, [9, M - 1]) > 0).all()
    assert [m[2] for m in O.lloyd_iter(X, C0)[3]] == [9, M - 1]


def test_empty_cases_relocate_one_and_three():
    for n_empty in (1, 3):
        X, C0 = K.empty_case(n_empty)
        C1, labels, _, moved = O.lloyd_iter(X, C0)
        assert [to for _, _, to in moved] == list(range(len(C0) - n_empty, len(C0)))
        d2 = O.assign(X, C0)[1]
        assert [n for n, _, _ in moved] == list(np.argsort(-d2, kind="stable")[:n_empty])
        assert len({frm for _, frm, _ in moved} & {to for _, _, to in moved}) == 0
        for n, _, to in moved:
            np.testing.assert_array_equal(C1[to], X[n])


def test_few_distinct_case():
    X, M = K.few_distinct_case()
    assert len(X) == 40 and len(np.unique(X, axis=0)) == 10 and M == 16
    o = O.kmeans(X, M, random_state=0)
    assert o["inertia"] == 0.0 and o["relocated"] == 0 and np.isfinite(o["centres"]).all()
    assert len(np.unique(o["seed_indices"])) < M                 # the potential reached 0: index 0 is drawn again
    u = np.random.default_rng(0).random((M, O.n_trials(M)))
    idx, draw_margin, win_margin = O.seed(X, M, u)
    np.testing.assert_array_equal(idx, o["seed_indices"])
    assert draw_margin > 1e-9 and win_margin > 1e-9              # the GPU test compares the indices exactly
