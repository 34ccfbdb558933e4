"""CPU: the case builders and the fp64 reference of tests/backward_forms_cases.py are what the GPU tests take them for --
the clamp recipes really put columns on both sides of their clamp, the reference loss's autograd gradients are the
derivatives of the loss (central differences), a one-hot upstream picks one column of W, and the restated launch
arithmetic gives the piece and chunk boundaries the shapes were chosen for."""
import pytest
import torch

import backward_forms_cases as BC

# (N, M, L) of the GPU file's shapes B, D, E
B, D, E = (300, 129, 2), (2100, 200, 2), (700, 640, 2)


@pytest.mark.parametrize("shape,recipe,whitened", [(B, "unwhitened_clamp", False), (D, "unwhitened_clamp", False),
                                                   (E, "unwhitened_clamp", False), (B, "whitened_clamp", True),
                                                   (D, "whitened_clamp", True)])
def test_clamp_recipes_put_columns_on_both_sides(shape, recipe, whitened):
    """Per latent: at least 5 % of the columns clamped, at least 5 % not, at most 5 % within 1e-2 of the threshold (those
    get gs = 0); and Kzz of the recipe is positive-definite (the oracle's Cholesky succeeds)."""
    c = BC.make_case(*shape, recipe=recipe)
    with torch.no_grad():
        p = BC.forward_parts(c, BC.make_leaves(c, requires_grad=False), whitened)
    assert torch.isfinite(p["scale"]).all() and torch.isfinite(p["chol"]).all()
    frac = p["clamped"].double().mean(1)
    near = p["near"].double().mean(1)
    print(shape, recipe, "clamped", frac.tolist(), "near", near.tolist())
    assert (frac >= 0.05).all() and (frac <= 0.95).all(), frac
    assert (near <= 0.05).all(), near
    up = BC.make_upstream(c, whitened, "dense")
    assert (up["gs"][p["near"]] == 0).all()
    if whitened:     # Hd's gate must see chunks with and without a clamped column when D runs in chunks of 1024
        per_chunk = [bool(p["clamped"][:, n0:n0 + 1024].any()) for n0 in range(0, shape[0], 1024)]
        print("chunks holding a clamped column:", per_chunk)
        if shape == D:
            assert any(per_chunk) and not all(per_chunk), per_chunk


@pytest.mark.parametrize("whitened", [True, False])
@pytest.mark.parametrize("kind", BC.KINDS)
def test_reference_gradients_against_central_differences(kind, whitened):
    """N=7, M=3, L=2 (the scalar kernel: L=1), inputs drawn 20 times closer so that every point sees its neighbours."""
    c = BC.make_case(7, 3, 1 if kind == "rbf_scalar" else 2, kind=kind)
    c["X"], c["Z"] = c["X"] / 20, c["Z"] / 20
    c["lengthscale"] = c["lengthscale"] / 4
    up = BC.make_upstream(c, whitened, "dense")
    leaf = BC.make_leaves(c)
    loss, _ = BC.oracle_loss(c, leaf, whitened, up, True)
    loss.backward()
    h = 1e-5
    for name, t in leaf.items():
        fd = torch.zeros_like(t)
        flat, out = t.detach().reshape(-1), fd.reshape(-1)
        for i in range(flat.numel()):
            vals = []
            for s in (1.0, -1.0):
                moved = {k: v.detach().clone() for k, v in leaf.items()}
                moved[name].reshape(-1)[i] += s * h
                with torch.no_grad():
                    vals.append(float(BC.oracle_loss(c, moved, whitened, up, True)[0]))
            out[i] = (vals[0] - vals[1]) / (2 * h)
        scale = max(float(fd.abs().max()), 1e-12)
        err = float((t.grad - fd).abs().max()) / scale
        # central differences are second order except across Matern-1/2's kink at a coincident pair (every inducing point
        # is a data point): both displaced evaluations see that covariance lowered by h / l, so the rest of the loss is
        # differenced at a point O(h / l) away -- a first-order error of that relative size
        tol = h / float(c["lengthscale"].min()) if (kind, name) == ("matern12", "Z") else 1e-6
        assert err < tol, (name, err)


def test_one_hot_mean_upstream_picks_a_column_of_w():
    from oracle import svgp_oracle as O
    c = BC.make_case(*B)
    leaf = BC.make_leaves(c)
    n, l = 137, 1
    zero = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    up = dict(gm=zero(2, 300), gs=zero(2, 300), w=zero(2), gc=zero(2, 129, 129))
    up["gm"][l, n] = 1.0
    loss, p = BC.oracle_loss(c, leaf, True, up, False)
    loss.backward()
    Kzx = O.kernel_matrix("nsf_rbf", c["Z"], c["X"], c["sigma"], c["lengthscale"])
    W = torch.linalg.solve_triangular(p["chol"].detach(), Kzx, upper=False)
    torch.testing.assert_close(leaf["mu"].grad[l], W[l, :, n], rtol=1e-12, atol=1e-14)
    assert float(W[l, :, n].abs().max()) > 1e-3
    assert not leaf["mu"].grad[0].any() and not leaf["Lu_raw"].grad.any()


def test_probe_columns_follow_the_launch_arithmetic():
    # D whole: ncp = 2176 = 17 * 128, three 128-row tiles per latent -> cut in two pieces of 1088 columns
    assert BC.wide_nt_pieces(256, 2176, 2) == 2 and BC.piece_extent(256, 2176, 2) == 1088
    assert BC.probe_columns(*D) == [0, 1087, 1088, 2099]
    # D in chunks of 1024: no cut inside a chunk, boundaries at 1024 and 2048 (the last chunk: 52 columns, one tile)
    assert BC.probe_columns(*D, chunk=1024) == [0, 1023, 1024, 2047, 2048, 2099]
    assert BC.probe_columns(*B) == [0, 299] and BC.probe_columns(1, 1, 1) == [0]
    # H: 11 row-tile slots x 16 latents = 176 tiles -> two pieces of 5504 columns
    assert BC.nt_tiles(5) == 11 and BC.piece_extent(640, 11008, 16) == 5504
    assert BC.probe_columns(11008, 640, 16) == [0, 5503, 5504, 11007]
    up = BC.make_upstream(BC.make_case(*D), True, "probe", 1024)
    cols = up["gm"].abs().sum(0).nonzero()[:, 0].tolist()
    assert cols == [0, 1023, 1024, 2047, 2048, 2099]
    assert float(up["gm"][:, cols].abs().min()) >= 1.0 and float(up["gm"].abs().max()) <= 2.0


def test_probe_columns_reach_the_inducing_points():
    """A dropped probe column must move a gradient: each one has a W column of size > 1e-2 in some latent."""
    from oracle import svgp_oracle as O
    for shape, chunk in ((D, 0), (D, 1024), (E, 0)):
        c = BC.make_case(*shape)
        Kzx = O.kernel_matrix("nsf_rbf", c["Z"], c["X"], c["sigma"], c["lengthscale"])
        Kzz = O.kernel_matrix("nsf_rbf", c["Z"], c["Z"], c["sigma"], c["lengthscale"]) + c["jitter"] * torch.eye(c["M"], dtype=torch.float64)
        W = torch.linalg.solve_triangular(torch.linalg.cholesky(Kzz), Kzx, upper=False)
        size = W[:, :, BC.probe_columns(*shape, chunk=chunk)].abs().amax((0, 1))
        print(shape, chunk, size.tolist())
        assert (size > 1e-2).all(), size


def test_form_rule_restated():
    # (N, M) of the GPU shapes: what the library picks with all parameters in fp32 whitened
    picks = {s: BC.library_picks_algebra(s[0], s[1], True, True, True) for s in ((300, 129), (129, 300), (2100, 200), (700, 640), (900, 700), (11008, 640))}
    assert picks == {(300, 129): False, (129, 300): False, (2100, 200): True, (700, 640): False, (900, 700): False, (11008, 640): True}
    assert BC.library_picks_algebra(300, 129, False, True, True)            # mu / Lu only: N >= 0.75 Mp
    assert not BC.library_picks_algebra(2100, 640, True, True, False)       # un-whitened fp32: N >= 4.4 Mp
    assert BC.library_picks_algebra(2100, 640, True, False, False)
