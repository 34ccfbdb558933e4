"""GPU: every entry gives the same bits whatever its scratch memory and its freshly allocated outputs held before.

gpzoo_amd/ops.py keeps one scratch buffer per (device, stream) and never clears it; outputs, ``info`` words and caches are
``torch.empty``.  For every row of tests/scratch_cases.py (tests/test_scratch_cases.py checks the table on the CPU):

  a. on the stream's one buffer, grown to the LARGE shape's size first: SMALL and LARGE on zeros (s0, l0), SMALL again on
     what LARGE left behind (s1), both on 0xFF bytes (NaN as fp32 and fp64, -1 as an integer: s2, l2) and on 0x40 bytes
     (3.0039 as fp32, 32.5 as fp64, a large positive integer: s3, l3).  s0 = s1 = s2 = s3 and l0 = l2 = l3, bit for bit.
     Opaque byte buffers (wt_cache, state, factor cache) are compared through the pass that consumes them and, where it is
     documented, on their written extent;
  b. with every ``torch.empty`` / ``torch.empty_like`` of gpzoo_amd.ops returning 0xFF bytes -- outputs, info, kl, scal,
     caches and a freshly grown workspace --: the bits of s0 / l0 again, every floating output finite, every index in range;
  c. the 0xFF run against the row's fp64 oracle at the tolerance of the entry's own test file (every row has one), so that
     equal bits are not two equal wrong answers;
  d. one test replays a training and an evaluation step on one buffer, each result the bits of the entry run alone.

DESIGN.md, "Scratch and output initialisation", lists every carved region with its first writer and reader."""
import os
import subprocess
import sys

import pytest
import torch

import scratch_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def differing(a: dict, b: dict) -> list:
    """Names of the outputs whose bits differ (shape and dtype must agree)."""
    assert set(a) == set(b)
    out = []
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        if not torch.equal(_bytes(a[k]), _bytes(b[k])):
            out.append(k)
    return out


def same_bits(a: dict, b: dict, what):
    bad = differing(a, b)
    assert not bad, (what, bad)


def _buffers(ops) -> list:
    torch.cuda.synchronize()
    assert ops._workspaces
    return list(ops._workspaces.values())


def _fill(ops, value: int):
    for w in _buffers(ops):
        w.fill_(value)


def sequence(r, ops):
    """Steps 1-6 on the stream's buffer; returns (s0, l0, s2, l2, small state, large state)."""
    small, large = r.prepare(r.inputs("small")), r.prepare(r.inputs("large"))
    ops.release_workspaces()
    r.run(ops, large)                                   # the buffer exists at the size the LARGE shape needs
    held = _buffers(ops)
    _fill(ops, 0)
    s0, l0 = r.run(ops, small), r.run(ops, large)
    s1 = r.run(ops, small)                              # LARGE's data lies behind SMALL's regions
    _fill(ops, 0xFF)
    s2, l2 = r.run(ops, small), r.run(ops, large)
    _fill(ops, 0x40)
    s3, l3 = r.run(ops, small), r.run(ops, large)
    now = _buffers(ops)
    assert len(now) == len(held) and all(a is b for a, b in zip(now, held)), "the buffer was reallocated during the sequence"
    if r.bytes is not None:
        assert all(w.numel() >= int(r.bytes("large")) for w in now)
    differ = []                                         # every step that differs is named, not only the first
    for which, first, runs in (("small", s0, (("step 4, after LARGE", s1), ("step 5, on 0xFF", s2), ("step 6, on 0x40", s3))),
                               ("large", l0, (("step 5, on 0xFF", l2), ("step 6, on 0x40", l3)))):
        for tag, other in runs:
            bad = differing(first, other)
            if bad:
                differ.append(f"{which}, {tag}: {', '.join(bad)}")
    assert not differ, (r.name, differ)
    return s0, l0, s2, l2, small, large


class _PoisonedTorch:
    """``torch`` for gpzoo_amd.ops with ``empty`` and ``empty_like`` returning 0xFF bytes."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _poison(t):
        if t.numel():
            t.reshape(-1).view(torch.uint8).fill_(0xFF)
        return t

    def empty(self, *a, **kw):
        return self._poison(torch.empty(*a, **kw))

    def empty_like(self, *a, **kw):
        return self._poison(torch.empty_like(*a, **kw))


def check_ranges(r, which, out):
    c = r.inputs(which)
    for k, v in out.items():
        if v.is_floating_point():
            assert bool(torch.isfinite(v).all()), (r.name, which, k)
    for k, bound in r.index.items():
        assert int(out[k].min()) >= 0 and int(out[k].max()) < int(bound(c)), (r.name, which, k)


def poisoned_allocations(r, ops, small, large, s0, l0, patch):
    """b. every allocation of gpzoo_amd.ops poisoned, the workspace included: it is grown afresh for each shape.
    ``patch(ops, "torch", proxy)`` installs the proxy; the caller takes it out again."""
    patch(ops, "torch", _PoisonedTorch())
    probe = ops.torch.empty(3, dtype=torch.float32, device="cuda")
    assert bool(torch.isnan(probe).all())
    for which, state, want in (("small", small, s0), ("large", large, l0)):
        ops.release_workspaces()
        got = r.run(ops, state)
        same_bits(want, got, (r.name, which, "poisoned allocations"))
        check_ranges(r, which, got)
    ops.release_workspaces()


@pytest.mark.parametrize("name", [r.name for r in S.ROWS])
def test_same_bits_on_stale_and_poisoned_memory(name, monkeypatch):
    from gpzoo_amd import ops
    r = S.row(name)
    s0, l0, s2, l2, small, large = sequence(r, ops)
    check_ranges(r, "small", s2)
    check_ranges(r, "large", l2)
    if name.startswith("factor-"):                      # the library's choice at these orders is the one-launch path
        from gpzoo_amd import _lib
        assert all(_lib.load().gpz_factor_path(M, 0) == 1 for M, _ in S.FACTOR_SHAPES.values())
    poisoned_allocations(r, ops, small, large, s0, l0, monkeypatch.setattr)
    monkeypatch.undo()
    # c. the 0xFF run against the oracle
    r.check("small", r.inputs("small"), s2)
    r.check("large", r.inputs("large"), l2)


STEP = ("svgp_forward-path1", "nb_nsf_sparse-batch-no_lgamma", "svgp_backward-algebra-wide-all-wt-f32",
        "vnngp-f32-state-grads-order", "nb_deviance", "svgp_forward-path1")


def test_a_training_and_evaluation_step_on_one_buffer():
    """svgp_forward, nb_nsf_sparse, svgp_backward, vnngp_forward (and its backward), nb_deviance and svgp_forward again, at
    their LARGE shapes on one buffer that starts as 0xFF bytes: each result is the bits of the entry run alone after
    ``release_workspaces()``."""
    from gpzoo_amd import ops
    rows = [S.row(n) for n in STEP]
    states = {r.name: r.prepare(r.inputs("large")) for r in rows}
    alone = {}
    for r in rows:
        if r.name not in alone:
            ops.release_workspaces()
            alone[r.name] = r.run(ops, states[r.name])
    ops.release_workspaces()
    for r in rows:                                      # grow the one buffer to the largest need, then poison it
        r.run(ops, states[r.name])
    _fill(ops, 0xFF)
    held = _buffers(ops)
    for i, r in enumerate(rows):
        same_bits(alone[r.name], r.run(ops, states[r.name]), (i, r.name))
    assert all(a is b for a, b in zip(_buffers(ops), held))
    ops.release_workspaces()


_LAUNCHES_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from gpzoo_amd import ops, _lib
import scratch_cases as S
import test_hip_scratch as T
assert all(_lib.load().gpz_factor_path(M, 0) == 0 for M, _ in S.FACTOR_SHAPES.values())
for name in ("factor-f64", "factor-f32"):
    r = S.row(name)
    s0, l0, s2, l2, small, large = T.sequence(r, ops)
    try:
        T.poisoned_allocations(r, ops, small, large, s0, l0, setattr)
    finally:
        ops.torch = torch
    r.check("small", r.inputs("small"), s2)
    r.check("large", r.inputs("large"), l2)
print("launch-per-step ok")
"""


def test_launch_per_step_factorisation():
    """GPZ_FACTOR_PATH=launches is read once per process, hence a child: the factorisation rows on the launch-per-step
    path, the same sequence, the same poisoned allocations and the same oracle."""
    env = dict(os.environ, GPZ_FACTOR_PATH="launches")
    p = subprocess.run([sys.executable, "-c", _LAUNCHES_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "launch-per-step ok" in p.stdout
