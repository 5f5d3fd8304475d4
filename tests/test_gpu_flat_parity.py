"""Flat-buffer mode against autograd mode, op by op.

Every op that takes parameters runs twice on the same inputs, the same
parameter values and the same torch.manual_seed: once with plain
requires_grad parameters, once with parameters carrying a `_flat_grad` view
(runtime/optimizer.py FlatParams), whose gradients the backward kernels
write in place.  Both modes launch the same kernels on the same operands,
so everything a kernel computes without atomics must come out bit-equal;
what goes through an fp32-atomics reduction is one sum taken in two orders
and gets the pair bound of _gpu_bounds._check_pair."""

import pytest
import torch

from _gpu_bounds import _check_pair

pytestmark = pytest.mark.gpu

P = 0.3


def _rn(g, *shape, scale=1.0):
    return (torch.randn(*shape, device="cuda", generator=g) * scale).bfloat16()


def _run_mode(call, inputs, params, flat_names, dy):
    """One forward + backward on fresh leaf copies.  Parameters named in
    `flat_names` carry a zeroed `_flat_grad` and a ready-callback counter.
    Returns (y, dy, {name: grad}, {flat name: ready count})."""
    from transformer_amd.ops import functional as F
    ins = {n: t.clone().requires_grad_() if t.is_floating_point() else t
           for n, t in inputs.items()}
    ps = {n: None if t is None else t.clone().requires_grad_()
          for n, t in params.items()}
    flat_ps = {n: ps[n] for n in flat_names if ps[n] is not None}
    for p in flat_ps.values():
        p._flat_grad = torch.zeros_like(p)
    counts = {n: 0 for n in flat_ps}
    by_id = {id(p): n for n, p in flat_ps.items()}

    def ready(p):
        counts[by_id[id(p)]] += 1
    F.set_grad_ready_callback(flat_ps.values(), ready)
    try:
        torch.manual_seed(11)
        y = call(ins, ps)
        if dy is None:
            g = torch.Generator(device="cuda").manual_seed(12)
            dy = _rn(g, *y.shape)
        y.backward(dy)
    finally:
        F.set_grad_ready_callback(flat_ps.values(), None)
    torch.cuda.synchronize()
    grads = {n: t.grad for n, t in ins.items() if t.is_floating_point()}
    for n, p in ps.items():
        if p is None:
            continue
        if n in flat_ps:
            assert p.grad is None, f"{n}: flat parameter got a .grad"
            grads[n] = p._flat_grad
        else:
            grads[n] = p.grad
    assert all(v is not None for v in grads.values()), \
        [n for n, v in grads.items() if v is None]
    return y.detach(), dy, grads, counts


def _parity(call, inputs, params, atomic, flat_names=None):
    """Plain run, then flat run; `atomic` names the gradients that come out
    of an fp32-atomics reduction (pair bound), the rest must be bit-equal."""
    flat_names = list(params) if flat_names is None else flat_names
    y0, dy, g0, _ = _run_mode(call, inputs, params, (), None)
    y1, _, g1, counts = _run_mode(call, inputs, params, flat_names, dy)
    assert torch.equal(y0, y1), "forward differs between the modes"
    assert set(g0) == set(g1)
    for n in g0:
        assert g0[n].shape == g1[n].shape, n
        if n in atomic:
            _check_pair(g0[n], g1[n], n)
        else:
            assert torch.equal(g0[n], g1[n]), f"{n} not bit-equal"
    expect = {n: 1 for n in flat_names if params[n] is not None}
    assert counts == expect, counts


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("activation", [None, "relu"])
@pytest.mark.parametrize("M,K,N", [
    (64, 128, 192),      # dX falls through to the library matmul
    (2048, 128, 128),    # smallest shape on the cached-W^T "wt" dX backend
])
def test_linear(M, K, N, activation, bias):
    from transformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + N)
    inputs = {"x": _rn(g, M, K)}
    params = {"w": _rn(g, N, K, scale=K ** -0.5),
              "b": _rn(g, N, scale=0.1) if bias else None}

    def call(i, p):
        return ops.linear(i["x"], p["w"], p["b"], activation=activation)
    # y: gemm_nt -> 128-tile kernel, K = 128 < 4*BK so no split-K; plain
    #    stores.  relu_bwd is element-wise.
    # x: (64,128,192) torch.matmul, one output tile, no split;
    #    (2048,128,128) gemm_nt against the cached W^T, contraction 128,
    #    again below the split-K threshold.  Bit-equal.
    # w: gemm_dw writes disjoint per-slice partials and reduces them in a
    #    fixed order -- no atomics.  Bit-equal.
    # b: colsum, fp32 atomicAdd per (column, 128-row chunk).  Pair bound.
    _parity(call, inputs, params, atomic={"b"})


@pytest.mark.parametrize("drop", [False, True])
def test_residual_layernorm(drop):
    from transformer_amd import ops
    rows, d = 48, 128
    g = torch.Generator(device="cuda").manual_seed(rows + d + drop)
    inputs = {"x": _rn(g, rows, d), "res": _rn(g, rows, d)}
    params = {"gamma": _rn(g, d), "beta": _rn(g, d, scale=0.1)}

    def call(i, p):
        if drop:
            return ops.dropout_residual_layernorm(
                i["x"], i["res"], p["gamma"], p["beta"], P, True)
        return ops.residual_layernorm(i["x"], i["res"], p["gamma"],
                                      p["beta"])
    # y, x, res: ln_fwd / ln_bwd work row by row (the dropout mask comes
    #   from the one host seed draw, the same under the same manual_seed).
    #   Bit-equal.
    # gamma, beta: per-block column partials added with fp32 atomics into
    #   the workspace.  Pair bound.
    _parity(call, inputs, params, atomic={"gamma", "beta"})


def test_embedding_scale_pe():
    from transformer_amd import ops
    V, d, B, S = 50, 128, 2, 8
    g = torch.Generator(device="cuda").manual_seed(V)
    tokens = torch.randint(1, V, (B, S), device="cuda", generator=g)
    tokens[0, 3] = tokens[1, 5] = tokens[0, 0]   # one id three times
    pe = _rn(g, S + 4, d)
    inputs = {"tokens": tokens}
    params = {"weight": _rn(g, V, d)}

    def call(i, p):
        return ops.embedding_scale_pe(i["tokens"], p["weight"], pe)
    # y: a gather.  Bit-equal.
    # weight: scatter-add with fp32 atomics into a workspace, then a cast
    #   (into the flat view in flat mode).  Pair bound.
    _parity(call, inputs, params, atomic={"weight"})


def test_mixed_flat_falls_back_to_separate_ops():
    """Only `w` flat: linear_dropout_residual_layernorm runs the flat linear
    followed by the plain dropout_residual_layernorm, against the one-node
    composite of the all-plain run.  No linear bias: linear() takes its mode
    from `w` alone, so a plain bias beside a flat weight has nowhere to put
    its gradient."""
    from transformer_amd import ops
    rows, k, d = 48, 128, 128
    g = torch.Generator(device="cuda").manual_seed(rows)
    inputs = {"x": _rn(g, rows, k), "res": _rn(g, rows, d)}
    params = {"w": _rn(g, d, k, scale=k ** -0.5),
              "gamma": _rn(g, d), "beta": _rn(g, d, scale=0.1)}

    def call(i, p):
        return ops.linear_dropout_residual_layernorm(
            i["x"], p["w"], None, i["res"], p["gamma"], p["beta"], P, True)
    # Same kernels on the same operands in both runs (gemm_nt, ln_fwd with
    # the one seed draw; ln_bwd, torch.matmul for dX at 48 rows, gemm_dw):
    # y, x, res and w bit-equal; gamma / beta atomics-ordered as above.
    _parity(call, inputs, params, atomic={"gamma", "beta"},
            flat_names=["w"])
