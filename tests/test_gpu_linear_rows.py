"""Skinny-M decode linears (linear_rows.hip) against fp64 references of the
bf16 inputs, N(0,1) from a seeded generator.

linear_rows: ref = X @ W^T + b in fp64, absterm = |X| @ |W|^T + |b|;
_check_u = 2^-8*|ref| + 1e-5*absterm (one bf16 rounding of an fp32 sum).
ReLU is 1-Lipschitz, so the pre-activation bound carries over.

linear_rows_ln: with t = X @ W^T + b + res in fp64 and
at = |X| @ |W|^T + |b| + |res|, the kernel's fp32 t is within e = 1e-5*at of
it.  To first order LayerNorm moves xhat by at most
2*rs*(1+|xhat|)*max_row(e): the centred value t - mean moves by at most
2*e_max, and rs moves relatively by at most 2*e_max*rs because
mean|t - m| <= sigma.  So the check is
_check_u(y, xhat*g+b, |xhat*g|+|b|, extra = 2*rs*|g|*(1+|xhat|)*e_max)."""

import pytest
import torch

from _gpu_bounds import _check_u

pytestmark = pytest.mark.gpu
EPS = 1e-6


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g).bfloat16()


@pytest.mark.parametrize("M,N,K,relu,bias", [
    (1, 202, 128, False, True),      # N tail, single row
    (16, 512, 520, True, True),      # K not a multiple of 32
    (17, 48, 2048, False, True),     # 2nd row group nearly empty, deep K
    (64, 130, 256, True, True),      # MG=4 plus N tail
    (3, 16, 8, False, False),        # one chunk, no bias, most waves idle
    (8, 1536, 512, False, True),     # the model's QKV shape
    (1, 512, 2048, False, True),     # ffn.w2 in a decode step: 8 waves, MG=1
    (64, 32, 2048, True, True),      # 8 waves with MG=4
])
def test_linear_rows_vs_fp64(M, N, K, relu, bias):
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(M * 1000 + N)
    x, w = _randn(g, M, K), _randn(g, N, K)
    b = _randn(g, N) if bias else None
    ref = x.double() @ w.double().T
    at = x.double().abs() @ w.double().abs().T
    if bias:
        ref, at = ref + b.double(), at + b.double().abs()
    y = E.linear_rows(x, w, b, relu)
    _check_u(y, ref.relu() if relu else ref, at, f"linear_rows {M}x{N}x{K}")
    assert torch.equal(y, E.linear_rows(x, w, b, relu))   # fixed order


def _ln_inputs(g, M, N, K):
    return (_randn(g, M, K), _randn(g, N, K), _randn(g, N), _randn(g, M, N),
            _randn(g, N), _randn(g, N))


def _check_ln(y, x, w, b, res, gamma, beta, name):
    x, w, b, res, gamma, beta = (t.double() for t in (x, w, b, res, gamma,
                                                     beta))
    t = x @ w.T + b + res
    e_max = (1e-5 * (x.abs() @ w.abs().T + b.abs() + res.abs())) \
        .amax(dim=1, keepdim=True)
    rs = (t.var(dim=1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xhat = (t - t.mean(dim=1, keepdim=True)) * rs
    _check_u(y, xhat * gamma + beta, (xhat * gamma).abs() + beta.abs(), name,
             extra=2 * rs * gamma.abs() * (1 + xhat.abs()) * e_max)


@pytest.mark.parametrize("M,N,K", [(1, 128, 128), (16, 512, 2048),
                                   (33, 130, 264)])
def test_linear_rows_ln_vs_fp64(M, N, K):
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(M + N + K)
    args = _ln_inputs(g, M, N, K)
    ws = E.linear_rows_workspace(64, 512)     # larger than any case
    for run in range(2):      # the second run needs the ticket re-zeroed
        y = E.linear_rows_ln(*args, EPS, ws)
        _check_ln(y, *args, f"linear_rows_ln {M}x{N}x{K} run{run}")


def test_linear_rows_ln_graph_replay():
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(11)
    M, N, K = 8, 512, 512
    x, w, b, res, gamma, beta = _ln_inputs(g, M, N, K)
    xs = _randn(g, 3, M, K)
    ws = E.linear_rows_workspace(M, N)
    E.linear_rows_ln(x, w, b, res, gamma, beta, EPS, ws)      # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = E.linear_rows_ln(x, w, b, res, gamma, beta, EPS, ws)
    for r in range(3):
        x.copy_(xs[r])
        graph.replay()
        _check_ln(y, xs[r], w, b, res, gamma, beta, f"replay {r}")


@pytest.mark.parametrize("skinny_ln", [False, True])
@pytest.mark.parametrize("fused_attn", [False, True])
def test_skinny_decode_matches_plain_greedy(fused_attn, skinny_ln):
    """Model and inputs of test_fused_decode_matches_plain_greedy (seed 3):
    both skinny-linear paths emit plain greedy_decode's tokens up to each
    row's end, alone and together with fused_attn, with the LayerNorms
    separate and fused (skinny_ln)."""
    from transformer_amd.models import Transformer
    from transformer_amd.models.transformer import (GraphedDecoder,
                                                    greedy_decode)
    torch.manual_seed(3)
    model = Transformer(num_layers=2, d_model=128, num_heads=4, dff=256,
                        input_vocab_size=202, target_vocab_size=202,
                        rate=0.0, max_position=128).to("cuda", torch.bfloat16)
    model.eval()
    B, S, max_len, start, end = 2, 24, 16, 200, 201
    inp = torch.randint(2, 200, (B, S), device="cuda")
    inp[1, 18:] = 0
    plain = greedy_decode(model, inp, start, end, max_len=max_len)
    dec = GraphedDecoder(model, B=B, S_src=S, max_len=max_len, start_id=start,
                         device=torch.device("cuda"), fused_attn=fused_attn,
                         skinny_linear=True, skinny_ln=skinny_ln)
    outs = {"graphed": dec(inp, end, max_len=max_len),
            "eager": greedy_decode(model, inp, start, end, max_len=max_len,
                                   fused_attn=fused_attn, skinny_linear=True,
                                   skinny_ln=skinny_ln)}
    for name, out in outs.items():
        for b in range(B):
            pr, fr = plain[b].tolist(), out[b].tolist()
            for i in range(min(len(pr), len(fr))):
                assert pr[i] == fr[i], (name, b, i, pr, fr)
                if pr[i] == end:
                    break
    assert torch.equal(outs["graphed"], dec(inp, end, max_len=max_len))
