"""linear_rows_preln (LayerNorm in the prologue of the decode linear that
consumes it) against fp64 references of the bf16 inputs, N(0,1) from a
seeded generator.

xn: with t = p + res in fp64, the kernel's fp32 t is within
e = 1e-5*(|p|+|res|) of it, and LayerNorm moves xhat by at most
2*rs*(1+|xhat|)*max_row(e) (test_gpu_linear_rows.py derives the form), so
_check_u(xn, xhat*g+b, |xhat*g|+|b|, extra = 2*rs*|g|*(1+|xhat|)*e_max).

y: against the kernel's OWN xn (its bf16 rounding is a discontinuity that
must stay out of the reference): ref = xn @ W^T + b in fp64,
absterm = |xn| @ |W|^T + |b|; ReLU is 1-Lipschitz.  The fused linear keeps
linear_rows' K split and sum order, so y is also bit-equal to
linear_rows(xn)."""

import pytest
import torch

from _gpu_bounds import _check_u

pytestmark = pytest.mark.gpu
EPS = 1e-6


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g).bfloat16()


@pytest.mark.parametrize("M,N,K,relu,bias", [
    (1, 202, 128, False, True),      # single row, N tail, more blocks than rows
    (17, 48, 520, True, True),       # 2nd group nearly empty, K % 64 != 0,
                                     # 3 blocks for 17 rows: XN owner wraps
    (33, 32, 1024, False, True),     # largest K, three live groups, 2 blocks
    (64, 130, 256, True, True),      # MG=4, N tail
    (3, 16, 8, False, False),        # one block, one K chunk, no bias
    (8, 1536, 512, False, True),     # the model's QKV shape
])
def test_linear_rows_preln_vs_fp64(M, N, K, relu, bias):
    from transformer_amd.ops import ext
    E, g = ext(), torch.Generator(device="cuda").manual_seed(M * 1000 + N)
    p, res, gamma, beta = (_randn(g, M, K), _randn(g, M, K), _randn(g, K),
                           _randn(g, K))
    w, b = _randn(g, N, K), _randn(g, N) if bias else None
    xn, y = E.linear_rows_preln(p, res, gamma, beta, EPS, w, b, relu)
    name = f"linear_rows_preln {M}x{N}x{K}"

    t = p.double() + res.double()
    e_max = (1e-5 * (p.double().abs() + res.double().abs())) \
        .amax(dim=1, keepdim=True)
    rs = (t.var(dim=1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xhat = (t - t.mean(dim=1, keepdim=True)) * rs
    gd, bd = gamma.double(), beta.double()
    _check_u(xn, xhat * gd + bd, (xhat * gd).abs() + bd.abs(), name + " xn",
             extra=2 * rs * gd.abs() * (1 + xhat.abs()) * e_max)

    ref = xn.double() @ w.double().T
    at = xn.double().abs() @ w.double().abs().T
    if bias:
        ref, at = ref + b.double(), at + b.double().abs()
    _check_u(y, ref.relu() if relu else ref, at, name + " y")
    assert torch.equal(y, E.linear_rows(xn, w, b, relu))
    xn2, y2 = E.linear_rows_preln(p, res, gamma, beta, EPS, w, b, relu)
    assert torch.equal(xn, xn2) and torch.equal(y, y2)


@pytest.mark.parametrize("fused_attn", [False, True])
def test_skinny_preln_decode_matches_plain_greedy(fused_attn):
    """Model and inputs of test_skinny_decode_matches_plain_greedy (seed 3):
    graphed and eager decode with every LayerNorm in its consumer's prologue
    emit plain greedy_decode's tokens up to each row's end."""
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
                         skinny_linear=True, skinny_preln=True)
    outs = {"graphed": dec(inp, end, max_len=max_len),
            "eager": greedy_decode(model, inp, start, end, max_len=max_len,
                                   fused_attn=fused_attn, skinny_linear=True,
                                   skinny_preln=True)}
    for name, out in outs.items():
        for b in range(B):
            pr, fr = plain[b].tolist(), out[b].tolist()
            for i in range(min(len(pr), len(fr))):
                assert pr[i] == fr[i], (name, b, i, pr, fr)
                if pr[i] == end:
                    break
    assert torch.equal(outs["graphed"], dec(inp, end, max_len=max_len))
