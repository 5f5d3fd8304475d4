"""CPU wiring of the skinny decode linears: the two ops against their
F.linear / reference.residual_layernorm compositions, and
greedy_decode(skinny_linear=True)."""

import torch
import torch.nn.functional as F

from transformer_amd import ops
from transformer_amd.ops import reference as R


def test_ops_match_reference_compositions():
    torch.manual_seed(0)
    x, w, b = torch.randn(2, 3, 16), torch.randn(24, 16), torch.randn(24)
    res, gamma, beta = torch.randn(2, 3, 24), torch.randn(24), torch.randn(24)
    ws = ops.linear_rows_workspace(6, 24, "cpu")
    assert ws.numel() == 0
    y = ops.linear_rows_residual_layernorm(x, w, b, res, gamma, beta, 1e-6,
                                           ws)
    assert torch.equal(y, R.residual_layernorm(F.linear(x, w, b), res, gamma,
                                               beta, 1e-6))
    assert torch.equal(ops.linear_rows(x, w, b, activation="relu"),
                       F.linear(x, w, b).relu())
    assert torch.equal(ops.linear_rows(x, w), F.linear(x, w))


def test_greedy_decode_skinny_linear_cpu():
    from transformer_amd.models import Transformer
    from transformer_amd.models.transformer import greedy_decode

    torch.manual_seed(3)
    model = Transformer(num_layers=2, d_model=32, num_heads=4, dff=64,
                        input_vocab_size=52, target_vocab_size=52, rate=0.0,
                        max_position=32)
    model.eval()
    inp = torch.randint(2, 50, (2, 9))
    inp[1, 6:] = 0
    plain = greedy_decode(model, inp, 50, 51, max_len=8)
    for fused_attn in (False, True):
        skinny = greedy_decode(model, inp, 50, 51, max_len=8,
                               fused_attn=fused_attn, skinny_linear=True,
                               skinny_ln=fused_attn)
        assert torch.equal(plain, skinny)
