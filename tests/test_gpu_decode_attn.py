"""Single-query decode attention (decode_attn.hip) against fp64 softmax
attention of the bf16 inputs.

Bound, element-wise: _check_u(o, ref, absterm) = 2^-8*|ref| + 1e-5*absterm
with absterm = sum_j p_j*|v_j| in fp64.  The kernel keeps scores, softmax
state and the accumulator in fp32 and rounds once to bf16: the u term is
that rounding, and the fp32 work (scores, exp, split recombination through
(m, l)) stays near 3e-7*absterm for N(0,1) inputs at these lengths."""

import math

import pytest
import torch

from _gpu_bounds import _check_pair, _check_u

pytestmark = pytest.mark.gpu


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g).bfloat16()


def _ref(q, k, v, live=None):
    """q (H,dh), k/v (n,H,dh) -> fp64 (ref, absterm), each (H,dh); live (n,)
    bool drops keys (a padded key's fp32 weight is exactly 0)."""
    q, k, v = q.double(), k.double(), v.double()
    if live is not None:
        k, v = k[live], v[live]
    s = torch.einsum("hd,nhd->hn", q, k) / math.sqrt(q.shape[-1])
    p = torch.softmax(s, dim=-1)
    return (torch.einsum("hn,nhd->hd", p, v),
            torch.einsum("hn,nhd->hd", p, v.abs()))


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_self_vs_fp64(dh):
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(dh)
    B, H, Lmax, lens = 4, 2, 600, [0, 63, 64, 257]
    qkv, cache0 = _randn(g, B, 1, 3, H, dh), _randn(g, B, Lmax, 2, H, dh)
    kv_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ws = E.decode_attn_workspace(B, H, dh, Lmax)
    assert E.decode_attn_nsplit(B * H, Lmax) >= 2
    outs = []
    for nsplit in (0, 1):      # 0: the production rule
        cache = cache0.clone()
        o = E.decode_attn_self(qkv, cache, kv_len, ws, dh ** -0.5, nsplit)
        assert kv_len.tolist() == lens
        want = cache0.clone()
        for b, n in enumerate(lens):
            want[b, n] = qkv[b, 0, 1:3]
            ref, at = _ref(qkv[b, 0, 0], want[b, :n + 1, 0], want[b, :n + 1, 1])
            _check_u(o[b, 0], ref, at, f"self dh{dh} nsplit{nsplit} n{n}")
        assert torch.equal(cache, want)   # append bitwise, the rest untouched
        outs.append(o)
    _check_pair(outs[0], outs[1], f"self dh{dh} split vs single")


@pytest.mark.parametrize("nsplit", [0, 3])     # the host rule; three splits
@pytest.mark.parametrize("dh", [64, 128])
def test_cross_vs_fp64(dh, nsplit):
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(100 + dh)
    B, H, Sk = 3, 2, 150
    q = _randn(g, B, 1, 3, H, dh)[:, :, 0]          # strided view
    kv = _randn(g, B, Sk, 2, H, dh)
    pad = torch.zeros(B, Sk, dtype=torch.uint8, device="cuda")
    pad[1, Sk - 37:] = 1
    pad[2] = 1
    ws = E.decode_attn_workspace(B, H, dh, 1024)   # room for 3 splits
    o = E.decode_attn_cross(q, kv, pad, ws, dh ** -0.5, nsplit)
    for b in range(B):
        if b == 2:     # all scores collapse to -1e9 in fp32: the mean of V
            v = kv[b, :, 1].double()
            ref, at = v.mean(0), v.abs().mean(0)
        else:
            ref, at = _ref(q[b, 0], kv[b, :, 0], kv[b, :, 1], pad[b] == 0)
        _check_u(o[b, 0], ref, at, f"cross dh{dh} nsplit{nsplit} row{b}")


def test_graph_replay_device_length():
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(7)
    B, H, dh, Lmax, R = 2, 2, 64, 128, 70
    rows = _randn(g, R, B, 1, 3, H, dh)
    qkv = rows[0].clone()
    cache = _randn(g, B, Lmax, 2, H, dh)
    kv_len = torch.zeros(B, dtype=torch.int32, device="cuda")
    ws = E.decode_attn_workspace(B, H, dh, 512)
    # two splits forced: the ticket's self-reset is live across replays
    E.decode_attn_self(qkv, cache.clone(), kv_len, ws, dh ** -0.5, 2)  # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = E.decode_attn_self(qkv, cache, kv_len, ws, dh ** -0.5, 2)
        kv_len.add_(1)
    for r in range(1, R + 1):
        qkv.copy_(rows[r - 1])
        graph.replay()
        if r in (1, 64, 65, 70):
            assert kv_len.tolist() == [r] * B
            for b in range(B):
                ref, at = _ref(rows[r - 1, b, 0, 0], rows[:r, b, 0, 1],
                               rows[:r, b, 0, 2])
                _check_u(o[b, 0], ref, at, f"replay {r} row{b}")


def test_full_row_is_clamped():
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(9)
    B, H, dh, Lmax = 2, 2, 64, 70
    qkv, cache = _randn(g, B, 1, 3, H, dh), _randn(g, B, Lmax, 2, H, dh)
    before = cache.clone()
    kv_len = torch.tensor([Lmax, Lmax + 3], dtype=torch.int32, device="cuda")
    ws = E.decode_attn_workspace(B, H, dh, 512)
    o = E.decode_attn_self(qkv, cache, kv_len, ws, dh ** -0.5, 2)
    assert torch.equal(cache, before) and bool(torch.isfinite(o).all())
    for b in range(B):     # a full row attends its Lmax keys plus the new one
        kv = torch.cat([before[b], qkv[b, :, 1:3]])
        ref, at = _ref(qkv[b, 0, 0], kv[:, 0], kv[:, 1])
        _check_u(o[b, 0], ref, at, f"full row{b}")


def test_fused_decode_matches_plain_greedy():
    """Model and inputs of test_graphed_decode_matches_eager (seed 3): both
    fused paths emit plain greedy_decode's tokens up to each row's end."""
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
                         device=torch.device("cuda"), fused_attn=True)
    fused = {"graphed": dec(inp, end, max_len=max_len),
             "eager": greedy_decode(model, inp, start, end, max_len=max_len,
                                    fused_attn=True)}
    for name, out in fused.items():
        for b in range(B):
            pr, fr = plain[b].tolist(), out[b].tolist()
            for i in range(min(len(pr), len(fr))):
                assert pr[i] == fr[i], (name, b, i, pr, fr)
                if pr[i] == end:
                    break
    assert torch.equal(fused["graphed"], dec(inp, end, max_len=max_len))
