"""Beam decode attention (decode_attn.hip beam kernels) against fp64 softmax
attention, beam_reindex exactly, beam_search_decode(indirect_kv=True) by
re-scoring.  Bound as test_gpu_decode_attn.py: 2^-8*|ref| + 1e-5*absterm,
absterm = sum_j p_j*|v_j| in fp64: the same fp32 state, rounded once."""

import math

import pytest
import torch

from tests._gpu_bounds import _check_lim, _check_pair, _check_u

pytestmark = pytest.mark.gpu


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g).bfloat16()


def _ref(q, k, v, live=None):
    """q (H,dh), k/v (n,H,dh) -> fp64 (ref, absterm), each (H,dh)."""
    q, k, v = q.double(), k.double(), v.double()
    if live is not None:
        k, v = k[live], v[live]
    s = torch.einsum("hd,nhd->hn", q, k) / math.sqrt(q.shape[-1])
    p = torch.softmax(s, dim=-1)
    return (torch.einsum("hn,nhd->hd", p, v),
            torch.einsum("hn,nhd->hd", p, v.abs()))


@pytest.mark.parametrize("lens", [[64, 130], [0, 63], [200, 130]])
@pytest.mark.parametrize("dh,K", [(32, 8), (64, 3), (128, 2), (64, 1)])
def test_self_beam_vs_fp64(dh, K, lens):
    """Table random in [0, K) below kv_len and 255 from there on; cache 1e30
    from kv_len on, so a stray read shows.  [200, 130]: sentence 0 is full
    (nothing stored, Lmax cached keys through the table plus the new one)."""
    E, g = _ext(), torch.Generator(device="cuda").manual_seed(dh + K)
    B, H, Lmax, Lt = 2, 2, 200, 208
    R = B * K
    row_len = [lens[r // K] for r in range(R)]
    qkv, cache0 = _randn(g, R, 1, 3, H, dh), _randn(g, R, Lmax, 2, H, dh)
    origin = torch.randint(0, K, (R, Lt), device="cuda", generator=g,
                           dtype=torch.uint8)
    for r, n in enumerate(row_len):
        cache0[r, n:] = 1e30
        origin[r, n:] = 255
    kv_len = torch.tensor(row_len, dtype=torch.int32, device="cuda")
    ws = E.decode_attn_beam_workspace(B, K, H, dh, 1024)
    outs = []
    for nsplit in (1, 3):
        cache = cache0.clone()
        o = E.decode_attn_self_beam(qkv, cache, kv_len, origin, K, ws,
                                    dh ** -0.5, nsplit)
        assert kv_len.tolist() == row_len
        want = cache0.clone()
        for r, n in enumerate(row_len):
            if n < Lmax:
                want[r, n] = qkv[r, 0, 1:3]
            src = r // K * K + origin[r, :n].long()
            kv = torch.cat([cache0[src, torch.arange(n, device="cuda")],
                            qkv[r, :, 1:3]])
            ref, at = _ref(qkv[r, 0, 0], kv[:, 0], kv[:, 1])
            _check_u(o[r, 0], ref, at, f"self dh{dh} K{K} ns{nsplit} row{r}")
        assert torch.equal(cache, want)   # append bitwise, the rest untouched
        # _check_pair puts |sum| in place of sum|terms|, which holds only
        # where the terms share a sign (an element that cancels to 1.7e-6
        # against absterm 0.73 differs by 3e-8 between the split counts, 250
        # times inside the fp64 bound and twice outside the pair bound): the
        # pair is taken on the same keys, queries and table with V >= 0
        qkv_p, cache_p = qkv.clone(), cache0.clone()
        qkv_p[:, :, 2].abs_()
        cache_p[:, :, 1].abs_()
        outs.append(E.decode_attn_self_beam(qkv_p, cache_p, kv_len, origin, K,
                                            ws, dh ** -0.5, nsplit))
    _check_pair(outs[0], outs[1], f"self beam dh{dh} K{K} split vs single")


def _cross_case(dh, K):
    g = torch.Generator(device="cuda").manual_seed(100 + dh + K)
    B, H, Sk = 3, 2, 150
    q = _randn(g, B * K, 1, 3, H, dh)[:, :, 0]          # strided view
    kv = _randn(g, B, Sk, 2, H, dh)
    pad = torch.zeros(B, Sk, dtype=torch.uint8, device="cuda")
    pad[1, Sk - 37:] = 1
    pad[2] = 1
    return q, kv, pad, _ext().decode_attn_beam_workspace(B, K, H, dh, 1024)


@pytest.mark.parametrize("nsplit", [0, 3])
@pytest.mark.parametrize("dh,K", [(64, 2), (64, 3), (128, 8), (32, 8)])
def test_cross_beam_vs_fp64(dh, K, nsplit):
    q, kv, pad, ws = _cross_case(dh, K)
    o = _ext().decode_attn_cross_beam(q, kv, pad, K, ws, dh ** -0.5, nsplit)
    assert o.shape == (3 * K, 1, 2, dh)
    for r in range(3 * K):
        b = r // K
        if b == 2:     # all scores collapse to -1e9 in fp32: the mean of V
            v = kv[b, :, 1].double()
            ref, at = v.mean(0), v.abs().mean(0)
        else:
            ref, at = _ref(q[r, 0], kv[b, :, 0], kv[b, :, 1], pad[b] == 0)
        _check_u(o[r, 0], ref, at, f"cross dh{dh} K{K} ns{nsplit} row{r}")


def test_cross_beam_graph_replay():
    """Three replays of a captured 3-split call are bit-equal to the eager
    call: the last arriver re-zeroes its ticket."""
    E, (q, kv, pad, ws) = _ext(), _cross_case(64, 4)
    eager = E.decode_attn_cross_beam(q, kv, pad, 4, ws, 0.125, 3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = E.decode_attn_cross_beam(q, kv, pad, 4, ws, 0.125, 3)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager)


@pytest.mark.parametrize("kv_before", [[0] * 6, [36] * 6,
                                       [49, 49, 49, 60, 60, 60]])
def test_beam_reindex_exact(kv_before):
    from transformer_amd import ops
    K, Lmax, Lt, src_row = 3, 50, 64, [0, 0, 2, 5, 5, 3]
    g = torch.Generator().manual_seed(5)
    tin = torch.randint(0, K, (6, Lt), generator=g, dtype=torch.uint8).cuda()
    keep, tout = tin.clone(), torch.full_like(tin, 7)
    dev = dict(dtype=torch.int32, device="cuda")
    ops.beam_reindex(tin, tout, torch.tensor(src_row, **dev),
                     torch.tensor(kv_before, **dev), K, Lmax)
    torch.cuda.synchronize()
    assert torch.equal(tin, keep)
    for r, sr in enumerate(src_row):
        n = min(kv_before[sr], Lmax)
        assert torch.equal(tout[r, :n], tin[sr, :n]), (r, n)
        if n < Lmax:
            assert int(tout[r, n]) == sr % K, (r, n)
        assert bool((tout[r, n + (n < Lmax):] == 7).all()), (r, n)
    with pytest.raises(RuntimeError, match="distinct tables"):
        ops.beam_reindex(tin, tin, torch.tensor(src_row, **dev),
                         torch.tensor(kv_before, **dev), K, Lmax)


@pytest.fixture(scope="module")
def seed3():
    """Model and inputs of test_gpu_beam_search.py."""
    from transformer_amd.models import Transformer
    torch.manual_seed(3)
    model = Transformer(num_layers=2, d_model=128, num_heads=4, dff=256,
                        input_vocab_size=202, target_vocab_size=202,
                        rate=0.0, max_position=128).to("cuda", torch.bfloat16)
    model.eval()
    inp = torch.randint(2, 200, (2, 24), device="cuda")
    inp[1, 18:] = 0
    return model, inp


def test_indirect_beam_size_1_is_greedy(seed3):
    from transformer_amd.models.transformer import (beam_search_decode,
                                                    greedy_decode)
    model, inp = seed3
    ref = greedy_decode(model, inp, 200, 201, max_len=16, fused_attn=True)
    hyps, _ = beam_search_decode(model, inp, 200, 201, beam_size=1,
                                 max_len=16, indirect_kv=True)
    for b in range(inp.shape[0]):
        pr, br = ref[b].tolist(), hyps[b, 0].tolist()
        for i in range(min(len(pr), len(br))):
            assert pr[i] == br[i], (b, i, pr, br)
            if pr[i] == 201:
                break


@pytest.mark.parametrize("skinny", [False, True])
def test_indirect_beam_4_scores_are_rescored(seed3, skinny):
    """As test_beam_4_scores_are_rescored, through the origin tables: every
    hypothesis is teacher-forced on a fresh indirect cache whose table is the
    identity (origin[r, j] = r % K: each row reads itself), which runs the
    same kernels at the same row count and NSPLIT.  Bound 1e-5 * sum_t (1 +
    |x_t| + |lse_t|).  A wrong table entry, a stale row or a shifted
    position changes the history a row attends and breaks it."""
    from transformer_amd.models.transformer import (DecodeCache,
                                                    beam_search_decode,
                                                    decode_step, encode)
    model, inp = seed3
    K, max_len, end = 4, 16, 201
    hyps, scores = beam_search_decode(model, inp, 200, end, beam_size=K,
                                      max_len=max_len, skinny_linear=skinny,
                                      indirect_kv=True)
    B, T = inp.shape[0], hyps.shape[2] - 1
    for b in range(B):
        assert len({tuple(h) for h in hyps[b].tolist()}) == K, hyps[b]
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), scores
    enc, pad = encode(model, inp)
    cache = DecodeCache(model, B * K, max_len + 1, enc, pad, fused_attn=True,
                        skinny_linear=skinny, beam_size=K, indirect_kv=True)
    assert len(cache.cross_kv[0]) == B and cache.self_kv_alt is None
    cache.origin[:] = (torch.arange(B * K, device="cuda") % K)[:, None]
    rows = hyps.view(B * K, T + 1)
    total = torch.zeros(B * K, dtype=torch.float64, device="cuda")
    bound = torch.zeros_like(total)
    alive = torch.ones_like(total)
    for t in range(T):
        lg = decode_step(model, rows[:, t:t + 1], cache)[:, 0].double()
        lse = torch.logsumexp(lg, dim=-1)
        x = lg.gather(1, rows[:, t + 1:t + 2]).squeeze(1)
        total += alive * (x - lse)
        bound += alive * 1e-5 * (1 + x.abs() + lse.abs())
        alive *= (rows[:, t + 1] != end).double()
    _check_lim(scores.view(-1), total, bound, f"re-score skinny={skinny}")
