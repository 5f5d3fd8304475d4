"""csrc/beam_search.hip: beam_topk against fp64, its tie rule and ticket
reset, beam_gather_kv exactly, beam_search_decode by tie-proof invariants.
A score is s_prev + x - lse and a relative error d in the fp32 sum l moves
log l by d, so tol = 1e-5 * (1 + |s_prev| + |x| + |lse|)."""

import pytest
import torch

from tests._gpu_bounds import _check_lim

pytestmark = pytest.mark.gpu

NINF = float("-inf")


@pytest.mark.parametrize("V,K,nchunk", [(202, 4, 0), (4099, 3, 0),
                                        (4099, 8, 5), (32002, 4, 0)])
def test_beam_topk_fp64(V, K, nchunk):
    """B = 2.  Sentence 0's last beam is finished (prior score 0, the best
    there is; its logits are 1e30, so reading them would take over the
    selection), sentence 1's first beam is dead."""
    from transformer_amd import ops
    B = 2
    g = torch.Generator().manual_seed(V + K)
    logits = (torch.randn(B * K, V, generator=g) * 4).to(torch.bfloat16).cuda()
    scores = (-5 * torch.rand(B, K, generator=g)).cuda()
    lens = torch.randint(1, 9, (B, K), generator=g).int().cuda()
    end_id = 5                     # (beam 0, end_id) of sentence 0 must win:
    logits[0, end_id] = 40.0       # log-prob ~ 0 on a prior of -0.25
    scores[0, 0] = -0.25
    finished = torch.zeros(B, K, dtype=torch.uint8, device="cuda")
    finished[0, K - 1] = 1
    scores[0, K - 1] = 0.0
    logits[K - 1] = 1e30
    scores[1, 0] = NINF
    ws = ops.beam_search_workspace(B, K, V, "cuda", nchunk)
    tok, parent, src_row, sc, fin, ln = ops.beam_topk(
        logits, scores, finished, lens, end_id, ws, nchunk)
    torch.cuda.synchronize()
    assert tok.shape == (B * K, 1) and tok.dtype == torch.int64
    tok, parent = tok.view(B, K), parent.long()

    x = logits.double().view(B, K, V)
    lse = torch.logsumexp(x, dim=-1, keepdim=True)
    s = scores.double()[:, :, None]
    full = s + (x - lse)                       # dead row: -inf throughout
    tol = 1e-5 * (1 + s.abs() + x.abs() + lse.abs())
    full[0, K - 1] = NINF
    full[0, K - 1, 0] = scores[0, K - 1]
    full, tol = full.view(B, K * V), tol.view(B, K * V)
    flat = parent * V + tok
    # each score against the fp64 score of its own (parent, token)
    _check_lim(sc, full.gather(1, flat), tol.gather(1, flat), "own score")
    # the selection compares computed scores, and the fp64 K-th best's
    # computed score is within ITS tol of it
    kth = full.topk(K, dim=1)
    floor = kth.values[:, -1:] - tol.gather(1, kth.indices[:, -1:])
    assert bool((sc.double() >= floor).all()), (sc, floor)
    assert bool((sc[:, :-1] >= sc[:, 1:]).all()), sc
    assert all(len(set(row)) == K for row in flat.tolist()), flat
    # the finished beam: once, token 0, score bit-unchanged; the dead: never
    hit = parent[0] == K - 1
    assert int(hit.sum()) == 1 and int(tok[0][hit]) == 0
    assert torch.equal(sc[0][hit], scores[0, K - 1:])
    assert not bool((parent[1] == 0).any())
    # state carried consistently with (parent, token)
    pfin = finished.gather(1, parent).bool()
    assert torch.equal(fin.bool(), pfin | (tok == end_id))
    assert bool(fin.any()) and not bool(fin.all())
    assert torch.equal(ln, lens.gather(1, parent) + (~pfin).int())
    rows = torch.arange(B, device="cuda")[:, None] * K + parent
    assert torch.equal(src_row.long(), rows.view(-1))


@pytest.mark.parametrize("V", [2, 50])
def test_beam_topk_ties_and_ticket_reset(V):
    """All logits equal, prior scores [0, 0, -inf, -inf]: the winners are the
    four lowest flat indices k*V + v of beams 0 and 1, in that order (V = 2:
    tokens 0, 1, 0, 1 from parents 0, 0, 1, 1).  Then three replays of a
    captured call with nchunk forced to 3 are bit-identical to the eager
    result: each merge re-zeroes its ticket."""
    from transformer_amd import ops
    B, K = 2, 4
    logits = torch.ones(B * K, V, dtype=torch.bfloat16, device="cuda")
    scores = torch.tensor([[0.0, 0.0, NINF, NINF]] * B, device="cuda")
    finished = torch.zeros(B, K, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(B, K, dtype=torch.int32, device="cuda")
    want = [k * V + v for k in (0, 1) for v in range(V)][:K]
    outs = {}
    for nchunk in (0, 3):
        ws = ops.beam_search_workspace(B, K, V, "cuda", nchunk)
        outs[nchunk] = ops.beam_topk(logits, scores, finished, lens, V + 1,
                                     ws, nchunk)
        tok, parent = outs[nchunk][:2]
        assert tok.view(B, K).tolist() == [[f % V for f in want]] * B
        assert parent.tolist() == [[f // V for f in want]] * B
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ops.beam_topk(logits, scores, finished, lens, V + 1, ws, 3)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(cap, outs[3]):
            assert torch.equal(got, ref)


@pytest.mark.parametrize("HD", [64, 512])
@pytest.mark.parametrize("kv_len", [[0] * 6, [36] * 6,
                                    [0, 49, 36, 7, 60, 1]])
def test_beam_gather_kv_exact(HD, kv_len):
    """2 layers, 6 rows, Lmax 50; the mixed lengths add a full row (49 + 1 =
    Lmax) and one past the end (clamped)."""
    from transformer_amd import ops
    rows, Lmax, src_row = 6, 50, [0, 0, 2, 5, 5, 3]
    g = torch.Generator().manual_seed(HD)
    src = [torch.randn(rows, Lmax, 2, 2, HD // 2, generator=g)
           .to(torch.bfloat16).cuda() for _ in range(2)]
    keep = [t.clone() for t in src]
    dst = [torch.full_like(t, 7.0) for t in src]
    ops.beam_gather_kv(src, dst,
                       torch.tensor(src_row, dtype=torch.int32, device="cuda"),
                       torch.tensor(kv_len, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for s, k, d in zip(src, keep, dst):
        assert torch.equal(s, k)
        for r, sr in enumerate(src_row):
            n = min(kv_len[sr] + 1, Lmax)
            assert torch.equal(d[r, :n], s[sr, :n]), (r, n)
            assert bool((d[r, n:] == 7.0).all()), (r, n)
    with pytest.raises(RuntimeError, match="distinct cache sets"):
        ops.beam_gather_table(src, [src[1], dst[0]])


@pytest.fixture(scope="module")
def seed3():
    """Model and inputs of test_fused_decode_matches_plain_greedy."""
    from transformer_amd.models import Transformer
    torch.manual_seed(3)
    model = Transformer(num_layers=2, d_model=128, num_heads=4, dff=256,
                        input_vocab_size=202, target_vocab_size=202,
                        rate=0.0, max_position=128).to("cuda", torch.bfloat16)
    model.eval()
    inp = torch.randint(2, 200, (2, 24), device="cuda")
    inp[1, 18:] = 0
    return model, inp


def test_beam_size_1_is_greedy(seed3):
    """Same kernels, same row count, same lowest-index tie rule as
    argmax_kernel: the tokens of greedy_decode(fused_attn=True) up to each
    row's end."""
    from transformer_amd.models.transformer import (beam_search_decode,
                                                    greedy_decode)
    model, inp = seed3
    ref = greedy_decode(model, inp, 200, 201, max_len=16, fused_attn=True)
    hyps, _ = beam_search_decode(model, inp, 200, 201, beam_size=1,
                                 max_len=16)
    for b in range(inp.shape[0]):
        pr, br = ref[b].tolist(), hyps[b, 0].tolist()
        for i in range(min(len(pr), len(br))):
            assert pr[i] == br[i], (b, i, pr, br)
            if pr[i] == 201:
                break


@pytest.mark.parametrize("skinny", [False, True])
def test_beam_4_scores_are_rescored(seed3, skinny):
    """Per sentence: 4 distinct hypotheses, scores non-increasing, and every
    score equals its hypothesis teacher-forced on a fresh cache of the same
    row count (same kernels, same NSPLIT): the fp64 log_softmax of its
    tokens summed up to and including end_id, within 1e-5 * sum_t (1 +
    |x_t| + |lse_t|).  Catches a wrong parent, a stale or shifted cache row."""
    from transformer_amd.models.transformer import (DecodeCache,
                                                    beam_search_decode,
                                                    decode_step, encode)
    model, inp = seed3
    K, max_len, end = 4, 16, 201
    hyps, scores = beam_search_decode(model, inp, 200, end, beam_size=K,
                                      max_len=max_len, skinny_linear=skinny)
    B, T = inp.shape[0], hyps.shape[2] - 1
    for b in range(B):
        assert len({tuple(h) for h in hyps[b].tolist()}) == K, hyps[b]
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), scores
    enc, pad = encode(model, inp)
    cache = DecodeCache(model, B * K, max_len + 1,
                        enc.repeat_interleave(K, dim=0),
                        pad.repeat_interleave(K, dim=0), fused_attn=True,
                        skinny_linear=skinny)
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
