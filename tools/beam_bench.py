"""Beam-search kernels (beam_search.hip) against the ATen composites they
replace, and beam_search_decode end to end.

Kernels: device events around a replayed graph of ITERS calls, best of 3,
kernel and composite alternated in one process.  beam_topk at V = 32002 and
K = 4 against log_softmax + add + topk + index arithmetic (which leaves the
finished / dead handling out, in the composite's favour); beam_gather_kv at
6 layers, d 512 against index_select + copy_ per layer on the [:n] slice (n
known on the host, which the kernel does not need).

    python tools/beam_bench.py            # kernels
    python tools/beam_bench.py --indirect # the no-copy beam kernels
    python tools/beam_bench.py --e2e      # eager ms/token, beam 4 (cache
                                          # copies | indirect_kv) vs greedy
    python tools/beam_bench.py --one_beam # one beam decode (for a profiler)
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_amd import ops  # noqa: E402

ITERS = 200


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            fn()
    g.replay()
    return g


def time_pair_us(fa, fb):
    """Best of 3 replays each, a and b alternated."""
    graphs, best = (graph_of(fa), graph_of(fb)), [float("inf")] * 2
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for _ in range(3):
        for i, g in enumerate(graphs):
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            best[i] = min(best[i], a.elapsed_time(b) * 1e3 / ITERS)
    return best


def bench_kernels():
    V, K = 32002, 4
    for BK in (4, 16, 32, 64):
        B = BK // K
        logits = (torch.randn(BK, V, device="cuda") * 4).bfloat16()
        scores = -torch.rand(B, K, device="cuda")
        fin = torch.zeros(B, K, dtype=torch.uint8, device="cuda")
        lens = torch.ones(B, K, dtype=torch.int32, device="cuda")
        base = torch.arange(B, device="cuda")[:, None] * K
        ws = ops.beam_search_workspace(B, K, V, "cuda")

        def composite():
            lp = torch.log_softmax(logits.float(), dim=-1).view(B, K, V)
            val, idx = (lp + scores[:, :, None]).view(B, K * V).topk(K)
            parent = idx // V
            return val, idx % V, parent, (base + parent).view(-1)

        t_k, t_c = time_pair_us(
            lambda: ops.beam_topk(logits, scores, fin, lens, 1, ws), composite)
        print(f"beam_topk B*K={BK} V={V} K={K}: kernel {t_k:.2f} us | "
              f"ATen composite {t_c:.2f} us | kernel/composite "
              f"{t_k / t_c:.3f}", flush=True)
    NL, H, dh, Lmax = 6, 8, 64, 272
    for BK in (4, 16, 32, 64):
        src = [torch.randn(BK, Lmax, 2, H, dh, device="cuda").bfloat16()
               for _ in range(NL)]
        dst = [torch.empty_like(t) for t in src]
        table = ops.beam_gather_table(src, dst)
        idx = torch.randint(0, BK, (BK,), device="cuda")
        src_row = idx.int()
        for kvl in (16, 64, 256):
            kv_len = torch.full((BK,), kvl, dtype=torch.int32, device="cuda")
            n = kvl + 1

            def composite():
                for s, d in zip(src, dst):
                    d[:, :n].copy_(s[:, :n].index_select(0, idx))

            t_k, t_c = time_pair_us(
                lambda: ops.beam_gather_kv(src, dst, src_row, kv_len, table),
                composite)
            mb = NL * BK * n * 2 * H * dh * 2 / 1e6
            print(f"beam_gather_kv B*K={BK} kv_len={kvl} ({mb:.1f} MB moved): "
                  f"kernel {t_k:.2f} us | index_select+copy_ x{NL} "
                  f"{t_c:.2f} us | kernel/composite {t_k / t_c:.3f}",
                  flush=True)


def _self_case(BK, K, kvl, H=8, dh=64):
    Lmax = kvl + 16
    qkv = torch.randn(BK, 1, 3, H, dh, device="cuda").bfloat16()
    cache = torch.randn(BK, Lmax, 2, H, dh, device="cuda").bfloat16()
    kv_len = torch.full((BK,), kvl, dtype=torch.int32, device="cuda")
    origin = torch.randint(0, K, (BK, Lmax), device="cuda", dtype=torch.uint8)
    return qkv, cache, kv_len, origin, Lmax


def bench_indirect():
    """The beam kernels that leave the cache where it is, each against what
    it replaces at the same shape (6 layers, H 8, dh 64, K 4)."""
    E, NL, H, dh, K = ops.ext(), 6, 8, 64, 4
    scale = dh ** -0.5
    for BK in (4, 16, 32, 64):
        src = [torch.randn(BK, 272, 2, H, dh, device="cuda").bfloat16()
               for _ in range(NL)]
        dst = [torch.empty_like(t) for t in src]
        table = ops.beam_gather_table(src, dst)
        src_row = torch.randint(0, BK, (BK,), device="cuda").int()
        tin = torch.randint(0, K, (BK, 272), device="cuda", dtype=torch.uint8)
        tout = torch.zeros_like(tin)
        for kvl in (16, 64, 256):
            kv_len = torch.full((BK,), kvl, dtype=torch.int32, device="cuda")
            t_r, t_g = time_pair_us(
                lambda: ops.beam_reindex(tin, tout, src_row, kv_len, K, 272),
                lambda: ops.beam_gather_kv(src, dst, src_row, kv_len, table))
            print(f"reorder B*K={BK} kv_len={kvl}: beam_reindex {t_r:.2f} us "
                  f"({BK * (kvl + 1)} B) | beam_gather_kv {t_g:.2f} us "
                  f"({NL * BK * (kvl + 1) * 2 * H * dh * 2 / 1e6:.1f} MB) | "
                  f"saved per step {t_g - t_r:.2f} us", flush=True)
    for BK in (4, 16, 32, 64):
        for kvl in (64, 256, 2048):
            qkv, cache, kv_len, origin, Lmax = _self_case(BK, K, kvl)
            ws = ops.decode_attention_beam_workspace(BK // K, K, H, dh, Lmax)
            t_b, t_p = time_pair_us(
                lambda: E.decode_attn_self_beam(qkv, cache, kv_len, origin, K,
                                                ws, scale),
                lambda: E.decode_attn_self(qkv, cache, kv_len, ws, scale))
            print(f"self B*K={BK} keys={kvl} "
                  f"nsplit={E.decode_attn_nsplit(BK * H, Lmax)}: "
                  f"decode_attn_self_beam {t_b:.2f} us | decode_attn_self "
                  f"{t_p:.2f} us | indirection costs {t_b - t_p:+.2f} us per "
                  f"call, {NL * (t_b - t_p):+.2f} us per step", flush=True)
    for BK in (4, 16, 32, 64):
        for Sk in (64, 256):
            B = BK // K
            q = torch.randn(BK, 1, H, dh, device="cuda").bfloat16()
            kv = torch.randn(B, Sk, 2, H, dh, device="cuda").bfloat16()
            kv_rep = kv.repeat_interleave(K, dim=0)
            pad = torch.zeros(B, Sk, dtype=torch.uint8, device="cuda")
            pad_rep = pad.repeat_interleave(K, dim=0)
            ws = ops.decode_attention_beam_workspace(B, K, H, dh, Sk)
            ws1 = ops.decode_attention_workspace(BK, H, dh, Sk)
            t_b, t_p = time_pair_us(
                lambda: E.decode_attn_cross_beam(q, kv, pad, K, ws, scale),
                lambda: E.decode_attn_cross(q, kv_rep, pad_rep, ws1, scale))
            print(f"cross B*K={BK} Sk={Sk}: decode_attn_cross_beam {t_b:.2f} "
                  f"us ({kv.numel() * 2 / 1e3:.0f} KB of K/V) | "
                  f"decode_attn_cross on {BK} replicated rows {t_p:.2f} us "
                  f"({kv_rep.numel() * 2 / 1e3:.0f} KB) | beam/replicated "
                  f"{t_b / t_p:.3f}", flush=True)
    Sk = 256
    for B in (1, 16):                      # B*H = 8 and 128
        q = torch.randn(B * K, 1, H, dh, device="cuda").bfloat16()
        kv = torch.randn(B, Sk, 2, H, dh, device="cuda").bfloat16()
        pad = torch.zeros(B, Sk, dtype=torch.uint8, device="cuda")
        # tickets + partials for up to 4 forced splits
        ws = torch.zeros(B * H * K * (1 + 4 * (dh + 4)), device="cuda")
        cols = []
        for ns in (1, 2, 3, 4):
            t, _ = time_pair_us(
                lambda: E.decode_attn_cross_beam(q, kv, pad, K, ws, scale, ns),
                lambda: E.decode_attn_cross_beam(q, kv, pad, K, ws, scale, ns))
            cols.append(f"nsplit {ns}: {t:.2f} us")
        print(f"cross_beam nsplit sweep B*H={B * H} Sk={Sk} (rule: "
              f"{E.decode_attn_nsplit(B * H, Sk)}): " + " | ".join(cols),
              flush=True)


def flagship():
    from transformer_amd.models import Transformer
    torch.manual_seed(0)
    return Transformer(num_layers=6, d_model=512, num_heads=8, dff=2048,
                       input_vocab_size=32002, target_vocab_size=32002,
                       rate=0.0, max_position=512).to("cuda",
                                                      torch.bfloat16).eval()


def bench_e2e(max_len=64):
    """end_id -1 never matches, so every decode runs max_len steps."""
    from transformer_amd.models.transformer import (beam_search_decode,
                                                    greedy_decode)
    model = flagship()
    for B, S, max_len in ((1, 32, max_len), (8, 32, max_len), (16, 256, 256)):
        inp = torch.randint(2, 32000, (B, S), device="cuda")
        for skinny in (False, True):
            runs = {
                "beam4": lambda: beam_search_decode(
                    model, inp, 32000, -1, beam_size=4, max_len=max_len,
                    skinny_linear=skinny),
                "indirect": lambda: beam_search_decode(
                    model, inp, 32000, -1, beam_size=4, max_len=max_len,
                    skinny_linear=skinny, indirect_kv=True),
                "greedy": lambda: greedy_decode(
                    model, inp, 32000, -1, max_len=max_len, fused_attn=True,
                    skinny_linear=skinny)}
            ms = {}
            for name, fn in runs.items():
                fn()
                best = float("inf")
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    best = min(best, time.perf_counter() - t0)
                ms[name] = best * 1e3 / max_len
            print(f"e2e B={B} src={S} tokens={max_len} "
                  f"skinny_linear={skinny}: beam_search_decode K=4 "
                  f"({4 * B} rows) {ms['beam4']:.3f} ms/token | indirect_kv "
                  f"{ms['indirect']:.3f} ms/token | greedy_decode "
                  f"fused_attn ({B} rows) {ms['greedy']:.3f} ms/token | "
                  f"indirect/beam {ms['indirect'] / ms['beam4']:.3f} | "
                  f"beam/greedy {ms['beam4'] / ms['greedy']:.2f}", flush=True)


def one_beam(max_len=16):
    from transformer_amd.models.transformer import beam_search_decode
    model = flagship()
    inp = torch.randint(2, 32000, (1, 32), device="cuda")
    beam_search_decode(model, inp, 32000, -1, beam_size=4, max_len=max_len)
    torch.cuda.synchronize()
    print(f"one beam decode done: K=4, {max_len} steps")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--e2e", action="store_true")
    p.add_argument("--one_beam", action="store_true")
    p.add_argument("--indirect", action="store_true")
    args = p.parse_args()
    if args.e2e:
        bench_e2e()
    elif args.indirect:
        bench_indirect()
    elif args.one_beam:
        one_beam()
    else:
        bench_kernels()
    print("beam bench done")
