"""NSPLIT sweep of the decode-attention kernel (decode_attn.hip).

Times decode_attn_self alone (device events around a replayed graph of
ITERS launches, cache nearly full: kv_len = L-1) for each forced split count and
for the host rule (nsplit 0), next to the training kernel at the same shape
(attn_fwd over the L cached keys, what decode used before).  dh = 64.

    python tools/decode_attn_bench.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_amd.ops import ext

E = ext()
H, DH, ITERS = 8, 64, 200
SCALE = DH ** -0.5


def time_us(fn):
    """Best of 3 replays of a graph of ITERS launches (no host launch cost)."""
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
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    best = float("inf")
    for _ in range(3):
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / ITERS)
    return best


for L in (64, 256, 2048):
    for BH in (8, 64, 512):
        B = BH // H
        qkv = torch.randn(B, 1, 3, H, DH, device="cuda").bfloat16()
        cache = torch.randn(B, L, 2, H, DH, device="cuda").bfloat16()
        kv_len = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
        rule = E.decode_attn_nsplit(BH, L)
        cands = sorted({n for n in (1, 2, 4, 8, 16, 32, 64)
                        if n <= max(1, L // 16)} | {rule})
        ws = torch.zeros(BH + 4 + BH * max(cands) * (DH + 4), device="cuda")
        res = {n: time_us(lambda: E.decode_attn_self(qkv, cache, kv_len, ws,
                                                     SCALE, n))
               for n in cands}
        q = qkv[:, :, 0].contiguous()
        k, v = cache.unbind(dim=2)
        t_old = time_us(lambda: E.attn_fwd(q, k, v, torch.Tensor(), False,
                                           SCALE))
        cols = " ".join(f"{n}:{t:.1f}" for n, t in res.items())
        print(f"L={L} BH={BH}: rule nsplit={rule} {res[rule]:.1f} us | "
              f"sweep(us) {cols} | attn_fwd {t_old:.1f} us", flush=True)
