"""A/B the fused attention kernels at model shapes (GPU box).

Forward: trv=1 (tr16 reads of natural V) vs trv=0 (transposed V image).
Backward: timed as-is.  python tools/attn_bench.py [iters]

--segments [L]: sequence packing.  Lays a corpus-like sentence-length mix
out as segment ids in rows of width L (default 256) and times forward and
backward of the segment kernels, which skip the tiles outside each block's
id range, against the same tokens as dense rows of width L (every tile
computed).  python tools/attn_bench.py --segments [L] [iters]
"""
import sys
import time

import torch

sys.path.insert(0, ".")
from transformer_amd.ops import ext  # noqa: E402


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


# (B, H, Sq, Sk, dh, causal, tag)
SHAPES = [
    (64, 8, 256, 256, 64, False, "base enc self"),
    (64, 8, 255, 255, 64, True, "base dec self"),
    (64, 8, 255, 256, 64, False, "base cross"),
    (64, 16, 256, 256, 64, False, "big enc self"),
    (8, 16, 4096, 4096, 64, False, "big4k enc"),
    (8, 16, 4095, 4095, 64, True, "big4k dec"),
]


def segments(L, iters, B=64, H=8, dh=64):
    """Corpus-like mix: lengths ~ 4 + geometric, mean about 17 tokens, capped
    at L, first-fit in arrival order until a row is full."""
    import random
    rng = random.Random(0)
    E = ext()
    seg = torch.zeros(B, L, dtype=torch.int32)
    nseg = 0
    for b in range(B):
        o, k = 0, 1
        while True:
            n = min(L, 4 + int(rng.expovariate(1 / 13.0)))
            if o + n > L:
                break
            seg[b, o:o + n] = k
            o, k = o + n, k + 1
        nseg += k - 1
    seg = seg.cuda()
    fill = float((seg != 0).float().mean())
    lens2 = sum(int((seg[b] == k).sum()) ** 2 for b in range(B)
                for k in range(1, int(seg[b].max()) + 1))
    print(f"L={L} B={B} H={H} dh={dh}: {nseg} segments, fill {fill:.3f}, "
          f"sum len^2 / B*L^2 = {lens2 / (B * L * L):.3f}")
    torch.manual_seed(0)
    nop = torch.Tensor()
    sc = dh ** -0.5
    q, k, v = (torch.randn(B, L, H, dh, device="cuda", dtype=torch.bfloat16)
               for _ in range(3))
    for causal in (False, True):
        o, lse = E.attn_fwd_seg(q, k, v, seg, seg, causal, sc)
        do = torch.randn_like(o)
        tf = timeit(lambda: E.attn_fwd_seg(q, k, v, seg, seg, causal, sc),
                    iters)
        tb = timeit(lambda: E.attn_bwd_seg(q, k, v, o, do, lse, seg, seg,
                                           causal, sc, 0), iters)
        o2, lse2 = E.attn_fwd(q, k, v, nop, causal, sc, 1)
        df = timeit(lambda: E.attn_fwd(q, k, v, nop, causal, sc, 1), iters)
        db = timeit(lambda: E.attn_bwd(q, k, v, o2, do, lse2, nop, causal,
                                       sc, 0), iters)
        print(f"causal={int(causal)}  fwd seg {tf*1e3:7.3f} ms vs dense "
              f"{df*1e3:7.3f} ({df/tf:4.2f}x) | bwd seg {tb*1e3:7.3f} vs "
              f"dense {db*1e3:7.3f} ({db/tb:4.2f}x)")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--segments":
        rest = [int(a) for a in sys.argv[2:]]
        segments(rest[0] if rest else 256, rest[1] if len(rest) > 1 else 30)
        return
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    E = ext()
    torch.manual_seed(0)
    nop = torch.Tensor()
    for (B, H, Sq, Sk, dh, causal, tag) in SHAPES:
        q = torch.randn(B, Sq, H, dh, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, Sk, H, dh, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(B, Sk, H, dh, device="cuda", dtype=torch.bfloat16)
        sc = dh ** -0.5
        t1 = timeit(lambda: E.attn_fwd(q, k, v, nop, causal, sc, 1), iters)
        t0 = timeit(lambda: E.attn_fwd(q, k, v, nop, causal, sc, 0), iters)
        o, lse = E.attn_fwd(q, k, v, nop, causal, sc, 1)
        do = torch.randn_like(o)
        tb = timeit(lambda: E.attn_bwd(q, k, v, o, do, lse, nop, causal,
                                       sc, 0), iters)
        fl = 4.0 * B * H * Sq * Sk * dh * (0.5 if causal else 1.0)
        print(f"{tag:14s} fwd trv {t1*1e3:7.3f} ms ({fl/t1/1e12:6.1f} TF) | "
              f"fwd img {t0*1e3:7.3f} ({fl/t0/1e12:6.1f}) | "
              f"bwd {tb*1e3:7.3f} ({2.5*fl/tb/1e12:6.1f})")


if __name__ == "__main__":
    main()
