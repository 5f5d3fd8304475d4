"""Skinny-M decode linear (linear_rows.hip) against the training GEMM.

Times linear_rows at 4 and at 8 waves per block and under the host rule
(nw 0), next to gemm_nt at the same shape (its zero-fill + kernel + finalize
together where it takes the split-K path), as device events around a
replayed graph of ITERS calls, best of 3.  For the 32k-vocabulary head the
achieved bytes/s, (N*K + M*K + M*N)*2 over the time, are printed as a share
of the HBM peak: that shape is bandwidth-bound, the others latency-bound.
For the N = 512 shapes, which feed a LayerNorm in the decoder, the fused
linear_rows_ln is timed against linear_rows + ln_fwd and gemm_nt + ln_fwd.
Last, linear_rows_preln (the LayerNorm in the consuming linear's prologue)
against ln_fwd + linear_rows at K = 512: the two graphs replayed in turn,
best of 3 each with the min..max spread, and whether the fused launch wins
by more than the larger spread (the dispatch rule's test).

    python tools/linear_rows_bench.py [--only_preln]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_amd.ops import ext

ap = argparse.ArgumentParser()
ap.add_argument("--only_preln", action="store_true")
args = ap.parse_args()

E = ext()
ITERS = 200
HBM_PEAK = 8.0e12     # MI355X HBM3E, bytes/s


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
    """(min, max) us per call of 3 replays of each graph of ITERS calls,
    the two replayed in turn."""
    graphs = (graph_of(fa), graph_of(fb))
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    ts = ([], [])
    for _ in range(3):
        for g, t in zip(graphs, ts):
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b) * 1e3 / ITERS)
    return tuple((min(t), max(t)) for t in ts)


def time_us(fn):
    """Best of 3 replays of a graph of ITERS calls (no host launch cost)."""
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


for N, K in (() if args.only_preln else
             ((1536, 512), (512, 512), (2048, 512), (512, 2048),
              (32002, 512))):
    w = torch.randn(N, K, device="cuda").bfloat16()
    bias = torch.randn(N, device="cuda").bfloat16()
    for M in (1, 8, 16, 64):
        x = torch.randn(M, K, device="cuda").bfloat16()
        t = {nw: time_us(lambda: E.linear_rows(x, w, bias, False, nw))
             for nw in (4, 8, 0)}
        t_gemm = time_us(lambda: E.gemm_nt(x, w, bias, 0))
        line = (f"M={M} N={N} K={K}: linear_rows nw4 {t[4]:.2f} us nw8 "
                f"{t[8]:.2f} us rule {t[0]:.2f} us | gemm_nt {t_gemm:.2f} us "
                f"| rule/gemm_nt {t[0] / t_gemm:.3f}")
        if N > 4096:
            bps = (N * K + M * K + M * N) * 2 / (t[0] * 1e-6)
            line += (f" | {bps / 1e12:.2f} TB/s = {100 * bps / HBM_PEAK:.0f}%"
                     " of HBM peak (bandwidth-bound)")
        print(line, flush=True)
        if N == 512:     # the shapes that feed a LayerNorm (w_o, ffn.w2)
            res = torch.randn(M, N, device="cuda").bfloat16()
            ws = E.linear_rows_workspace(M, N)
            t_ln = time_us(lambda: E.linear_rows_ln(x, w, bias, res, bias,
                                                    bias, 1e-6, ws))
            t_sep = time_us(lambda: E.ln_fwd(E.linear_rows(x, w, bias), res,
                                             bias, bias, 1e-6))
            t_two = time_us(lambda: E.ln_fwd(E.gemm_nt(x, w, bias, 0), res,
                                             bias, bias, 1e-6))
            print(f"M={M} N={N} K={K}: linear_rows_ln {t_ln:.2f} us | "
                  f"linear_rows + ln_fwd {t_sep:.2f} us | "
                  f"gemm_nt + ln_fwd {t_two:.2f} us", flush=True)
K = 512
gamma, beta = (torch.randn(K, device="cuda").bfloat16() for _ in range(2))
for N in (512, 1536, 2048, 32002):
    w = torch.randn(N, K, device="cuda").bfloat16()
    bias = torch.randn(N, device="cuda").bfloat16()
    for M in (1, 8, 16, 64):
        p, r = (torch.randn(M, K, device="cuda").bfloat16() for _ in range(2))
        (f0, f1), (t0, t1) = time_pair_us(
            lambda: E.linear_rows_preln(p, r, gamma, beta, 1e-6, w, bias),
            lambda: E.linear_rows(E.ln_fwd(p, r, gamma, beta, 1e-6)[0], w,
                                  bias))
        spread = max(f1 - f0, t1 - t0)
        print(f"M={M} N={N} K={K}: linear_rows_preln {f0:.2f} us "
              f"[{f0:.2f}..{f1:.2f}] | ln_fwd + linear_rows {t0:.2f} us "
              f"[{t0:.2f}..{t1:.2f}] | fused/two {f0 / t0:.3f} | "
              f"{'WINS' if t0 - f0 > spread else 'no win'} "
              f"(margin {t0 - f0:.2f} us, spread {spread:.2f} us)", flush=True)
print("linear_rows bench done")
