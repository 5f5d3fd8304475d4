"""Microbenchmark the GEMM paths at the model's actual shapes (GPU box).

    python tools/gemm_bench.py [iters]

For each backward shape it times BOTH implementations:
  dX:  gemm_nn(dy, w)            vs  transpose2d(w) + gemm_nt(dy, wT)
  dW:  gemm_tn(dy, x)            vs  transpose2d(dy)+transpose2d(x)+gemm_nt
so the functional layer's dispatch choices are measurement-driven.

gemm256 epilogue arms (TFMX_G256_EPI, read per call), device events, arms
interleaved round-robin in one process, one JSON line per result:

    python tools/gemm_bench.py --ksweep [rounds] [iters]
        gemm256_nt at the QKV / attn-O / FFN1 / logits forward (M, N) for
        K = 128..2048 per arm, and the line fit  us = fixed + slope * K/64
        (fixed = per-call prologue + epilogue, slope = one K-tile).
    python tools/gemm_bench.py --epi [rounds] [iters]
        scalar vs vec8 vs lds at the seven forward and five dX shapes
        (dX as the trainer runs it: NT against the transposed weight).
    python tools/gemm_bench.py --ffn [rounds] [iters]
        FFN2 dX + relu_bwd and FFN1 dX + add at M=16384: GEMM + separate
        pass vs the fused relu-mask / residual-add epilogue, per arm.
"""

import json
import os
import statistics
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


# forward shapes: (M, N, K, tag) — transformer-base B=64 S=256 + big-model
FWD = [
    (16384, 1536, 512, "QKV fwd"),
    (16384, 512, 512, "attn O fwd"),
    (16384, 2048, 512, "FFN1 fwd"),
    (16384, 512, 2048, "FFN2 fwd"),
    (16320, 32770, 512, "logits fwd"),
    (16384, 3072, 1024, "big QKV fwd"),
    (16384, 4096, 1024, "big FFN1 fwd"),
]

# dX shapes: dy (M, N_out) @ w (N_out, K_in): (M, N_out, K_in, tag)
DX = [
    (16384, 1536, 512, "QKV dx"),
    (16384, 512, 512, "attn O dx"),
    (16384, 512, 2048, "FFN1 dx"),
    (16384, 2048, 512, "FFN2 dx"),
    (16320, 32770, 512, "logits dx"),
]

# dW shapes: dy (Mtok, N_out), x (Mtok, K_in): (Mtok, N_out, K_in, tag)
DW = [
    (16384, 1536, 512, "QKV dW"),
    (16384, 512, 512, "attn O dW"),
    (16384, 2048, 512, "FFN1 dW"),
    (16384, 512, 2048, "FFN2 dW"),
    (16320, 32770, 512, "logits dW"),
]


EPI_ARMS = ("scalar", "vec8", "lds")


def _with_arm(arm, fn):
    def run():
        os.environ["TFMX_G256_EPI"] = arm
        fn()
    return run


def time_arms(arms, rounds, iters, warmup=3):
    """{name: us/call stats}; arms take turns inside every round."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / iters)
    os.environ.pop("TFMX_G256_EPI", None)
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in times.items()}


def _rb(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def ksweep(rounds, iters):
    import numpy as np
    E = ext()
    ks = (128, 256, 512, 1024, 2048)
    for (m, n, _, tag) in (FWD[0], FWD[1], FWD[2], FWD[4]):
        bias = _rb(n)
        out = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
        ops = {k: (_rb(m, k), _rb(n, k)) for k in ks}
        arms = {}
        for k in ks:
            a, w = ops[k]
            for arm in EPI_ARMS:
                arms[f"{arm}:{k}"] = _with_arm(
                    arm, lambda a=a, w=w: E.gemm256_nt(a, w, bias, 0, out))
        res = time_arms(arms, rounds, iters)
        for arm in EPI_ARMS:
            us = [res[f"{arm}:{k}"]["median_us"] for k in ks]
            slope, fixed = np.polyfit([k / 64 for k in ks], us, 1)
            print(json.dumps({
                "bench": "ksweep", "shape": tag, "M": m, "N": n, "arm": arm,
                "us_by_K": dict(zip(ks, us)),
                "fixed_us": round(float(fixed), 2),
                "us_per_ktile": round(float(slope), 3),
                "fixed_share_at_K512": round(
                    float(fixed) / res[f"{arm}:512"]["median_us"], 3),
            }), flush=True)


def epi_arms(rounds, iters):
    E = ext()
    cases = [(m, n, k, tag, True) for (m, n, k, tag) in FWD]
    for (m, n_out, k_in, tag) in DX:
        # the head's dY arrives zero-padded to a multiple of 256 columns
        kc = (n_out + 255) // 256 * 256 if n_out % 64 else n_out
        cases.append((m, k_in, kc, tag, False))
    for (m, n, k, tag, has_bias) in cases:
        a, w = _rb(m, k), _rb(n, k)
        bias = _rb(n) if has_bias else torch.Tensor()
        out = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
        on256 = bool(E.gemm256_viable(m, n, k))
        arms = {arm: _with_arm(arm, lambda: E.gemm_nt(a, w, bias, 0))
                for arm in EPI_ARMS}
        res = time_arms(arms, rounds, iters)
        print(json.dumps({"bench": "epi", "shape": tag, "M": m, "N": n,
                          "K": k, "gemm256": on256, "times": res}),
              flush=True)
        del a, w, out


def ffn_fused(rounds, iters):
    E = ext()
    m, d, dff = 16384, 512, 2048
    nob = torch.Tensor()
    dxm, w2t, h = _rb(m, d), _rb(dff, d), torch.relu(_rb(m, dff))
    dz, w1t, dres = _rb(m, dff), _rb(d, dff), _rb(m, d)
    arms = {}
    for arm in EPI_ARMS:
        arms[f"ffn2_split:{arm}"] = _with_arm(
            arm, lambda: E.relu_bwd(E.gemm_nt(dxm, w2t, nob, 0), h))
        arms[f"ffn2_fused:{arm}"] = _with_arm(
            arm, lambda: E.gemm256_nt(dxm, w2t, nob, 2, None, h))
        arms[f"ffn1_split:{arm}"] = _with_arm(
            arm, lambda: E.gemm_nt(dz, w1t, nob, 0) + dres)
        arms[f"ffn1_fused:{arm}"] = _with_arm(
            arm, lambda: E.gemm256_nt(dz, w1t, nob, 3, None, dres))
    res = time_arms(arms, rounds, iters)
    print(json.dumps({"bench": "ffn", "M": m, "times": res}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("--ksweep", "--epi", "--ffn"):
        rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
        iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
        torch.manual_seed(0)
        {"--ksweep": ksweep, "--epi": epi_arms,
         "--ffn": ffn_fused}[sys.argv[1]](rounds, iters)
        return
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    E = ext()
    torch.manual_seed(0)

    print("== 256-template vs 128-kernel vs torch.matmul (hipBLASLt) ==")
    for (m, n, k, tag) in FWD + [(16384, 512, 2048, "FFN2 fwd"),
                                 (1536, 512, 16384, "QKV dW"),
                                 (32770, 512, 16320, "logits dW"),
                                 (4096, 4096, 4096, "4096^3 cal"),
                                 (8192, 8192, 8192, "8192^3 cal")]:
        a = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
        nob = torch.Tensor()
        ref = (a[:512].float() @ w.t().float()[:, :512])
        got = E.gemm256_nt(a, w, nob, 0)[:512, :512].float()
        err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1)
        t256 = timeit(lambda: E.gemm256_nt(a, w, nob, 0), iters)
        t128 = timeit(lambda: E.gemm128_nt(a, w, nob, 0), iters)
        tbl = timeit(lambda: torch.matmul(a, w.t()), iters)
        fl = 2.0 * m * n * k
        print(f"{tag:14s} 256 {t256*1e3:8.3f} ms ({fl/t256/1e12:6.1f} TF) | "
              f"128 {t128*1e3:8.3f} ({fl/t128/1e12:6.1f}) | "
              f"blaslt {tbl*1e3:8.3f} ({fl/tbl/1e12:6.1f})  relerr {err:.2e}")

    print("== forward: gemm_nt ==")
    for (m, n, k, tag) in FWD:
        a = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
        b = torch.randn(n, device="cuda", dtype=torch.bfloat16)
        dt = timeit(lambda: E.gemm_nt(a, w, b, 0), iters)
        fl = 2.0 * m * n * k
        print(f"{tag:14s} M{m:6d} N{n:6d} K{k:6d} {dt*1e3:8.3f} ms {fl/dt/1e12:7.1f} TF/s")

    print("== dX: gemm_nn vs transpose(w)+gemm_nt ==")
    for (m, n, k, tag) in DX:
        dy = torch.randn(m, n, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
        t_nn = timeit(lambda: E.gemm_nn(dy, w), iters)
        t_tr = timeit(lambda: E.gemm_nt(dy, E.transpose2d(w), torch.Tensor(), 0), iters)
        t_bl = timeit(lambda: torch.matmul(dy, w), iters)
        fl = 2.0 * m * n * k
        print(f"{tag:14s} nn {t_nn*1e3:8.3f} ms ({fl/t_nn/1e12:6.1f} TF) | "
              f"tr+nt {t_tr*1e3:8.3f} ms ({fl/t_tr/1e12:6.1f} TF) | "
              f"blaslt {t_bl*1e3:8.3f} ({fl/t_bl/1e12:6.1f})")

    print("== dW: gemm_tn vs transpose(dy)+transpose(x)+gemm_nt ==")
    for (mt, n, k, tag) in DW:
        dy = torch.randn(mt, n, device="cuda", dtype=torch.bfloat16)
        x = torch.randn(mt, k, device="cuda", dtype=torch.bfloat16)
        t_tn = timeit(lambda: E.gemm_tn(dy, x), iters)
        t_tr = timeit(lambda: E.gemm_nt(E.transpose2d(dy), E.transpose2d(x),
                                        torch.Tensor(), 0), iters)
        t_bl = timeit(lambda: torch.matmul(dy.t(), x), iters)
        t_dw = timeit(lambda: E.gemm_dw(dy, x), iters)
        fl = 2.0 * mt * n * k
        print(f"{tag:14s} tn {t_tn*1e3:8.3f} ms ({fl/t_tn/1e12:6.1f} TF) | "
              f"tr+nt {t_tr*1e3:8.3f} ms ({fl/t_tr/1e12:6.1f} TF) | "
              f"blaslt {t_bl*1e3:8.3f} ({fl/t_bl/1e12:6.1f}) | "
              f"dw {t_dw*1e3:8.3f} ({fl/t_dw/1e12:6.1f})")


if __name__ == "__main__":
    main()
