"""Bias-gradient column sums: the row-streaming kernel against the column
kernel it replaces, with `adam_fused` as the bandwidth yardstick of the run.

    python tools/colsum_bench.py [--rounds 5] [--iters 20]
                                 [--out profiles/colsum_rows_bench.jsonl]

Per shape the arms are `cols` (colsum_kernel, selected per call with
TFMX_COLSUM=cols: the previous kernel in the same process), `rows`
(colsum_rows_kernel, `rows`) and `adam_fused` on the transformer-base flat buffer
(28 B/param).  Shapes are the trainer's bias-gradient calls at B=64, S=256:
(16384, 512 / 1024 / 1536 / 2048), the dlogits view (16320, 32770) with row
stride 33024, and (256, 512) for the fixed cost; then four narrow / short
shapes around the default's dispatch rule.  The FFN1 pair at
(16384, 2048) is timed three ways: relu_bwd + colsum(cols), relu_bwd +
colsum(rows), relu_bwd_db.

Arms are interleaved round-robin in ONE process; each round times `iters`
back-to-back calls between two device events; median and min-max over the
rounds are reported.  One JSON line per shape, printed and appended to
--out.  Needs a GPU; there is no CPU fallback.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_bench import MODELS, flat_numel  # noqa: E402
from transformer_amd.ops import ext  # noqa: E402

SHAPES = [  # (M, N, lda)
    (16384, 512, 512), (16384, 1024, 1024), (16384, 1536, 1536),
    (16384, 2048, 2048), (16320, 32770, 33024), (256, 512, 512),
    # narrow and short: where the default keeps the column kernel
    (2048, 64, 64), (2048, 192, 192), (2048, 512, 512), (16384, 192, 192),
]


def time_arms(arms, rounds, iters, warmup):
    """arms: {name: (TFMX_COLSUM value or None, fn)}.  The variable is read
    per call by the extension, so it is set once around each timed window,
    not inside it: the window holds nothing but the `iters` launches."""
    def window(arm, fn, n):
        if arm is None:
            os.environ.pop("TFMX_COLSUM", None)
        else:
            os.environ["TFMX_COLSUM"] = arm
        try:
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
        finally:
            os.environ.pop("TFMX_COLSUM", None)
        return a.elapsed_time(b) * 1e3 / n  # us/call
    for arm, fn in arms.values():
        window(arm, fn, warmup)
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for name, (arm, fn) in arms.items():
            times[name].append(window(arm, fn, iters))
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2),
                "max_us": round(max(v), 2)} for k, v in times.items()}


def adam_arm(e, n):
    g = torch.Generator(device="cuda").manual_seed(0)
    master = torch.randn(n, device="cuda", generator=g) * 0.02
    m, v = torch.zeros_like(master), torch.zeros_like(master)
    grad = torch.randn(n, device="cuda", generator=g).bfloat16()
    w = master.bfloat16()
    return lambda: e.adam_fused(master, m, v, grad, w, 1e-4, 0.9, 0.98,
                                1e-9, 10)


def gbps(nbytes, t):
    return {k: round(nbytes / t[k] / 1e3, 1)
            for k in ("median_us", "min_us", "max_us")}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--vocab", type=int, default=32768)
    p.add_argument("--out", type=str,
                   default="profiles/colsum_rows_bench.jsonl")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colsum_bench needs a GPU")
    e = ext()
    n_flat = flat_numel(MODELS["base"], args.vocab + 2)
    adam = adam_arm(e, n_flat)
    lines = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for M, N, lda in SHAPES:
        buf = torch.zeros(M, lda, device="cuda", dtype=torch.bfloat16)
        buf[:, :N] = torch.randn(M, N, device="cuda", generator=g).bfloat16()
        a = buf[:, :N]
        out = torch.empty(N, device="cuda", dtype=torch.bfloat16)
        arms = {"cols": ("cols", lambda: e.colsum(a, out)),
                "rows": ("rows", lambda: e.colsum(a, out)),
                "adam_fused": (None, adam)}
        t = time_arms(arms, args.rounds, args.iters, args.warmup)
        nbytes = 2 * M * N
        lines.append({
            "op": "colsum", "M": M, "N": N, "lda": lda, "bytes": nbytes,
            "rounds": args.rounds, "iters_per_round": args.iters, "times": t,
            "cols_GBps": gbps(nbytes, t["cols"]),
            "rows_GBps": gbps(nbytes, t["rows"]),
            "adam_fused_GBps": gbps(28 * n_flat, t["adam_fused"]),
            "rows_over_cols_median": round(
                t["rows"]["median_us"] / t["cols"]["median_us"], 4),
        })
        print(json.dumps(lines[-1]), flush=True)
        del buf, a

    M, N = 16384, 2048
    dy = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    y = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    db = torch.empty(N, device="cuda", dtype=torch.bfloat16)
    arms = {
        "relu_bwd+cols": ("cols", lambda: e.colsum(e.relu_bwd(dy, y), db)),
        "relu_bwd+rows": ("rows", lambda: e.colsum(e.relu_bwd(dy, y), db)),
        "relu_bwd_db": (None, lambda: e.relu_bwd_db(dy, y, db)),
        "relu_bwd": (None, lambda: e.relu_bwd(dy, y)),
        "adam_fused": (None, adam),
    }
    t = time_arms(arms, args.rounds, args.iters, args.warmup)
    nbytes = 6 * M * N   # read dy and y, write dz
    lines.append({
        "op": "ffn1_pair", "M": M, "N": N, "bytes_needed": nbytes,
        "rounds": args.rounds, "iters_per_round": args.iters, "times": t,
        "relu_bwd_db_GBps": gbps(nbytes, t["relu_bwd_db"]),
        "adam_fused_GBps": gbps(28 * n_flat, t["adam_fused"]),
        "db_over_pair_cols_median": round(
            t["relu_bwd_db"]["median_us"] / t["relu_bwd+cols"]["median_us"],
            4),
        "db_over_pair_rows_median": round(
            t["relu_bwd_db"]["median_us"] / t["relu_bwd+rows"]["median_us"],
            4),
    })
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
