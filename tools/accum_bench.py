"""Cost of gradient accumulation: the accumulate pass, the accumulator-reading
Adam kernel, and the whole training step at N = 1, 2, 4 micro-batches.

    python tools/accum_bench.py [--rounds 7] [--iters 50] [--steps 20]
                                [--no_steps]

Kernels, at the transformer-base flat-buffer size, timed with device events
(arms interleaved round-robin in one process, median over rounds):

    grad_accum       10 B/param  (2 read bf16 + 4 read + 4 write fp32)
    adam_fused_acc   34 B/param  (fp32 master/m/v read+write, fp32 acc
                                  read + zero write, bf16 weight write)
    adam_fused       28 B/param  the yardstick: its GB/s in the same run

Steps: Train.train_step on transformer-base, B=64 S=256, synthetic tokens,
N = 1 (today's path), 2, 4, eager and captured; median step time over
`--steps` steps after warmup and torch.cuda.max_memory_allocated.  Each arm
runs in a fresh child process so the peak-memory figures are independent.

Prints one JSON line per measurement.  Needs a GPU; no CPU fallback.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from transformer_amd.models import Transformer  # noqa: E402
from transformer_amd.ops import ext  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_bench import MODELS, flat_numel, time_arms  # noqa: E402

VOCAB = 32768 + 2


def bench_kernels(args):
    torch.manual_seed(0)
    e = ext()
    n = flat_numel(MODELS["base"], VOCAB)
    master = torch.randn(n, device="cuda") * 0.02
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    g = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    acc = torch.zeros(n, device="cuda")
    w = master.bfloat16()
    hyp = (1e-4, 0.9, 0.98, 1e-9, 10)
    arms = {
        "grad_accum": lambda: e.grad_accum(g, acc),
        "adam_fused_acc": lambda: e.adam_fused_acc(master, m, v, acc, w,
                                                   *hyp),
        "adam_fused": lambda: e.adam_fused(master, m, v, g, w, *hyp),
    }
    res = time_arms(arms, args.rounds, args.iters, args.warmup)
    gbps = lambda b, k: round(b * n / res[k]["median_us"] / 1e3, 1)
    out = {"bench": "kernels", "model": "base", "flat_numel": n,
           "rounds": args.rounds, "iters_per_round": args.iters,
           "times": res,
           "grad_accum_GBps": gbps(10, "grad_accum"),
           "adam_fused_acc_GBps": gbps(34, "adam_fused_acc"),
           "adam_fused_GBps": gbps(28, "adam_fused")}
    out["grad_accum_over_adam_fused_GBps"] = round(
        out["grad_accum_GBps"] / out["adam_fused_GBps"], 3)
    out["adam_fused_acc_over_adam_fused_GBps"] = round(
        out["adam_fused_acc_GBps"] / out["adam_fused_GBps"], 3)
    print(json.dumps(out), flush=True)


class _Tok:
    vocab_size = VOCAB - 2


def bench_step(n_micro, captured, steps, warmup):
    from transformer_amd.runtime.train_loop import Train
    torch.manual_seed(0)
    B, S = 64, 256
    model = Transformer(input_vocab_size=VOCAB, target_vocab_size=VOCAB,
                        rate=0.1, max_position=4096,
                        **MODELS["base"]).to("cuda", torch.bfloat16)
    tr = Train(1, captured, model, _Tok(), _Tok(), B, None, None, 1,
               tempfile.mkdtemp(prefix="accum_bench_"), 512,
               grad_accum_steps=n_micro)
    src = torch.randint(1, VOCAB - 2, (B, S), device="cuda")
    tar = torch.randint(1, VOCAB - 2, (B, S), device="cuda")
    for _ in range(warmup):
        tr.train_step((src, tar))
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        tr.train_step((src, tar))   # ends in the step's host read
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({
        "bench": "step", "model": "base", "B": B, "S": S,
        "grad_accum_steps": n_micro, "captured": captured, "steps": steps,
        "step_ms_median": round(statistics.median(times), 3),
        "step_ms_min": round(min(times), 3),
        "max_memory_allocated_MiB": round(
            torch.cuda.max_memory_allocated() / 2 ** 20, 1),
        "optimizer_steps": tr.optimizer.step_count}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--no_steps", action="store_true")
    p.add_argument("--_child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench needs a GPU")
    if args._child:
        bench_step(int(args._child[0]), args._child[1] == "1", args.steps,
                   args.warmup)
        return
    bench_kernels(args)
    if args.no_steps:
        return
    for captured in (False, True):
        for n_micro in (1, 2, 4):
            # a fresh process per arm: independent peak-memory figures
            subprocess.check_call(
                [sys.executable, os.path.abspath(__file__), "--steps",
                 str(args.steps), "--warmup", str(args.warmup), "--_child",
                 str(n_micro), "1" if captured else "0"], timeout=300)


if __name__ == "__main__":
    main()
