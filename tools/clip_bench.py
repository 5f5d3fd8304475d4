"""Cost of the gradient guard (global-norm clip + non-finite skip) on the
optimizer step, at the transformer-base and transformer-big flat-buffer
sizes.

    python tools/clip_bench.py [--models base big] [--rounds 7] [--iters 50]
                               [--parent_ext path/to/older/_tfmx_C*.so]

For each size it times, with device events, `NoamAdam.step()` with the guard
off and on (max_grad_norm=1, skip_nonfinite=True, random gradient so the
clip engages), plus the raw adam_fused / grad_norm_clip / adam_fused_clip
ops (the two Adam kernels on both optimizers' buffer sets).  Arms are
interleaved round-robin in ONE process, each round times
`iters` back-to-back calls between two events; median and min over rounds
are reported.  With --parent_ext the adam_fused of an older build of the
extension is timed in the same rotation on the same buffers.

Bytes moved per parameter: Adam 28 B (fp32 master/m/v read+write, bf16 grad
read, bf16 weight write); the norm pass reads the bf16 gradient once more:
2 B.  Expected on/off ratio from bytes alone: 30/28 = 1.071.

Prints one JSON line per size.  Needs a GPU; there is no CPU fallback.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from transformer_amd.models import Transformer  # noqa: E402
from transformer_amd.ops import ext  # noqa: E402
from transformer_amd.runtime import NoamAdam  # noqa: E402
from transformer_amd.runtime.optimizer import _ALIGN  # noqa: E402

MODELS = {
    "base": dict(num_layers=6, d_model=512, num_heads=8, dff=2048),
    "big": dict(num_layers=6, d_model=1024, num_heads=16, dff=4096),
}


def flat_numel(cfg, vocab):
    """Flat-buffer length FlatParams would allocate, without building the
    model on the device."""
    with torch.device("meta"):
        m = Transformer(input_vocab_size=vocab, target_vocab_size=vocab,
                        rate=0.1, max_position=4096, **cfg)
    return sum((p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
               for p in m.parameters() if p.requires_grad)


class _Flat(torch.nn.Module):
    """One bf16 parameter of the flat size: NoamAdam sees the same single
    contiguous buffer it sees for the real model."""

    def __init__(self, n):
        super().__init__()
        self.w = torch.nn.Parameter(
            torch.randn(n, device="cuda", dtype=torch.bfloat16) * 0.02)


def load_ext_from(path):
    spec = importlib.util.spec_from_file_location("_tfmx_C", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def time_arms(arms, rounds, iters, warmup):
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
            times[name].append(a.elapsed_time(b) * 1e3 / iters)  # us/call
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2),
                "max_us": round(max(v), 2)} for k, v in times.items()}


def bench_size(name, n, args, parent):
    torch.manual_seed(0)
    e = ext()
    off = NoamAdam(_Flat(n), 512, use_flat=True)
    on = NoamAdam(_Flat(n), 512, use_flat=True, max_grad_norm=1.0,
                  skip_nonfinite=True)
    assert off.flat.numel == n and not off.guarded and on.guarded
    for o in (off, on):
        o.flat.flat_g.normal_()
    ws = torch.empty(e.grad_norm_blocks(n), device="cuda")
    st = torch.zeros(4, device="cuda")
    hyp = (1e-4, 0.9, 0.98, 1e-9, 10)
    buf = lambda o: (o.master, o.m, o.v, o.flat.flat_g, o.flat.flat_w)
    arms = {
        "step_off": off.step,
        "step_on": on.step,
        "adam_fused": lambda: e.adam_fused(*buf(off), *hyp),
        "grad_norm_clip": lambda: e.grad_norm_clip(on.flat.flat_g, ws, st,
                                                   1.0, True),
        "adam_fused_clip": lambda: e.adam_fused_clip(*buf(on), *hyp, st),
        # the same two kernels with the buffer sets swapped: separates what
        # the kernel costs from where its five buffers happen to lie
        "adam_fused@on_bufs": lambda: e.adam_fused(*buf(on), *hyp),
        "adam_fused_clip@off_bufs": lambda: e.adam_fused_clip(*buf(off),
                                                              *hyp, st),
    }
    if parent is not None:
        arms["parent_adam_fused"] = lambda: parent.adam_fused(*buf(off), *hyp)
    res = time_arms(arms, args.rounds, args.iters, args.warmup)
    torch.cuda.synchronize()
    assert on.skipped_steps == 0 and on.last_grad_norm() > 1.0
    adam_bytes, norm_bytes = 28 * n, 2 * n
    out = {
        "model": name, "flat_numel": n, "rounds": args.rounds,
        "iters_per_round": args.iters, "times": res,
        "ratio_on_over_off_median": round(
            res["step_on"]["median_us"] / res["step_off"]["median_us"], 4),
        "ratio_expected_from_bytes": round(30 / 28, 4),
        "adam_fused_GBps": round(
            adam_bytes / res["adam_fused"]["median_us"] / 1e3, 1),
        "grad_norm_clip_GBps": round(
            norm_bytes / res["grad_norm_clip"]["median_us"] / 1e3, 1),
    }
    if parent is not None:
        out["ratio_off_over_parent_median"] = round(
            res["adam_fused"]["median_us"]
            / res["parent_adam_fused"]["median_us"], 4)
    print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", nargs="+", default=["base", "big"],
                   choices=list(MODELS))
    p.add_argument("--vocab", type=int, default=32768)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent_ext", type=str, default=None,
                   help="older build of the extension to time adam_fused from")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench needs a GPU")
    parent = load_ext_from(args.parent_ext) if args.parent_ext else None
    for name in args.models:
        bench_size(name, flat_numel(MODELS[name], args.vocab + 2), args,
                   parent)


if __name__ == "__main__":
    main()
