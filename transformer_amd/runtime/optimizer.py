"""Noam-scheduled Adam (C11+C12, K15) with flat-buffer fused GPU path.

MI355X design: all model parameters live as views into ONE contiguous bf16
buffer, gradients accumulate into one contiguous bf16 buffer, and the Adam
update (β1=0.9, β2=0.98, ε=1e-9 — reference train.py:65-66) runs as a single
fused multi-element HIP kernel over fp32 master weights + m/v state
(SURVEY.md §2.4 design (b): bf16 wire gradients, fp32 Adam master).  The
flat gradient buffer is also what the DP runtime all-reduces in bucket
slices (parallel/ddp.py) — fewer, larger collectives for xGMI.

CPU path: per-parameter fp32 Adam via ops/reference.py (the kernel's
numerics oracle).

Optional guard (off by default): global-norm gradient clipping and skipping
of non-finite steps.  On the GPU flat path the norm, the clip scale and the
skip decision are computed and consumed ON DEVICE (grad_clip.hip + the
clipped Adam kernels), so a hipGraph-captured step can veto itself without
a host sync.  flat_g's alignment padding is always zero, so one reduction
over the buffer is the exact global norm; it is also the buffer the DP
runtime all-reduces, so every rank takes the same decision.

Optional gradient accumulation (accum_steps > 1, off by default): every
backward kernel OVERWRITES its slice of flat_g, so "backward N times, then
step" needs a second buffer.  accumulate() adds the bf16 micro-gradient into
one fp32 accumulator of flat.numel (grad_accum.hip); step() and
step_captured() then take the norm pass and the Adam update from that
accumulator, and the Adam kernel stores zeros back into it as it goes, so
the accumulator is all-zero between optimizer steps and needs no "first
micro-step" case anywhere.  With accum_steps == 1 nothing is allocated and
exactly the bf16-gradient kernels are launched.
"""

from __future__ import annotations

import math

import torch

from ..ops import ext, has_ext, reference as R
from .schedule import NoamSchedule

_ALIGN = 64  # elements; keeps every param slice 128-byte aligned for kernels
_F32_MAX = 3.4028234663852886e38


class FlatParams:
    """Rebind every parameter of `model` as a view into one flat buffer and
    hand every backward kernel a gradient DESTINATION view into a flat
    gradient buffer (`p._flat_grad`).

    Must be called AFTER model.to(device, dtype).  The custom autograd
    Functions (ops/functional.py) write weight gradients straight into these
    views and return them, so autograd binds p.grad to the flat slice with
    ZERO per-parameter accumulate kernels per step (~200 launches saved on
    transformer-base).  Each parameter gets exactly one gradient
    contribution per backward (true for this model family); `check()`
    asserts post-backward that .grad aliases the flat buffer."""

    def __init__(self, model: torch.nn.Module):
        params = [p for p in model.parameters() if p.requires_grad]
        if not params:
            raise ValueError("model has no trainable parameters")
        dev, dt = params[0].device, params[0].dtype
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.flat_w = torch.zeros(total, device=dev, dtype=dt)
        self.flat_g = torch.zeros(total, device=dev, dtype=dt)
        self.params = params
        self.offsets = offs
        self.numel = total
        # GPU: backward kernels write into p._flat_grad views directly
        # (zero accumulate kernels).  CPU (plain torch autograd): pre-assign
        # .grad views so AccumulateGrad lands gradients in the flat buffer.
        self.direct_write = dev.type == "cuda"
        for p, off in zip(params, offs):
            n = p.numel()
            self.flat_w[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_w[off:off + n].view(p.shape)
            if self.direct_write:
                p._flat_grad = self.flat_g[off:off + n].view(p.shape)
            else:
                p.grad = self.flat_g[off:off + n].view(p.shape)

    def check(self):
        if self.direct_write:
            # GPU path: weights are hidden from autograd; kernels write into
            # p._flat_grad views directly, so there is no .grad to verify.
            for p in self.params:
                fg = getattr(p, "_flat_grad", None)
                if fg is None:
                    raise RuntimeError("parameter lost its _flat_grad view")
            return
        base = self.flat_g.data_ptr()
        end = base + self.flat_g.numel() * self.flat_g.element_size()
        for p in self.params:
            if p.grad is None or not (base <= p.grad.data_ptr() < end):
                raise RuntimeError(
                    "flat-gradient aliasing broken: autograd rebound .grad "
                    "(check torch accumulate_grad in-place semantics)")

    def zero_grad(self):
        self.flat_g.zero_()


class NoamAdam:
    """Adam with the Noam schedule computed host-side per step (K15).

    GPU: one fused HIP kernel over the whole flat parameter set.
    CPU: reference per-tensor fp32 Adam.

    max_grad_norm > 0 clips the gradient to that global L2 norm
    (scale = max_norm / (norm + 1e-6) when norm > max_norm, else exactly 1).
    skip_nonfinite=True drops a step whose fp32 sum of squared gradients is
    not finite — inf/NaN elements, and also a finite but absurd gradient
    whose sum of squares overflows fp32 (norm > ~1.8e19): master, m, v and
    the weights stay untouched, `skipped_steps` grows by one, and
    `step_count` (hence the Noam schedule) still advances.  With both off
    (the default) step()/step_captured() launch exactly the unguarded
    kernels.

    accum_steps > 1 switches the gradient source to an fp32 accumulator:
    call accumulate() after each micro backward, then step() once.  The
    guard then judges the accumulated gradient.  The accumulator(s) are
    all-zero after every step(), skipped or not."""

    def __init__(self, model: torch.nn.Module, d_model: int,
                 warmup_steps: int = 60000, betas=(0.9, 0.98), eps: float = 1e-9,
                 use_flat: bool | None = None, max_grad_norm: float = 0.0,
                 skip_nonfinite: bool = False, accum_steps: int = 1):
        if int(accum_steps) < 1:
            raise ValueError(f"accum_steps must be >= 1, got {accum_steps}")
        self.accum_steps = int(accum_steps)
        self.acc = None         # flat fp32 accumulator (accum_steps > 1)
        self.schedule = NoamSchedule(d_model, warmup_steps)
        self.betas, self.eps = betas, eps
        self.step_count = 0
        self.max_grad_norm = float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm > 0 or self.skip_nonfinite
        self._skipped = 0       # host count (CPU paths / restored value)
        self._last_norm = 0.0   # host value (CPU paths)
        self._gn_stats = None   # device {norm, scale, skipped, skipped_total}
        p0 = next(model.parameters())
        self.is_cuda = p0.is_cuda
        if use_flat is None:
            use_flat = self.is_cuda
        self.flat: FlatParams | None = None
        if use_flat:
            self.flat = FlatParams(model)
            self.master = self.flat.flat_w.float()
            self.m = torch.zeros_like(self.master)
            self.v = torch.zeros_like(self.master)
        else:
            self.params = [p for p in model.parameters() if p.requires_grad]
            self.state = [
                {"m": torch.zeros_like(p, dtype=torch.float32),
                 "v": torch.zeros_like(p, dtype=torch.float32),
                 "master": p.detach().float().clone()}
                for p in self.params
            ]
        if self.guarded and self.flat is not None and self.is_cuda:
            # allocated once, never inside a capture
            dev = self.flat.flat_g.device
            self._gn_ws = torch.empty(
                ext().grad_norm_blocks(self.flat.numel), dtype=torch.float32,
                device=dev)
            self._gn_stats = torch.zeros(4, dtype=torch.float32, device=dev)
        if self.accum_steps > 1:
            # allocated once, never inside a capture
            if self.flat is not None:
                self.acc = torch.zeros(self.flat.numel, dtype=torch.float32,
                                       device=self.flat.flat_g.device)
            else:
                for p, st in zip(self.params, self.state):
                    st["acc"] = torch.zeros_like(p, dtype=torch.float32)
                    st["acc_live"] = False

    # ---- gradient guard ---------------------------------------------------
    def last_grad_norm(self) -> float:
        """Global gradient norm (pre-clip) of the most recent guarded step.
        On the GPU this reads the device stats buffer and therefore
        SYNCHRONISES — call it at logging cadence, not per step."""
        if self._gn_stats is not None:
            return float(self._gn_stats[0].item())
        return self._last_norm

    @property
    def skipped_steps(self) -> int:
        """Steps dropped as non-finite so far.  The GPU count lives on the
        device (it is advanced inside captured graphs), so reading it
        synchronises."""
        if self._gn_stats is not None:
            return int(self._gn_stats[3].item())
        return self._skipped

    def _device_norm_pass(self):
        if self.acc is not None:
            ext().grad_norm_clip_f32(self.acc, self._gn_ws, self._gn_stats,
                                     self.max_grad_norm, self.skip_nonfinite)
            return
        ext().grad_norm_clip(self.flat.flat_g, self._gn_ws, self._gn_stats,
                             self.max_grad_norm, self.skip_nonfinite)

    # ---- gradient accumulation -------------------------------------------
    def _need_accum(self):
        if self.accum_steps <= 1:
            raise RuntimeError(
                "gradient accumulation is off: construct NoamAdam with "
                "accum_steps > 1")

    @torch.no_grad()
    def accumulate(self):
        """Add the gradient of the micro backward that just finished into
        the fp32 accumulator(s).  Graph-capturable on the GPU flat path."""
        self._need_accum()
        if self.flat is not None:
            self.flat.check()
            if self.is_cuda:
                ext().grad_accum(self.flat.flat_g, self.acc)
            else:
                self.acc.add_(self.flat.flat_g.float())
            return
        for p, st in zip(self.params, self.state):
            if p.grad is not None:
                st["acc"].add_(p.grad.float())
                st["acc_live"] = True

    @torch.no_grad()
    def discard_accum(self):
        """Zero the accumulator(s): drop the micro-gradients of an aborted
        optimizer step."""
        self._need_accum()
        if self.flat is not None:
            self.acc.zero_()
            return
        for st in self.state:
            st["acc"].zero_()
            st["acc_live"] = False

    def _host_guard(self, grads):
        """CPU semantics of the device guard: (skip, scale)."""
        norm = R.global_grad_norm_reference(grads)
        self._last_norm = norm
        # same rule as the kernel: the fp32 sum of squares must be finite
        if self.skip_nonfinite and not (math.isfinite(norm)
                                        and norm * norm <= _F32_MAX):
            self._skipped += 1
            return True, 1.0
        return False, R.clip_scale_reference(norm, self.max_grad_norm)

    @property
    def lr(self) -> float:
        return self.schedule(max(self.step_count, 1))

    # ---- HIP-graph capture support (Q12) ---------------------------------
    def graph_state(self):
        """Device-side (step, coefs) tensors for captured steps.  The step
        tensor doubles as the dropout seed epoch (ops.set_graph_rng)."""
        assert self.flat is not None and self.is_cuda
        if not hasattr(self, "_step_t"):
            dev = self.flat.flat_w.device
            self._step_t = torch.tensor([self.step_count], dtype=torch.int64,
                                        device=dev)
            self._coefs = torch.zeros(3, dtype=torch.float32, device=dev)
        return self._step_t, self._coefs

    @torch.no_grad()
    def step_captured(self):
        """Graph-capturable optimizer step: the Noam lr and Adam bias
        corrections are derived ON DEVICE from a step tensor advanced
        in-graph, so a replayed graph keeps the schedule moving.  The host
        `step_count` must be advanced by the replay wrapper.

        With the gradient guard on, the norm pass and the clipped Adam
        kernel are captured instead.  On a skipped step the device step
        tensor STILL advances, so the Noam schedule and the host
        `step_count` stay in lock-step with no sync."""
        from ..ops import ext as _ext_fn
        st, cf = self.graph_state()
        b1, b2 = self.betas
        self.flat.check()
        if self.acc is not None:
            # accumulated gradient: fp32 norm pass (if guarded), then the
            # accumulator-reading update, which re-zeroes the accumulator
            if self.guarded:
                self._device_norm_pass()
            _ext_fn().adam_fused_dev_acc(
                self.master, self.m, self.v, self.acc, self.flat.flat_w, st,
                cf, self.schedule.d_model, self.schedule.warmup_steps, b1,
                b2, self.eps, self._gn_stats)
            return
        if self.guarded:
            self._device_norm_pass()
            _ext_fn().adam_fused_dev_clip(
                self.master, self.m, self.v, self.flat.flat_g,
                self.flat.flat_w, st, cf, self.schedule.d_model,
                self.schedule.warmup_steps, b1, b2, self.eps, self._gn_stats)
            return
        _ext_fn().adam_fused_dev(self.master, self.m, self.v,
                                  self.flat.flat_g, self.flat.flat_w, st, cf,
                                  self.schedule.d_model,
                                  self.schedule.warmup_steps, b1, b2,
                                  self.eps)

    def zero_grad(self, set_to_none: bool = False):
        if self.flat is not None:
            self.flat.zero_grad()
        else:
            for p in self.params:
                if p.grad is not None:
                    p.grad.zero_()

    @torch.no_grad()
    def step(self):
        from ..ops import functional as _F
        _F.bump_weight_version()  # invalidate weight-derived caches
        self.step_count += 1
        lr = self.schedule(self.step_count)
        b1, b2 = self.betas
        if self.accum_steps > 1:
            return self._accum_step(lr, b1, b2)
        if self.guarded:
            return self._guarded_step(lr, b1, b2)
        if self.flat is not None:
            self.flat.check()
            if self.is_cuda:
                ext().adam_fused(self.master, self.m, self.v,
                                 self.flat.flat_g, self.flat.flat_w,
                                 lr, b1, b2, self.eps, self.step_count)
            else:
                g = self.flat.flat_g.float()
                R.adam_step_reference(self.master, g, self.m, self.v,
                                      self.step_count, lr, b1, b2, self.eps)
                self.flat.flat_w.copy_(self.master.to(self.flat.flat_w.dtype))
        else:
            for p, st in zip(self.params, self.state):
                if p.grad is None:
                    continue
                R.adam_step_reference(st["master"], p.grad.float(), st["m"],
                                      st["v"], self.step_count, lr, b1, b2,
                                      self.eps)
                p.data.copy_(st["master"].to(p.dtype))

    def _guarded_step(self, lr, b1, b2):
        """step() with clipping and/or non-finite skipping engaged."""
        if self.flat is not None:
            self.flat.check()
            if self.is_cuda:
                self._device_norm_pass()
                ext().adam_fused_clip(self.master, self.m, self.v,
                                      self.flat.flat_g, self.flat.flat_w,
                                      lr, b1, b2, self.eps, self.step_count,
                                      self._gn_stats)
                return
            skip, scale = self._host_guard([self.flat.flat_g])
            if skip:
                return
            g = self.flat.flat_g.float()
            if scale != 1.0:
                g = g * scale
            R.adam_step_reference(self.master, g, self.m, self.v,
                                  self.step_count, lr, b1, b2, self.eps)
            self.flat.flat_w.copy_(self.master.to(self.flat.flat_w.dtype))
            return
        live = [(p, st) for p, st in zip(self.params, self.state)
                if p.grad is not None]
        skip, scale = self._host_guard([p.grad for p, _ in live])
        if skip:
            return
        for p, st in live:
            g = p.grad.float()
            if scale != 1.0:
                g = g * scale
            R.adam_step_reference(st["master"], g, st["m"], st["v"],
                                  self.step_count, lr, b1, b2, self.eps)
            p.data.copy_(st["master"].to(p.dtype))

    def _accum_step(self, lr, b1, b2):
        """step() from the fp32 accumulator(s); leaves them all-zero."""
        if self.flat is not None:
            if self.is_cuda:
                if self.guarded:
                    self._device_norm_pass()
                ext().adam_fused_acc(self.master, self.m, self.v, self.acc,
                                     self.flat.flat_w, lr, b1, b2, self.eps,
                                     self.step_count, self._gn_stats)
                return
            skip, scale = (self._host_guard([self.acc]) if self.guarded
                           else (False, 1.0))
            if not skip:
                g = self.acc if scale == 1.0 else self.acc * scale
                R.adam_step_reference(self.master, g, self.m, self.v,
                                      self.step_count, lr, b1, b2, self.eps)
                self.flat.flat_w.copy_(self.master.to(self.flat.flat_w.dtype))
            self.acc.zero_()
            return
        live = [(p, st) for p, st in zip(self.params, self.state)
                if st["acc_live"]]
        skip, scale = (self._host_guard([st["acc"] for _, st in live])
                       if self.guarded else (False, 1.0))
        for p, st in live:
            if not skip:
                g = st["acc"] if scale == 1.0 else st["acc"] * scale
                R.adam_step_reference(st["master"], g, st["m"], st["v"],
                                      self.step_count, lr, b1, b2, self.eps)
                p.data.copy_(st["master"].to(p.dtype))
            st["acc"].zero_()
            st["acc_live"] = False

    # -- checkpointing (C16) ------------------------------------------------
    def state_dict(self):
        d = {"step": self.step_count,
             "skipped_steps": self.skipped_steps,
             "d_model": self.schedule.d_model,
             "warmup_steps": self.schedule.warmup_steps}
        if self.flat is not None:
            d.update(master=self.master, m=self.m, v=self.v)
        else:
            d.update(state=[{k: st[k] for k in ("m", "v", "master")}
                            for st in self.state])
        return d

    def load_state_dict(self, d):
        self.step_count = d["step"]
        # absent in checkpoints written before the guard existed
        self._skipped = int(d.get("skipped_steps", 0))
        if self._gn_stats is not None:
            self._gn_stats[3] = float(self._skipped)
        if hasattr(self, "_step_t"):  # keep captured-graph schedule in sync
            self._step_t.fill_(self.step_count)
        if self.flat is not None:
            self.master.copy_(d["master"].to(self.master.device))
            self.m.copy_(d["m"].to(self.m.device))
            self.v.copy_(d["v"].to(self.v.device))
            self.flat.flat_w.copy_(self.master.to(self.flat.flat_w.dtype))
        else:
            for st, sd in zip(self.state, d["state"]):
                for k in ("m", "v", "master"):
                    st[k].copy_(sd[k].to(st[k].device))
            for p, st in zip(self.params, self.state):
                p.data.copy_(st["master"].to(p.dtype))
