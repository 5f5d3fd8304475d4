"""HIP-graph captured training step (the reference's
`--enable_function` tf.function toggle maps to capturing the whole
fwd+bwd+Adam step into one hipGraph and replaying it).

The step is captured once with static input/output buffers; each call
copies the batch into the static buffers and replays the graph — ~1100
kernel launches collapse into one hipGraphLaunch, removing host launch
overhead and CPU jitter (which matters most for multi-rank lockstep).

Replay-variant state lives on device:
  - the Noam schedule / Adam bias corrections read a device step tensor
    advanced in-graph (ops adam_coefs kernel, optimizer.step_captured);
  - dropout seeds combine that step tensor with a per-call-site salt
    (ops.functional.set_graph_rng), so masks differ every replay.

DP>1 is not captured (RCCL collectives inside graph capture are not
supported on this stack) — callers fall back to the eager step.

With gradient accumulation (NoamAdam accum_steps > 1) the step is TWO graphs,
CapturedAccumTrainStep: a micro graph replayed once per micro-batch and an
apply graph replayed once per optimizer step.
"""

from __future__ import annotations

import torch


class CapturedTrainStep:
    """Captures fwd+loss+bwd+opt for fixed-shape (src, tar) batches."""

    def __init__(self, model, optimizer, loss_fn, src_shape, tar_shape,
                 device, warmup_iters: int = 2):
        from .. import ops
        self.model = model
        self.opt = optimizer
        self.loss_fn = loss_fn
        self.src = torch.zeros(src_shape, dtype=torch.int64, device=device)
        self.tar = torch.zeros(tar_shape, dtype=torch.int64, device=device)

        step_t, _ = optimizer.graph_state()

        def run():
            tar_inp = self.tar[:, :-1].contiguous()
            tar_real = self.tar[:, 1:].contiguous()
            logits, _ = model((self.src, tar_inp), training=True)
            loss = loss_fn(tar_real, logits)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step_captured()
            return loss, logits, tar_real

        # warmup on a side stream (cuDNN-style), then capture.  The warmup
        # iterations execute REAL fwd+bwd+Adam steps on the zero-filled
        # static buffers — harmless at first capture (m=v=0) but a
        # mid-training recapture (batch exceeding the captured shape) would
        # apply zero-gradient Adam updates to live state.  Snapshot the fp32
        # master + m/v around the warmup so recapture is state-neutral.
        ops.functional.set_graph_rng(step_t)
        snap = (optimizer.master.clone(), optimizer.m.clone(),
                optimizer.v.clone())
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(warmup_iters):
                    run()
            torch.cuda.current_stream().wait_stream(s)
            optimizer.master.copy_(snap[0])
            optimizer.m.copy_(snap[1])
            optimizer.v.copy_(snap[2])
            optimizer.flat.flat_w.copy_(
                optimizer.master.to(optimizer.flat.flat_w.dtype))
            del snap

            # make the weight-derived caches (transposed-weight buffers)
            # stale so the capture RECORDS their batched refresh — replays
            # then refresh them after each in-graph Adam step.  The
            # descriptor table must exist BEFORE capture (H2D copy).
            ops.functional.prepare_weight_caches()
            ops.functional.bump_weight_version()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.loss, self.logits, self.tar_real = run()
        finally:
            ops.functional.set_graph_rng(None)
        # warmup advanced the device step; resync to the host counter
        step_t.fill_(optimizer.step_count)

    def fits(self, src, tar) -> bool:
        return (src.shape[0] <= self.src.shape[0]
                and src.shape[1] <= self.src.shape[1]
                and tar.shape[0] <= self.tar.shape[0]
                and tar.shape[1] <= self.tar.shape[1])

    def __call__(self, src: torch.Tensor, tar: torch.Tensor) -> torch.Tensor:
        """Replay on a batch; smaller batches are padded with pad id 0
        (zero rows are fully masked by kv_pad/the CE pad mask)."""
        if src.shape == self.src.shape and tar.shape == self.tar.shape:
            self.src.copy_(src, non_blocking=True)
            self.tar.copy_(tar, non_blocking=True)
        else:
            self.src.zero_()
            self.tar.zero_()
            self.src[:src.shape[0], :src.shape[1]].copy_(src,
                                                         non_blocking=True)
            self.tar[:tar.shape[0], :tar.shape[1]].copy_(tar,
                                                         non_blocking=True)
        self.graph.replay()
        self.opt.step_count += 1
        from ..ops import functional as _F
        _F.bump_weight_version()  # replay updated weights in-graph
        return self.loss


class CapturedAccumTrainStep:
    """Captured optimizer step over N micro-batches (gradient accumulation).

    Micro graph, at the micro shape (ceil(B/N), S), replayed per chunk:
        micro counter += 1, zero_grad, forward, loss, backward,
        optimizer.accumulate(), loss / accuracy-count sums.
    Apply graph, replayed once per optimizer step:
        norm pass (if guarded), adam_fused_dev_acc (which re-zeroes the
        accumulator), batched refresh of the cached W^T buffers.

    Dropout seeds: the Adam step tensor advances only in the apply graph, so
    all N micro replays of one optimizer step would draw identical masks
    from it.  The micro graph therefore owns an int64 device counter that it
    advances itself on every replay, installed through set_graph_rng.

    Cached W^T refresh: recorded in the APPLY graph, right after the Adam
    kernel.  The micro graph is captured with the caches current, so it
    records no refresh; the first micro replay after an apply sees the new
    weights' transposes, and the refresh runs once per optimizer step, not N
    times.  apply() still bumps the host-side weight version: replays never
    look at it, and eager code that runs a backward between captured steps
    then refreshes once more instead of trusting a registry the graph may
    not have covered.

    The loss sum and the accuracy counts accumulate on the device and come
    to the host once per optimizer step."""

    def __init__(self, model, optimizer, loss_fn, src_shape, tar_shape,
                 device, warmup_iters: int = 2):
        from .. import ops
        if optimizer.acc is None:
            raise ValueError("CapturedAccumTrainStep needs NoamAdam("
                             "accum_steps > 1) on the flat GPU path")
        self.model = model
        self.opt = optimizer
        self.loss_fn = loss_fn
        self.n_micro = optimizer.accum_steps
        # static buffers at the MICRO shape
        self.src = torch.zeros(src_shape, dtype=torch.int64, device=device)
        self.tar = torch.zeros(tar_shape, dtype=torch.int64, device=device)
        # micro replay counter = dropout seed epoch; starts past every value
        # an earlier capture of this run can have used
        self.micro_t = torch.tensor(
            [optimizer.step_count * self.n_micro], dtype=torch.int64,
            device=device)
        # per-optimizer-step sums: [loss, correct, total]
        self.sums = torch.zeros(3, dtype=torch.float64, device=device)

        step_t, _ = optimizer.graph_state()

        def run_micro():
            self.micro_t.add_(1)
            tar_inp = self.tar[:, :-1].contiguous()
            tar_real = self.tar[:, 1:].contiguous()
            logits, _ = model((self.src, tar_inp), training=True)
            loss = loss_fn(tar_real, logits)
            optimizer.zero_grad()
            loss.backward()
            optimizer.accumulate()
            with torch.no_grad():
                self.sums[0:1].add_(loss.detach().reshape(1))
                self.sums[1:3].add_(
                    ops.masked_accuracy_counts_t(logits.detach(), tar_real))
            return loss, logits, tar_real

        def run_apply():
            optimizer.step_captured()
            ops.functional.refresh_weight_caches()

        # Warmup on a side stream runs REAL micro + apply steps on the
        # zero-filled static buffers; snapshot the fp32 master + m/v around
        # it so a mid-training recapture is state-neutral.  The apply leaves
        # the accumulator zero; discard_accum() makes that unconditional.
        ops.functional.set_graph_rng(self.micro_t)
        snap = (optimizer.master.clone(), optimizer.m.clone(),
                optimizer.v.clone())
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(warmup_iters):
                    run_micro()
                    run_apply()
            torch.cuda.current_stream().wait_stream(s)
            optimizer.master.copy_(snap[0])
            optimizer.m.copy_(snap[1])
            optimizer.v.copy_(snap[2])
            optimizer.flat.flat_w.copy_(
                optimizer.master.to(optimizer.flat.flat_w.dtype))
            optimizer.discard_accum()
            del snap

            # Bring the W^T caches up to date with the restored weights
            # BEFORE capturing (this also builds the descriptor table, a
            # host->device copy that is illegal during capture): the micro
            # graph must record no refresh, the apply graph records one.
            ops.functional.bump_weight_version()
            ops.functional.refresh_weight_caches()
            ops.functional.set_graph_rng(self.micro_t)  # salts restart at 0
            self.micro_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.micro_graph):
                self.loss, self.logits, self.tar_real = run_micro()
            self.apply_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.apply_graph):
                run_apply()
        finally:
            ops.functional.set_graph_rng(None)
        # warmup advanced the device step and the sums; resync
        step_t.fill_(optimizer.step_count)
        self.sums.zero_()

    def fits(self, src, tar) -> bool:
        """Whether the micro-batches of this batch fit the captured shape."""
        rows = -(-src.shape[0] // self.n_micro)
        return (rows <= self.src.shape[0]
                and src.shape[1] <= self.src.shape[1]
                and tar.shape[1] <= self.tar.shape[1])

    def micro(self, src: torch.Tensor, tar: torch.Tensor) -> torch.Tensor:
        """Replay the micro graph on one micro-batch (zero-padded to the
        captured shape; zero rows are fully masked).  Returns the static
        micro-loss tensor."""
        if src.shape == self.src.shape and tar.shape == self.tar.shape:
            self.src.copy_(src, non_blocking=True)
            self.tar.copy_(tar, non_blocking=True)
        else:
            self.src.zero_()
            self.tar.zero_()
            self.src[:src.shape[0], :src.shape[1]].copy_(src,
                                                         non_blocking=True)
            self.tar[:tar.shape[0], :tar.shape[1]].copy_(tar,
                                                         non_blocking=True)
        self.micro_graph.replay()
        return self.loss

    def apply(self):
        """Replay the apply graph: one optimizer step from the accumulator."""
        self.apply_graph.replay()
        self.opt.step_count += 1
        from ..ops import functional as _F
        _F.bump_weight_version()  # replay updated weights in-graph

    def __call__(self, src: torch.Tensor, tar: torch.Tensor):
        """One optimizer step on a full batch, split along dim 0 into
        n_micro consecutive ceil(B/N)-row chunks (empty chunks skipped).
        Returns (loss, correct, total) as host floats — the only host read
        of the step."""
        rows = -(-src.shape[0] // self.n_micro)
        for i in range(self.n_micro):
            s, t = src[i * rows:(i + 1) * rows], tar[i * rows:(i + 1) * rows]
            if s.shape[0] == 0:
                continue
            self.micro(s, t)
        self.apply()
        loss, correct, total = self.sums.tolist()
        self.sums.zero_()
        return loss, correct, total
