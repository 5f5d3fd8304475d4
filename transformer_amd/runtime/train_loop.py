"""Training runtime (C17/C18/C19 — reference train.py:37-213) and the DP
subclass (C20 — reference distributed_train.py:25-121).

Train owns the optimizer (Noam-Adam), loss (padding-masked CE, sum/global
batch — SURVEY.md §8 Q4), metrics, summary writers and checkpoint manager,
exactly the reference's responsibilities (train.py:64-80).  Deliberate
behaviour fixes over the reference, per SURVEY.md §8: masked accuracy (Q5),
tgt-tokenizer ids + EOS stop in predict (Q6), checkpoint cadence intent
"every 5 epochs or at end" (Q7), fixed eval-batch count (Q8).
"""

from __future__ import annotations

import time

import torch

from .. import ops
from ..runtime.optimizer import NoamAdam
from ..runtime.metrics import Mean
from ..runtime.summary import SummaryWriter
from ..runtime.checkpoint import CheckpointManager


class Train:
    def __init__(self, epochs, enable_function, transformer, src_tokenizer,
                 tgt_tokenizer, batch_size, train_log_dir, test_log_dir,
                 max_ckpt_keep, ckpt_path, d_model,
                 warmup_steps: int = 60000, label_smoothing: float = 0.0,
                 device=None, log_interval: int = 100, eval_steps: int = 50,
                 max_decode_len: int = 10, is_rank0: bool = True,
                 use_flat: bool | None = None,
                 clip_grad_norm: float = 0.0,
                 skip_nonfinite_grads: bool = False,
                 grad_accum_steps: int = 1,
                 pack_sequences: bool = False):
        self.epochs = epochs
        self.enable_function = enable_function
        self.transformer = transformer
        self.src_tokenizer = src_tokenizer
        self.tgt_tokenizer = tgt_tokenizer
        self.batch_size = batch_size  # GLOBAL batch (loss scale, Q4)
        # micro-batches per optimizer step; the loss of every micro-batch is
        # still divided by the GLOBAL batch, so the micro-gradients simply
        # sum to the full-batch gradient
        self.grad_accum_steps = int(grad_accum_steps)
        self.label_smoothing = label_smoothing
        self.log_interval = log_interval
        self.eval_steps = eval_steps
        self.max_decode_len = max_decode_len
        self.is_rank0 = is_rank0
        p0 = next(transformer.parameters())
        self.device = device if device is not None else p0.device

        self.optimizer = NoamAdam(transformer, d_model, warmup_steps,
                                  use_flat=use_flat,
                                  max_grad_norm=clip_grad_norm,
                                  skip_nonfinite=skip_nonfinite_grads,
                                  accum_steps=self.grad_accum_steps)
        self.train_loss = Mean("train_loss")
        self.test_loss = Mean("test_loss")
        self.train_accuracy = Mean("train_accuracy")
        self.test_accuracy = Mean("test_accuracy")
        self.train_summary_writer = (SummaryWriter(train_log_dir)
                                     if (is_rank0 and train_log_dir) else None)
        self.test_summary_writer = (SummaryWriter(test_log_dir)
                                    if (is_rank0 and test_log_dir) else None)
        self.ckpt_manager = CheckpointManager(transformer, self.optimizer,
                                              ckpt_path, max_ckpt_keep)
        self.pack_sequences = bool(pack_sequences)
        if self.pack_sequences:
            self._refuse_packed_capture()

    _PACKED_CAPTURE_MSG = (
        "--pack_sequences is not supported together with --enable_function "
        "(the HIP-graph captured train step has no packed-batch buffers "
        "yet); run with --noenable_function")

    def _refuse_packed_capture(self):
        """Packed batches run the eager step only.  Fail loudly — at start-up
        when the flag is set — instead of falling back silently."""
        if self._graph_eligible():
            raise ValueError(self._PACKED_CAPTURE_MSG)

    # -- loss (C13, reference train.py:83-88) -------------------------------
    def loss_function(self, real, pred):
        return ops.masked_cross_entropy(pred, real, self.batch_size,
                                        self.label_smoothing)

    # -- steps (C18, reference train.py:124-156) ----------------------------
    def _grad_sync(self):
        """Hook point for the DP subclass (bucket finalize)."""

    def _graph_eligible(self) -> bool:
        """enable_function (Q12) -> HIP-graph capture of the whole step.
        DP>1 keeps the eager step (collectives are not captured)."""
        import torch.distributed as dist
        return (self.enable_function and self.device.type == "cuda"
                and self.optimizer.flat is not None
                and not (dist.is_available() and dist.is_initialized()
                         and dist.get_world_size() > 1))

    def _grad_sync_accum(self):
        """Hook point for the DP subclass (accumulator all-reduce)."""

    def _accum_train_step(self, src, tar):
        """One optimizer step over grad_accum_steps micro-batches:
        consecutive ceil(B/N)-row chunks of the batch (a short tail chunk is
        fine, empty ones are skipped), forward + backward on each with the
        unchanged loss_function, fp32 accumulation, one optimizer step.  The
        step loss is the sum of the micro losses and the accuracy counts are
        summed; both come to the host once per optimizer step."""
        n = self.grad_accum_steps
        rows = -(-src.shape[0] // n)
        if self._graph_eligible():
            cap = getattr(self, "_captured", None)
            if cap is None or not cap.fits(src, tar):
                from .graph import CapturedAccumTrainStep
                cap = CapturedAccumTrainStep(
                    self.transformer, self.optimizer, self.loss_function,
                    (rows, src.shape[1]), (rows, tar.shape[1]), self.device)
                self._captured = cap
            loss, c, t = cap(src, tar)
            self.train_loss.update(loss)
            self.train_accuracy.update(c / max(t, 1), weight=t)
            return torch.tensor(loss)

        def micro():
            for i in range(n):
                s = src[i * rows:(i + 1) * rows]
                t = tar[i * rows:(i + 1) * rows]
                if s.shape[0]:
                    yield ((s, t[:, :-1].contiguous()),
                           t[:, 1:].contiguous())
        return self._accum_eager(micro())

    def _accum_eager(self, micro):
        """Eager accumulation over an iterable of (model input, labels)."""
        sums = None
        for model_in, tar_real in micro:
            predictions, _ = self.transformer(model_in, training=True)
            loss = self.loss_function(tar_real, predictions)
            # per micro-batch: the embedding scatter and the column-sum
            # reductions accumulate into flat_g and need it clear
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.accumulate()
            with torch.no_grad():
                part = torch.cat([
                    loss.detach().reshape(1).to(torch.float64),
                    ops.masked_accuracy_counts_t(predictions.detach(),
                                                 tar_real)])
                sums = part if sums is None else sums + part
        if sums is None:
            raise ValueError("train_step got an empty batch")
        self._grad_sync_accum()
        # clip/skip (if enabled) acts on the all-reduced accumulator
        self.optimizer.step()
        loss, c, t = sums.tolist()      # the step's only host read
        self.train_loss.update(loss)
        self.train_accuracy.update(c / max(t, 1), weight=t)
        return sums[0].to(torch.float32)

    def _captured_step(self, src, tar):
        cap = getattr(self, "_captured", None)
        if cap is None or not cap.fits(src, tar):
            from .graph import CapturedTrainStep
            cap = CapturedTrainStep(self.transformer, self.optimizer,
                                    self.loss_function, tuple(src.shape),
                                    tuple(tar.shape), self.device)
            self._captured = cap
        loss = cap(src, tar)
        self.train_loss.update(loss.item())
        c, t = ops.masked_accuracy_counts(cap.logits, cap.tar_real)
        self.train_accuracy.update(c / max(t, 1), weight=t)
        return loss

    def _packed_train_step(self, pb):
        """train_step on a PackedBatch: the same loss_function with the same
        GLOBAL batch divisor over the packed (rows, L) logits and labels —
        the pad mask of the CE and of the accuracy drops id-0 slots — and
        the same optimizer step.  Gradient accumulation chunks ROWS."""
        self._refuse_packed_capture()
        n = self.grad_accum_steps
        if n > 1:
            rows = -(-pb.src.shape[0] // n)
            return self._accum_eager(
                (c, c.tar_real) for c in
                (pb.rows(i * rows, (i + 1) * rows) for i in range(n))
                if c.src.shape[0])
        predictions, _ = self.transformer(pb, training=True)
        loss = self.loss_function(pb.tar_real, predictions)
        self.optimizer.zero_grad()
        loss.backward()
        self._grad_sync()
        self.optimizer.step()
        self.train_loss.update(loss.detach().item())
        c, t = ops.masked_accuracy_counts(predictions.detach(), pb.tar_real)
        self.train_accuracy.update(c / max(t, 1), weight=t)
        return loss

    def train_step(self, inputs):
        if hasattr(inputs, "src_seg"):      # data.PackedBatch
            return self._packed_train_step(
                inputs.to(self.device, non_blocking=True))
        src, tar = inputs
        src = src.to(self.device, non_blocking=True)
        tar = tar.to(self.device, non_blocking=True)
        if self.grad_accum_steps > 1:
            return self._accum_train_step(src, tar)
        if self._graph_eligible():
            return self._captured_step(src, tar)
        tar_inp, tar_real = tar[:, :-1].contiguous(), tar[:, 1:].contiguous()

        predictions, _ = self.transformer((src, tar_inp), training=True)
        loss = self.loss_function(tar_real, predictions)
        self.optimizer.zero_grad()
        loss.backward()
        self._grad_sync()
        # clip/skip (if enabled) acts on the all-reduced flat gradient, so
        # every rank takes the identical decision with no extra collective
        self.optimizer.step()

        self.train_loss.update(loss.detach().item())
        # token-weighted accumulation: batches contribute by real-token
        # count, matching the reference's streaming accuracy semantics
        c, t = ops.masked_accuracy_counts(predictions.detach(), tar_real)
        self.train_accuracy.update(c / max(t, 1), weight=t)
        return loss

    @torch.no_grad()
    def test_step(self, inputs):
        src, tar = inputs
        src = src.to(self.device, non_blocking=True)
        tar = tar.to(self.device, non_blocking=True)
        tar_inp, tar_real = tar[:, :-1].contiguous(), tar[:, 1:].contiguous()
        predictions, _ = self.transformer((src, tar_inp), training=False)
        t_loss = self.loss_function(tar_real, predictions)
        self.test_loss.update(t_loss.item())
        c, t = ops.masked_accuracy_counts(predictions, tar_real)
        self.test_accuracy.update(c / max(t, 1), weight=t)

    # -- greedy inference (C19, reference train.py:91-121; Q6 fixes) --------
    @torch.no_grad()
    def predict(self, input_sentence):
        """Greedy decode one sentence (str) or a batch (list[str]) — the
        reference accepted a list but decoded only sequentially; here a
        list runs as one padded batch through the KV-cached decoder."""
        batch = (list(input_sentence)
                 if isinstance(input_sentence, (list, tuple))
                 else [input_sentence])
        src_start = self.src_tokenizer.vocab_size
        src_end = src_start + 1
        tgt_start = self.tgt_tokenizer.vocab_size
        tgt_end = tgt_start + 1
        seqs = [[src_start] + self.src_tokenizer.encode(t) + [src_end]
                for t in batch]
        S = max(len(s) for s in seqs)
        encoder_input = torch.zeros(len(seqs), S, dtype=torch.int64,
                                    device=self.device)  # pad id 0
        for i, s in enumerate(seqs):
            encoder_input[i, :len(s)] = torch.tensor(s, dtype=torch.int64)
        # KV-cached greedy decode: encoder runs once, each step is O(1) in
        # prefix length (SURVEY.md §3.3 — vs the reference's full re-run per
        # token, train.py:109-118).
        from ..models.transformer import greedy_decode
        output = greedy_decode(self.transformer, encoder_input,
                               tgt_start, tgt_end,
                               max_len=self.max_decode_len)
        if isinstance(input_sentence, (list, tuple)):
            return output.cpu()
        return output.squeeze(0).cpu()

    def load_ckpt(self):
        meta = self.ckpt_manager.restore()
        if meta is not None:
            print("Latest checkpoint restored!!")
        return meta

    # -- epoch loop (C17, reference train.py:167-213) -----------------------
    def _run_eval(self, test_dataset):
        self.test_loss.reset()
        self.test_accuracy.reset()
        n = 0
        for batch in test_dataset:
            self.test_step(batch)
            n += 1
            if n >= self.eval_steps:
                break

    def _save_if_due(self, epoch: int, step: int):
        # Q7 intent: save every 5 epochs or at the end.
        if self.is_rank0 and ((epoch + 1) % 5 == 0 or (epoch + 1) == self.epochs):
            self.ckpt_manager.save(step, epoch)

    def install_signal_handler(self):
        """Failure handling: SIGTERM/SIGINT requests a clean
        stop — the loop finishes the current step, checkpoints, and
        returns, so training resumes from the interruption point."""
        import signal

        def _handler(signum, _frame):
            self._stop_requested = True
            if self.is_rank0:
                print(f"signal {signum}: will checkpoint and stop "
                      "after the current step")

        signal.signal(signal.SIGTERM, _handler)
        signal.signal(signal.SIGINT, _handler)

    def trace_steps(self, train_dataset, n_steps: int, trace_dir: str):
        """Tracing/profiling: run n_steps under
        torch.profiler (Kineto-ROCm) and write a chrome trace to
        trace_dir.  Separate from the timed loops."""
        from torch.profiler import profile, ProfilerActivity
        import os
        os.makedirs(trace_dir, exist_ok=True)
        it = iter(train_dataset)
        acts = [ProfilerActivity.CPU]
        if self.device.type == "cuda":
            acts.append(ProfilerActivity.CUDA)
        with profile(activities=acts) as prof:
            for _ in range(n_steps):
                try:
                    self.train_step(next(it))
                except StopIteration:
                    break
        path = os.path.join(trace_dir, "train_steps.json")
        prof.export_chrome_trace(path)
        if self.is_rank0:
            print(f"trace written: {path}")
        return path

    def training_loop(self, train_dataset, test_dataset):
        template = ("Epoch {}  Loss {:.4f} Accuracy {:.4f}, "
                    "Test Loss {:.4f}, Test Accuracy {:.4f}")
        step = self.optimizer.step_count
        self._stop_requested = getattr(self, "_stop_requested", False)
        for epoch in range(self.epochs):
            start = time.time()
            for m in (self.train_loss, self.train_accuracy,
                      self.test_loss, self.test_accuracy):
                m.reset()
            if hasattr(train_dataset, "set_epoch"):
                train_dataset.set_epoch(epoch)

            interval_tokens = 0
            interval_t0 = time.time()
            for inputs in train_dataset:
                if hasattr(inputs, "src_seg"):
                    # packed: count REAL tokens (a padded batch counts its
                    # slots, as before)
                    interval_tokens += inputs.real_tokens()
                else:
                    src, tar = inputs
                    interval_tokens += src.numel() + tar.numel()
                self.train_step(inputs)
                step += 1
                if self._stop_requested:
                    if self.is_rank0:
                        self.ckpt_manager.save(step, epoch)
                        print("checkpointed on stop request; exiting loop")
                    return
                if step % self.log_interval == 0:
                    # tokens/sec over the interval (the north-star metric;
                    # SURVEY.md §5 metrics) — whole-job rate in DP
                    import torch.distributed as dist
                    world = (dist.get_world_size()
                             if dist.is_available() and dist.is_initialized()
                             else 1)
                    dt = max(time.time() - interval_t0, 1e-9)
                    tps = interval_tokens * world / dt
                    interval_tokens = 0
                    interval_t0 = time.time()
                    self._run_eval(test_dataset)
                    if self.is_rank0:
                        print(template.format(
                            epoch + 1, self.train_loss.result(),
                            self.train_accuracy.result(),
                            self.test_loss.result(),
                            self.test_accuracy.result())
                            + f", {tps:,.0f} tokens/s")
                    if self.train_summary_writer:
                        self.train_summary_writer.add_scalar(
                            "tokens_per_sec", tps, step)
                        if self.optimizer.guarded:
                            # the only device reads of the guard: once per
                            # interval, so graph replays stay sync-free
                            self.train_summary_writer.add_scalar(
                                "grad_norm",
                                self.optimizer.last_grad_norm(), step)
                            self.train_summary_writer.add_scalar(
                                "skipped_steps",
                                self.optimizer.skipped_steps, step)

            # end-of-epoch eval so the epoch summary always reflects a real
            # test sweep (Q8/Q10: the reference could silently report
            # nothing when steps/epoch < log_interval or the test files
            # were missing).
            self._run_eval(test_dataset)
            for m in (self.train_loss, self.train_accuracy,
                      self.test_loss, self.test_accuracy):
                m.sync()
            if self.train_summary_writer:
                self.train_summary_writer.add_scalar("loss", self.train_loss.result(), epoch)
                self.train_summary_writer.add_scalar("accuracy", self.train_accuracy.result(), epoch)
            if self.test_summary_writer:
                self.test_summary_writer.add_scalar("loss", self.test_loss.result(), epoch)
                self.test_summary_writer.add_scalar("accuracy", self.test_accuracy.result(), epoch)
            self._save_if_due(epoch, step)
            if self.is_rank0:
                print(template.format(
                    epoch + 1, self.train_loss.result(),
                    self.train_accuracy.result(),
                    self.test_loss.result(), self.test_accuracy.result()))
                print(f"Time taken for 1 epoch: {time.time() - start} secs\n")


class DistributedTrain(Train):
    """DP training over N GPUs (C20).  Differences from Train: bucketed
    RCCL all-reduce finalization before each optimizer step, X1 parameter
    broadcast at start, rank-0-only logging/checkpointing."""

    def __init__(self, *args, ddp=None, **kwargs):
        kwargs.setdefault("use_flat", True)
        super().__init__(*args, **kwargs)
        if ddp is None:
            import os
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() \
                    and (dist.get_world_size() > 1
                         or os.environ.get("TFMX_DDP_FORCE") == "1"):
                from ..parallel import BucketedDataParallel
                ddp = BucketedDataParallel(self.optimizer.flat)
        self.ddp = ddp
        if ddp is not None:
            ddp.broadcast_parameters()
            if self.grad_accum_steps > 1:
                # one all-reduce per bucket per OPTIMIZER step, on the
                # accumulator, not one per micro backward
                ddp.set_accumulate(True)

    def _grad_sync(self):
        if self.ddp is not None:
            self.ddp.finalize()

    def _grad_sync_accum(self):
        if self.ddp is not None:
            self.ddp.finalize_accum(self.optimizer.acc)
