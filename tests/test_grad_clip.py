"""Global-norm gradient clipping and non-finite step skipping — CPU paths
(ops/reference.py oracle functions, NoamAdam flat and per-parameter paths,
flags, checkpoint round-trip, gloo world-2).

Adam is almost scale-invariant (eps = 1e-9), so clipping barely shows in the
weights; the tests read it off the first moment instead: after one step from
zero state, ||m|| = (1 - beta1) * min(||g||, max_norm)."""

import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from transformer_amd.config import parse_flags, flags_dict
from transformer_amd.models import Transformer
from transformer_amd.ops import reference as R
from transformer_amd.parallel import BucketedDataParallel
from transformer_amd.runtime import NoamAdam

MAX_NORM = 0.25  # well below the toy model's initial gradient norm (> 1)


def _model():
    torch.manual_seed(0)
    return Transformer(num_layers=1, d_model=16, num_heads=2, dff=32,
                       input_vocab_size=50, target_vocab_size=50, rate=0.0,
                       max_position=32)


def _batch(global_batch=4, seq=6):
    torch.manual_seed(99)
    return (torch.randint(1, 50, (global_batch, seq)),
            torch.randint(1, 50, (global_batch, seq)))


def _backward(model, opt, lo=None, hi=None):
    inp, tar = _batch()
    b = inp.shape[0]
    lo, hi = (0, b) if lo is None else (lo, hi)
    logits, _ = model((inp[lo:hi], tar[lo:hi]), training=True)
    loss = R.masked_cross_entropy(logits, tar[lo:hi], batch_size=b)
    opt.zero_grad()
    loss.backward()


def _state(opt):
    """(master, m, v) as flat fp32 tensors, for either optimizer layout."""
    if opt.flat is not None:
        return opt.master, opt.m, opt.v
    cat = lambda k: torch.cat([st[k].reshape(-1) for st in opt.state])
    return cat("master"), cat("m"), cat("v")


def _weights(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


# ---------------------------------------------------------------------------
# reference functions
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e4])
def test_reference_matches_torch_clip(max_norm):
    torch.manual_seed(3)
    grads = [torch.randn(s) for s in [(7,), (13, 5), (64,), (3, 3, 3)]]
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    norm = R.global_grad_norm_reference(grads)
    assert norm == pytest.approx(float(total), rel=1e-6)
    scale = R.clip_scale_reference(norm, max_norm)
    if norm <= max_norm:
        assert scale == 1.0
    else:
        assert scale == max_norm / (norm + 1e-6)
    for p, g in zip(params, grads):
        assert torch.allclose(p.grad, g * scale, rtol=1e-6, atol=0)


def test_reference_rule_edges():
    assert R.clip_scale_reference(5.0, 0.0) == 1.0      # off
    assert R.clip_scale_reference(5.0, -1.0) == 1.0     # off
    assert R.clip_scale_reference(2.0, 2.0) == 1.0      # on the bound
    assert R.clip_scale_reference(4.0, 2.0) == 2.0 / (4.0 + 1e-6)
    assert math.isinf(R.global_grad_norm_reference(
        [torch.tensor([1.0, float("inf")])]))
    assert math.isnan(R.global_grad_norm_reference(
        [torch.tensor([1.0, float("nan")])]))


# ---------------------------------------------------------------------------
# NoamAdam: clipping
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("use_flat", [True, False])
def test_first_moment_identity(use_flat):
    model = _model()
    opt = NoamAdam(model, 16, warmup_steps=10, use_flat=use_flat,
                   max_grad_norm=MAX_NORM)
    _backward(model, opt)
    opt.step()
    norm = opt.last_grad_norm()
    assert norm > 4 * MAX_NORM, norm  # clipping really engaged
    _, m, _ = _state(opt)
    # scale = max/(norm + 1e-6) puts ||g*scale|| within 1e-6/norm of max
    want = (1 - opt.betas[0]) * min(norm, MAX_NORM)
    assert float(m.double().norm()) == pytest.approx(want, rel=1e-5)
    assert opt.skipped_steps == 0


@pytest.mark.parametrize("use_flat", [True, False])
def test_large_max_norm_equals_feature_off(use_flat):
    ma, mb = _model(), _model()
    oa = NoamAdam(ma, 16, warmup_steps=10, use_flat=use_flat)
    ob = NoamAdam(mb, 16, warmup_steps=10, use_flat=use_flat,
                  max_grad_norm=1e6, skip_nonfinite=True)
    assert not oa.guarded and ob.guarded
    for _ in range(2):
        _backward(ma, oa)
        oa.step()
        _backward(mb, ob)
        ob.step()
    assert ob.last_grad_norm() < 1e6
    for a, b in zip(_state(oa), _state(ob)):
        assert torch.equal(a, b)
    assert torch.equal(_weights(ma), _weights(mb))


# ---------------------------------------------------------------------------
# NoamAdam: non-finite steps
# ---------------------------------------------------------------------------

def _poison(model, opt, value):
    if opt.flat is not None:
        opt.flat.flat_g[5] = value
    else:
        next(p for p in opt.params if p.grad is not None).grad.view(-1)[5] = value


@pytest.mark.parametrize("use_flat", [True, False])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_step_is_skipped(use_flat, bad):
    model = _model()
    opt = NoamAdam(model, 16, warmup_steps=10, use_flat=use_flat,
                   max_grad_norm=MAX_NORM, skip_nonfinite=True)
    _backward(model, opt)
    opt.step()  # one real step so m/v are not trivially zero
    before = [t.clone() for t in _state(opt)] + [_weights(model).clone()]
    _backward(model, opt)
    _poison(model, opt, bad)
    opt.step()
    after = list(_state(opt)) + [_weights(model)]
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert opt.skipped_steps == 1
    assert opt.step_count == 2  # the schedule still advances
    # and training goes on afterwards
    _backward(model, opt)
    opt.step()
    assert opt.skipped_steps == 1 and opt.step_count == 3
    assert not torch.equal(before[0], _state(opt)[0])
    assert torch.isfinite(_weights(model)).all()


def test_fp32_overflow_counts_as_nonfinite():
    """A finite gradient whose fp32 sum of squares overflows is skipped too
    (the documented rule of the device kernel, mirrored on the CPU)."""
    model = _model()
    opt = NoamAdam(model, 16, use_flat=True, skip_nonfinite=True)
    _backward(model, opt)
    opt.flat.flat_g[5] = 3e19  # 9e38 > FLT_MAX
    w0 = _weights(model).clone()
    opt.step()
    assert opt.skipped_steps == 1
    assert torch.equal(w0, _weights(model))


@pytest.mark.parametrize("use_flat", [True, False])
def test_guard_off_keeps_old_behaviour(use_flat):
    """skip_nonfinite=False, max_grad_norm=0: the old code path, which lets
    a non-finite gradient through exactly as a default optimizer does."""
    ma, mb = _model(), _model()
    oa = NoamAdam(ma, 16, warmup_steps=10, use_flat=use_flat)
    ob = NoamAdam(mb, 16, warmup_steps=10, use_flat=use_flat,
                  max_grad_norm=0.0, skip_nonfinite=False)
    assert not ob.guarded
    for model, opt in ((ma, oa), (mb, ob)):
        _backward(model, opt)
        _poison(model, opt, float("nan"))
        opt.step()
    wa, wb = _weights(ma), _weights(mb)
    assert torch.isnan(wa).any()
    assert torch.equal(torch.isnan(wa), torch.isnan(wb))
    assert torch.equal(torch.nan_to_num(wa), torch.nan_to_num(wb))
    assert ob.skipped_steps == 0


# ---------------------------------------------------------------------------
# checkpointing
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("use_flat", [True, False])
def test_state_dict_keeps_skipped_steps(use_flat):
    model = _model()
    opt = NoamAdam(model, 16, use_flat=use_flat, skip_nonfinite=True)
    _backward(model, opt)
    _poison(model, opt, float("inf"))
    opt.step()
    sd = opt.state_dict()
    assert sd["skipped_steps"] == 1

    opt2 = NoamAdam(_model(), 16, use_flat=use_flat, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    assert opt2.skipped_steps == 1 and opt2.step_count == 1

    old = {k: v for k, v in sd.items() if k != "skipped_steps"}
    opt3 = NoamAdam(_model(), 16, use_flat=use_flat, skip_nonfinite=True)
    opt3.load_state_dict(old)  # checkpoint from before the feature
    assert opt3.skipped_steps == 0 and opt3.step_count == 1


# ---------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------

def test_flags():
    d = flags_dict(parse_flags([]))
    assert d["clip_grad_norm"] == 0.0
    assert d["skip_nonfinite_grads"] is False
    a = parse_flags(["--clip_grad_norm=1.5", "--skip_nonfinite_grads"])
    assert a.clip_grad_norm == 1.5 and a.skip_nonfinite_grads is True
    d = flags_dict(a)
    assert d["clip_grad_norm"] == 1.5 and d["skip_nonfinite_grads"] is True
    a = parse_flags(["--clip_grad_norm", "2", "--noskip_nonfinite_grads"])
    assert a.clip_grad_norm == 2.0 and a.skip_nonfinite_grads is False


def test_train_passes_options_to_optimizer(tmp_path):
    from transformer_amd.runtime.train_loop import Train

    class Tok:
        vocab_size = 48

    tr = Train(1, False, _model(), Tok(), Tok(), 4, None, None, 2,
               str(tmp_path / "ck"), 16, clip_grad_norm=1.5,
               skip_nonfinite_grads=True)
    assert tr.optimizer.max_grad_norm == 1.5
    assert tr.optimizer.skip_nonfinite is True
    tr = Train(1, False, _model(), Tok(), Tok(), 4, None, None, 2,
               str(tmp_path / "ck"), 16)
    assert not tr.optimizer.guarded


def test_training_loop_logs_guard_scalars(tmp_path):
    """grad_norm / skipped_steps go to the train summary at log_interval."""
    from transformer_amd.runtime.train_loop import Train

    class Tok:
        vocab_size = 48

    tr = Train(1, False, _model(), Tok(), Tok(), 4, str(tmp_path / "log"),
               None, 2, str(tmp_path / "ck"), 16, warmup_steps=10,
               log_interval=2, clip_grad_norm=MAX_NORM)
    seen = []
    real = tr.train_summary_writer.add_scalar
    tr.train_summary_writer.add_scalar = (
        lambda tag, val, step: (seen.append((tag, val, step)),
                                real(tag, val, step)))
    tr.training_loop([_batch()] * 4, [])
    norms = [(v, s) for t, v, s in seen if t == "grad_norm"]
    skips = [(v, s) for t, v, s in seen if t == "skipped_steps"]
    assert [s for _, s in norms] == [2, 4] == [s for _, s in skips]
    assert all(v > MAX_NORM for v, _ in norms)
    assert all(v == 0 for v, _ in skips)


# ---------------------------------------------------------------------------
# gloo world-2: the clip decision is taken on the all-reduced gradient
# ---------------------------------------------------------------------------

def _worker(rank, world, tmpdir, q):
    dist.init_process_group("gloo", init_method=f"file://{tmpdir}/pg",
                            rank=rank, world_size=world)
    try:
        model = _model()
        opt = NoamAdam(model, 16, warmup_steps=10, use_flat=True,
                       max_grad_norm=MAX_NORM, skip_nonfinite=True)
        ddp = BucketedDataParallel(opt.flat, bucket_mb=0.01)
        ddp.broadcast_parameters()
        b = _batch()[0].shape[0]
        _backward(model, opt, rank * b // world, (rank + 1) * b // world)
        ddp.finalize()
        opt.step()
        flat = opt.flat.flat_w.detach().clone()
        gathered = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(gathered, flat)
        if rank == 0:
            q.put((torch.equal(gathered[0], gathered[1]), flat,
                   opt.m.clone(), opt.v.clone(), opt.last_grad_norm(),
                   opt.skipped_steps))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_dp2_clipped_step_matches_dp1(tmp_path):
    model = _model()
    opt = NoamAdam(model, 16, warmup_steps=10, use_flat=True,
                   max_grad_norm=MAX_NORM, skip_nonfinite=True)
    _backward(model, opt)
    g = opt.flat.flat_g.detach().clone()
    opt.step()

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    ps = [ctx.Process(target=_worker, args=(r, 2, str(tmp_path), q))
          for r in range(2)]
    for p in ps:
        p.start()
    same, dp_w, dp_m, dp_v, dp_norm, dp_skipped = q.get()
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    assert same, "ranks diverged after a clipped step"
    assert dp_skipped == 0
    assert dp_norm > 4 * MAX_NORM
    assert float(dp_m.double().norm()) == pytest.approx(
        0.1 * MAX_NORM, rel=1e-5)
    # tolerance of test_dp2_gradients_match_dp1: atol = 1e-5 * max(scale, 1)
    tol = lambda ref: 1e-5 * max(ref.abs().max().item(), 1.0)
    assert dp_norm == pytest.approx(opt.last_grad_norm(), rel=1e-5)
    assert torch.allclose(opt.m, dp_m, atol=tol(opt.m))
    assert torch.allclose(opt.v, dp_v, atol=tol(opt.v))
    # Adam's step lr*m/(sqrt(v)+1e-9) is ill-conditioned where |g| is at
    # the level of the all-reduce's own rounding (e.g. key biases, whose
    # true gradient is zero), so the weights are compared where the
    # gradient is numerically meaningful.
    solid = g.abs() > 1e-3 * g.abs().max()
    assert solid.sum() > 100
    assert torch.allclose(opt.flat.flat_w[solid], dp_w[solid],
                          atol=tol(opt.flat.flat_w))
