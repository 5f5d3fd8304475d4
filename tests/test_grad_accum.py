"""Gradient accumulation — CPU paths (fp32, deterministic): Train.train_step
split into micro-batches, the NoamAdam accumulator bookkeeping on the flat
and the per-parameter layouts, the flag, and gloo world-2.

How "rtol = 1e-5" is applied here.  A split step differs from the unsplit
one only in the ORDER of fp32 additions inside each gradient element, i.e.
by a few 2^-24 of the element's largest summand — not of the element itself,
which may be a cancelled sum.  So every tensor (the loss, each parameter,
each m and v) is compared with |got - ref| <= 1e-5 * (|ref| + max|ref|):
relative to the tensor's own scale, the measure tests/test_ddp_cpu.py uses
for the same kind of reordering.  A dropped chunk, a 1/N or Nx scale error
or a stale accumulator miss it by orders of magnitude.

Adam's eps.  With the default eps = 1e-9 the update lr * g / (|g| + eps) is
a sign function wherever the true gradient is zero (key biases: softmax is
shift-invariant), and there the post-step weight is decided by rounding
noise (tests/test_grad_clip.py masks those elements out for that reason).
The steps below run with eps = 0.1 instead, above the largest gradient
element of this model: the update lr * g / (|g| + eps) is then close to
linear in g, so a reordering error of the gradient reaches the weight
un-amplified (its derivative lr * eps / (|g| + eps)^2 is largest at g = 0,
where it is lr / eps; with eps = 1e-3 that factor measured ~50x the
tolerance's headroom).  Every weight can then be compared, and the update is
also sensitive to the gradient's SCALE, which near-scale-invariant Adam
would hide."""

import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from transformer_amd.config import parse_flags, flags_dict
from transformer_amd.models import Transformer
from transformer_amd.ops import reference as R
from transformer_amd.runtime import NoamAdam
from transformer_amd.runtime.train_loop import Train

EPS = 0.1
RTOL = 1e-5


class Tok:
    vocab_size = 48


def _model():
    torch.manual_seed(0)
    return Transformer(num_layers=1, d_model=16, num_heads=2, dff=32,
                       input_vocab_size=50, target_vocab_size=50, rate=0.0,
                       max_position=32)


def _batch(B=8, seq=6, pad_rows=()):
    torch.manual_seed(99)
    src = torch.randint(1, 50, (B, seq))
    tar = torch.randint(1, 50, (B, seq))
    src[0, 4:] = 0          # ordinary trailing padding
    tar[1, 3:] = 0
    for r in pad_rows:      # whole rows of padding
        src[r] = 0
        tar[r] = 0
    return src, tar


def _train(tmp_path, B, n, use_flat, **kw):
    tr = Train(1, False, _model(), Tok(), Tok(), B, None, None, 2,
               str(tmp_path / f"ck{n}"), 16, warmup_steps=10,
               use_flat=use_flat, grad_accum_steps=n, **kw)
    tr.optimizer.eps = EPS
    return tr


def _state(opt):
    """[(name, tensor)] of master/m/v per parameter, for either layout."""
    out = []
    if opt.flat is not None:
        for i, (p, off) in enumerate(zip(opt.flat.params, opt.flat.offsets)):
            for k in ("master", "m", "v"):
                out.append((f"{k}[{i}]",
                            getattr(opt, k)[off:off + p.numel()]))
        return out
    for i, st in enumerate(opt.state):
        for k in ("master", "m", "v"):
            out.append((f"{k}[{i}]", st[k].reshape(-1)))
    return out


def _weights(model):
    return [(f"w[{i}]", p.detach().reshape(-1))
            for i, p in enumerate(model.parameters())]


def _close(got, ref, name):
    tol = RTOL * (ref.abs() + ref.abs().max())
    bad = (got - ref).abs() > tol
    assert not bad.any(), (name, float((got - ref).abs().max()),
                           float(ref.abs().max()))


def _accs(opt):
    if opt.flat is not None:
        return [opt.acc]
    return [st["acc"] for st in opt.state]


# ---------------------------------------------------------------------------
# split equals unsplit
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def unsplit(tmp_path_factory):
    """N=1 reference steps, computed once per (B, pad, use_flat)."""
    cache = {}

    def get(B, pad, use_flat):
        key = (B, pad, use_flat)
        if key not in cache:
            tr = _train(tmp_path_factory.mktemp("ref"), B, 1, use_flat)
            loss = tr.train_step(_batch(B, pad_rows=pad))
            cache[key] = (float(loss.detach()), tr.train_accuracy.result(),
                          [(n, t.clone()) for n, t in _state(tr.optimizer)],
                          [(n, t.clone()) for n, t in _weights(tr.transformer)])
        return cache[key]
    return get


@pytest.mark.parametrize("use_flat", [True, False])
@pytest.mark.parametrize("pad", [(), (2, 3, 7)])
@pytest.mark.parametrize("B,n", [(8, 2), (8, 4), (6, 4)])
def test_split_equals_unsplit(tmp_path, unsplit, B, n, pad, use_flat):
    """(6, 4) gives chunks 2, 2, 2 and one empty chunk, which is skipped;
    pad rows (2, 3) make one whole N=4 micro-batch of B=8 all-pad."""
    pad = tuple(r for r in pad if r < B)
    ref_loss, ref_acc, ref_state, ref_w = unsplit(B, pad, use_flat)
    tr = _train(tmp_path, B, n, use_flat)
    loss = tr.train_step(_batch(B, pad_rows=pad))
    assert float(loss) == pytest.approx(ref_loss, rel=RTOL)
    assert tr.train_loss.result() == pytest.approx(ref_loss, rel=RTOL)
    assert tr.train_accuracy.result() == pytest.approx(ref_acc, rel=1e-12)
    assert tr.optimizer.step_count == 1
    for (name, got), (_, ref) in zip(_state(tr.optimizer), ref_state):
        _close(got, ref, name)
    for (name, got), (_, ref) in zip(_weights(tr.transformer), ref_w):
        _close(got, ref, name)
    for a in _accs(tr.optimizer):
        assert not a.any()


@pytest.mark.parametrize("use_flat", [True, False])
def test_second_step_starts_from_zero(tmp_path, unsplit, use_flat):
    """Two split steps equal two unsplit steps: nothing of step 1's
    gradient is left in the accumulator for step 2."""
    a = _train(tmp_path, 8, 1, use_flat)
    b = _train(tmp_path, 8, 4, use_flat)
    for tr in (a, b):
        tr.train_step(_batch(8))
        tr.train_step(_batch(8, pad_rows=(5,)))
    assert b.optimizer.step_count == 2
    for (name, got), (_, ref) in zip(_state(b.optimizer),
                                     _state(a.optimizer)):
        _close(got, ref, name)


# ---------------------------------------------------------------------------
# accumulator bookkeeping
# ---------------------------------------------------------------------------

def _micro_backward(model, opt, lo, hi, B=8):
    src, tar = _batch(B)
    logits, _ = model((src[lo:hi], tar[lo:hi, :-1]), training=True)
    loss = R.masked_cross_entropy(logits, tar[lo:hi, 1:], batch_size=B)
    opt.zero_grad()
    loss.backward()


def _opt(model, use_flat, n=2, **kw):
    return NoamAdam(model, 16, warmup_steps=10, use_flat=use_flat, eps=EPS,
                    accum_steps=n, **kw)


def _full_step(model, opt):
    _micro_backward(model, opt, 0, 4)
    opt.accumulate()
    _micro_backward(model, opt, 4, 8)
    opt.accumulate()
    opt.step()


@pytest.mark.parametrize("use_flat", [True, False])
def test_accumulator_is_zero_after_step(use_flat):
    model = _model()
    opt = _opt(model, use_flat, max_grad_norm=0.25)
    _micro_backward(model, opt, 0, 4)
    opt.accumulate()
    assert any(a.any() for a in _accs(opt))
    _micro_backward(model, opt, 4, 8)
    opt.accumulate()
    opt.step()
    for a in _accs(opt):
        assert a.dtype == torch.float32 and not a.any()
    assert opt.step_count == 1 and opt.skipped_steps == 0


@pytest.mark.parametrize("use_flat", [True, False])
def test_nonfinite_micro_gradient_skips_and_zeroes(use_flat):
    model = _model()
    opt = _opt(model, use_flat, skip_nonfinite=True)
    _full_step(model, opt)   # one real step so m/v are not trivially zero
    before = [t.clone() for _, t in _state(opt) + _weights(model)]
    _micro_backward(model, opt, 0, 4)
    if opt.flat is not None:   # inf in ONE micro-gradient
        opt.flat.flat_g[5] = float("inf")
    else:
        next(p for p in opt.params
             if p.grad is not None).grad.view(-1)[5] = float("inf")
    opt.accumulate()
    _micro_backward(model, opt, 4, 8)   # a clean one on top
    opt.accumulate()
    opt.step()
    for a, (_, b) in zip(before, _state(opt) + _weights(model)):
        assert torch.equal(a, b)
    assert opt.skipped_steps == 1 and opt.step_count == 2
    for a in _accs(opt):
        assert not a.any()     # the inf did not survive into the next step
    _full_step(model, opt)
    assert opt.skipped_steps == 1
    assert all(torch.isfinite(t).all() for _, t in _weights(model))
    assert not torch.equal(before[0], _state(opt)[0][1])


@pytest.mark.parametrize("use_flat", [True, False])
def test_discard_accum(use_flat):
    ma, mb = _model(), _model()
    oa, ob = _opt(ma, use_flat), _opt(mb, use_flat)
    _micro_backward(mb, ob, 0, 2)   # an aborted step: other rows
    ob.accumulate()
    assert any(a.any() for a in _accs(ob))
    ob.discard_accum()
    for a in _accs(ob):
        assert not a.any()
    _full_step(ma, oa)
    _full_step(mb, ob)
    for (name, a), (_, b) in zip(_state(oa), _state(ob)):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("use_flat", [True, False])
def test_clip_decision_uses_norm_of_the_sum(use_flat):
    """max_norm sits between the norm of the last micro-gradient and the
    norm of the sum, so clipping engages only if the SUM is judged; then
    ||m|| = (1 - beta1) * max_norm after one step from zero state."""
    def grads(lo, hi):
        model = _model()
        opt = NoamAdam(model, 16, use_flat=use_flat)
        _micro_backward(model, opt, lo, hi)
        return [p.grad.detach().clone() for p in model.parameters()
                if p.grad is not None]
    last = R.global_grad_norm_reference(grads(4, 8))
    full = R.global_grad_norm_reference(grads(0, 8))
    assert last < 0.8 * full
    max_norm = 0.5 * (last + full)

    model = _model()
    opt = _opt(model, use_flat, max_grad_norm=max_norm)
    _full_step(model, opt)
    assert opt.last_grad_norm() == pytest.approx(full, rel=RTOL)
    m = torch.cat([t for n, t in _state(opt) if n.startswith("m[")])
    assert float(m.double().norm()) == pytest.approx(0.1 * max_norm,
                                                     rel=1e-5)


# ---------------------------------------------------------------------------
# flag and N=1 footprint
# ---------------------------------------------------------------------------

def test_flag():
    assert flags_dict(parse_flags([]))["grad_accum_steps"] == 1
    a = parse_flags(["--grad_accum_steps=4"])
    assert a.grad_accum_steps == 4
    assert flags_dict(a)["grad_accum_steps"] == 4
    assert parse_flags(["--grad_accum_steps", "2"]).grad_accum_steps == 2


@pytest.mark.parametrize("use_flat", [True, False])
def test_n1_constructs_no_accumulator(tmp_path, use_flat):
    tr = Train(1, False, _model(), Tok(), Tok(), 4, None, None, 2,
               str(tmp_path / "ck"), 16, use_flat=use_flat)
    opt = tr.optimizer
    assert tr.grad_accum_steps == 1 and opt.accum_steps == 1
    assert opt.acc is None
    if opt.flat is None:
        assert all(set(st) == {"m", "v", "master"} for st in opt.state)
    with pytest.raises(RuntimeError):
        opt.accumulate()
    with pytest.raises(RuntimeError):
        opt.discard_accum()
    with pytest.raises(ValueError):
        NoamAdam(_model(), 16, accum_steps=0)


def test_train_passes_steps_to_optimizer(tmp_path):
    tr = _train(tmp_path, 8, 4, True)
    assert tr.optimizer.accum_steps == 4
    assert tr.optimizer.acc.dtype == torch.float32
    assert tr.optimizer.acc.numel() == tr.optimizer.flat.numel


def test_checkpoint_format_is_unchanged():
    for use_flat in (True, False):
        a = NoamAdam(_model(), 16, use_flat=use_flat).state_dict()
        b = _opt(_model(), use_flat).state_dict()
        assert set(a) == set(b)
        if not use_flat:
            assert all(set(x) == set(y)
                       for x, y in zip(a["state"], b["state"]))


# ---------------------------------------------------------------------------
# gloo world-2: one all-reduce per bucket per OPTIMIZER step
# ---------------------------------------------------------------------------

def _dp_worker(rank, world, tmpdir, q):
    os.environ["TFMX_BUCKET_MB"] = "0.01"   # many buckets
    dist.init_process_group("gloo", init_method=f"file://{tmpdir}/pg",
                            rank=rank, world_size=world)
    try:
        from transformer_amd.runtime.train_loop import DistributedTrain
        tr = DistributedTrain(
            1, False, _model(), Tok(), Tok(), 8, None, None, 2,
            f"{tmpdir}/ckpt", 16, warmup_steps=10, is_rank0=(rank == 0),
            grad_accum_steps=2, clip_grad_norm=1e6)
        tr.optimizer.eps = EPS
        src, tar = _batch(8, pad_rows=(5,))
        lo, hi = rank * 4, rank * 4 + 4
        loss = tr.train_step((src[lo:hi], tar[lo:hi]))
        opt = tr.optimizer
        flat = opt.flat.flat_w.detach().clone()
        gathered = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(gathered, flat)
        losses = [torch.zeros(()) for _ in range(world)]
        dist.all_gather(losses, loss.detach().float().reshape(()))
        if rank == 0:
            q.put((torch.equal(gathered[0], gathered[1]),
                   float(losses[0] + losses[1]),
                   opt.master.clone(), opt.m.clone(), opt.v.clone(),
                   dict(tr.ddp.stats), len(tr.ddp.buckets),
                   bool(opt.acc.any()), opt.last_grad_norm()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_dp2_accumulated_step_matches_single_process(tmp_path):
    ref = _train(tmp_path, 8, 1, True, clip_grad_norm=1e6)
    ref_loss = float(ref.train_step(_batch(8, pad_rows=(5,))).detach())

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    ps = [ctx.Process(target=_dp_worker, args=(r, 2, str(tmp_path), q))
          for r in range(2)]
    for p in ps:
        p.start()
    same, loss, master, m, v, stats, nbuckets, acc_left, norm = q.get()
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    assert same, "ranks diverged after an accumulated step"
    assert nbuckets > 1
    # once per optimizer step, not once per micro backward
    assert stats["accum"] == nbuckets
    assert stats["callback"] == 0 and stats["finalize"] == 0
    assert not acc_left
    assert loss == pytest.approx(ref_loss, rel=RTOL)
    # the guard saw the REDUCED accumulator
    assert norm == pytest.approx(ref.optimizer.last_grad_norm(), rel=RTOL)
    opt = ref.optimizer
    for k, got in (("master", master), ("m", m), ("v", v)):
        for i, (p, off) in enumerate(zip(opt.flat.params, opt.flat.offsets)):
            sl = slice(off, off + p.numel())
            _close(got[sl], getattr(opt, k)[sl], f"{k}[{i}]")
