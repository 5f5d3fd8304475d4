"""Gradient accumulation on the device: grad_accum (grad_accum.hip), the fp32
norm pass (grad_clip.hip), the accumulator-reading Adam kernels (adam.hip),
and their use from NoamAdam / Train eagerly and as the two captured graphs
of CapturedAccumTrainStep.

Inf and NaN below are ordinary data values; nothing here provokes a fault."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from _gpu_bounds import _check_pair
from transformer_amd.ops import reference as R

E = None


def _ext():
    global E
    if E is None:
        from transformer_amd.ops import ext as _e
        E = _e()
    return E


def assert_close(got, ref, tol, name=""):
    """Same measure as tests/test_gpu_kernels.py: max error over max(1, |ref|max)."""
    got = got.float().cpu()
    ref = ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().clamp(min=1.0)
    err = (got - ref).abs().max() / scale
    assert err < tol, f"{name}: rel-max err {err:.6f} (tol {tol})"


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


SIZES = [1, 7, 8, 9, 63, 64, 65, 2047, 10000]
PAD = 8  # sentinel elements kept on either side of every slice


def _accum_wrap_size():
    # just past one full sweep of the capped grid (8 elements per thread per
    # trip, 256 threads per block) plus an odd tail: a second, partial trip
    return _ext().grad_accum_max_blocks() * 256 * 8 + 8 * 37 + 5


def _norm_wrap_size():
    return _ext().grad_norm_max_blocks() * 256 * 8 + 8 * 37 + 5


@pytest.fixture(scope="module")
def big():
    """Shared read-only random buffers: three bf16 gradients and one fp32
    accumulator start value.  Tests slice them and never modify them."""
    torch.manual_seed(0)
    n = max(_accum_wrap_size(), _norm_wrap_size()) + 2 * PAD + 8
    g = [torch.randn(n, device="cuda", dtype=torch.bfloat16) for _ in range(3)]
    a = torch.randn(n, device="cuda")
    return g, a


# ---------------------------------------------------------------------------
# grad_accum: one fp32 add of a bf16 value per element — exact
# ---------------------------------------------------------------------------

def _accum_case(big, n, goff, aoff, rounds=1):
    """acc slice at element offset PAD + aoff of a private copy, gradient
    slices at PAD + goff; returns nothing, asserts exactness and that the
    sentinels around the accumulator slice are untouched."""
    gs, a0 = big
    buf = a0[:n + 2 * PAD + 4].clone()
    before = buf.clone()
    lo = PAD + aoff
    acc = buf[lo:lo + n]
    assert acc.data_ptr() % 16 == (4 * aoff) % 16
    want = before[lo:lo + n].clone()
    for r in range(rounds):
        g = gs[r][PAD + goff:PAD + goff + n]
        assert g.data_ptr() % 16 == (2 * (PAD + goff)) % 16
        _ext().grad_accum(g, acc)
        want = want + g.float()          # sequential fp32 sum
    assert torch.equal(_bits(acc), _bits(want)), (n, goff, aoff)
    assert torch.equal(_bits(buf[:lo]), _bits(before[:lo])), "before slice"
    assert torch.equal(_bits(buf[lo + n:]), _bits(before[lo + n:])), "after"


@pytest.mark.parametrize("n", SIZES)
def test_accum_is_exact(big, n):
    _accum_case(big, n, 0, 0)


def test_accum_grid_stride_wrap(big):
    _accum_case(big, _accum_wrap_size(), 0, 0)
    _accum_case(big, _accum_wrap_size(), 3, 1)


@pytest.mark.parametrize("aoff", [0, 1, 2, 3])
@pytest.mark.parametrize("goff", [0, 1, 2, 3, 4, 5, 6, 7])
def test_accum_misaligned_bases(big, goff, aoff):
    for n in (1, 3, 5, 9, 65, 10000):
        _accum_case(big, n, goff, aoff)


@pytest.mark.parametrize("n,goff,aoff", [(10000, 0, 0), (2047, 5, 3),
                                         (65, 4, 0), (7, 1, 2)])
def test_three_accumulations_equal_sequential_sum(big, n, goff, aoff):
    _accum_case(big, n, goff, aoff, rounds=3)


def test_accum_leaves_gradient_alone(big):
    g = big[0][0][:10000].clone()
    keep = g.clone()
    acc = torch.zeros(10000, device="cuda")
    _ext().grad_accum(g, acc)
    assert torch.equal(_bits(g), _bits(keep))
    assert torch.equal(acc, keep.float())


def test_accum_binding_checks(big):
    e = _ext()
    g = big[0][0][:1000]
    acc = torch.zeros(1000, device="cuda")
    with pytest.raises(RuntimeError):   # length
        e.grad_accum(g, acc[:999])
    with pytest.raises(RuntimeError):   # dtypes
        e.grad_accum(g.float(), acc)
    with pytest.raises(RuntimeError):
        e.grad_accum(g, acc.bfloat16())
    with pytest.raises(RuntimeError):   # contiguity
        e.grad_accum(big[0][0][:2000:2], acc)
    with pytest.raises(RuntimeError):   # device
        e.grad_accum(g.cpu(), acc)
    with pytest.raises(RuntimeError):   # empty
        e.grad_accum(g[:0], acc[:0])


# ---------------------------------------------------------------------------
# grad_norm_clip_f32
# ---------------------------------------------------------------------------

# Tolerance: the derivation of tests/test_gpu_grad_clip.py carries over.  The
# fp32 stage 1 keeps 8 lanes per thread per trip on the same gn_blocks(n)
# grid, so the longest add chain is the same 14 adds; what is new is that the
# square of an fp32 value is itself rounded (a bf16 value's square is exact
# in fp32), one more 2^-24 per term: 15 * 2^-24 = 8.9e-7 relative on the sum
# of squares, half that on the norm, far inside 1e-5.
NORM_RTOL = 1e-5


def _norm_call(a, max_norm=0.0, skip=False, stats=None):
    e = _ext()
    ws = torch.empty(e.grad_norm_blocks(a.numel()), device="cuda")
    if stats is None:
        stats = torch.zeros(4, device="cuda")
    e.grad_norm_clip_f32(a, ws, stats, max_norm, skip)
    return stats


def _ref_norm(a):
    return float(a.double().pow(2).sum().sqrt())


@pytest.mark.parametrize("n", SIZES)
def test_norm_f32_matches_fp64(big, n):
    a = big[1][:n]
    st = _norm_call(a)
    assert st[0].item() == pytest.approx(_ref_norm(a), rel=NORM_RTOL)
    assert st[1].item() == 1.0 and st[2].item() == 0.0 and st[3].item() == 0.0


@pytest.mark.parametrize("off", [1, 2, 3])
def test_norm_f32_misaligned_base(big, off):
    for n in (1, 3, 9, 65, 10000):
        a = big[1][off:off + n]
        assert a.data_ptr() % 16 == 4 * off
        assert _norm_call(a)[0].item() == pytest.approx(_ref_norm(a),
                                                        rel=NORM_RTOL)


@pytest.mark.parametrize("off", [0, 1])
def test_norm_f32_grid_stride_wrap(big, off):
    n = _norm_wrap_size()
    assert _ext().grad_norm_blocks(n) == _ext().grad_norm_max_blocks()
    a = big[1][off:off + n]
    assert _norm_call(a)[0].item() == pytest.approx(_ref_norm(a),
                                                    rel=NORM_RTOL)


@pytest.mark.parametrize("n", [9, 10000, None])
def test_norm_f32_is_deterministic(big, n):
    a = big[1][1:1 + (n or _norm_wrap_size())]
    x, y = _norm_call(a), _norm_call(a)
    assert torch.equal(_bits(x), _bits(y))


def test_norm_f32_exact_on_small_integers():
    # 3-4-12 triple spread over head, body and tail of a misaligned slice
    a = torch.zeros(40, device="cuda")
    a[1], a[20], a[39] = 3.0, 4.0, 12.0
    assert _norm_call(a[1:])[0].item() == 13.0


def test_norm_f32_agrees_with_bf16_kernel_rules(big):
    """Same finalize: scale is bitwise 1 within the bound, and
    max_norm / (norm + 1e-6) beyond it."""
    a = big[1][:10000]
    norm = _norm_call(a)[0].item()
    for max_norm in (0.0, norm, norm * 1.5):
        st = _norm_call(a, max_norm)
        assert st[1:2].view(torch.int32).item() == 0x3F800000, max_norm
    st = _norm_call(a, norm * 0.5)
    assert st[0].item() == norm
    assert st[1].item() == pytest.approx(0.5 * norm / (norm + 1e-6), rel=1e-6)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_norm_f32_nonfinite_sets_flag(big, bad):
    n = 2048 * 3 + 8 * 5 + 3      # several blocks
    stats = torch.zeros(4, device="cuda")
    count = 0
    for base in (0, 3):           # aligned; head of 1 element
        clean = big[1][base:base + n]
        for pos in (0, n - 1, n - 3, 1, n // 2):
            a = clean.clone()
            a[pos] = bad
            _norm_call(a, 1.0, True, stats)
            count += 1
            assert stats[2].item() == 1.0, (base, pos)
            assert stats[3].item() == count, (base, pos)
            _norm_call(clean, 1.0, True, stats)
            assert stats[2].item() == 0.0 and stats[3].item() == count
            _norm_call(a, 1.0, False, stats)   # skipping disabled
            assert stats[2].item() == 0.0 and stats[3].item() == count


def test_norm_f32_binding_checks(big):
    e = _ext()
    st = torch.zeros(4, device="cuda")
    ws = torch.empty(e.grad_norm_blocks(10000), device="cuda")
    a = big[1][:10000]
    with pytest.raises(RuntimeError):  # dtype
        e.grad_norm_clip_f32(a.bfloat16(), ws, st, 0.0, False)
    with pytest.raises(RuntimeError):  # contiguity
        e.grad_norm_clip_f32(big[1][:20000:2], ws, st, 0.0, False)
    with pytest.raises(RuntimeError):  # stats too small
        e.grad_norm_clip_f32(a, ws, st[:3], 0.0, False)
    with pytest.raises(RuntimeError):  # workspace too small
        e.grad_norm_clip_f32(a, ws[:1], st, 0.0, False)


# ---------------------------------------------------------------------------
# Adam from the accumulator
# ---------------------------------------------------------------------------

def _adam_inputs(n):
    torch.manual_seed(0)
    master = torch.randn(n, device="cuda")
    m = torch.randn(n, device="cuda").abs() * 0.01
    v = torch.randn(n, device="cuda").abs() * 0.01
    grad = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    return [master, m, v, grad, master.bfloat16()]


def _acc_inputs(a):
    """The same inputs with the gradient as an fp32 accumulator holding
    exactly the bf16 values."""
    b = [t.clone() for t in a]
    b[3] = a[3].float()
    return b


def _stats(scale, skipped=0.0):
    return torch.tensor([1.0, scale, skipped, 0.0], device="cuda")


HYP = (1e-3, 0.9, 0.98, 1e-9, 3)     # lr, b1, b2, eps, step
DEV = (64.0, 100.0, 0.9, 0.98, 1e-9)  # d_model, warmup, b1, b2, eps


def _dev_state(step0=2):
    return (torch.tensor([step0], dtype=torch.int64, device="cuda"),
            torch.zeros(3, device="cuda"))


def _same_update(a, b):
    for i, name in ((0, "master"), (1, "m"), (2, "v"), (4, "param")):
        assert torch.equal(_bits(a[i]), _bits(b[i])), name
    assert not b[3].any(), "accumulator not zeroed"


@pytest.mark.parametrize("n", [4, 64, 10000])
def test_adam_acc_bitwise_equals_adam_fused(n):
    a = _adam_inputs(n)
    b = _acc_inputs(a)
    _ext().adam_fused(*a, *HYP)
    _ext().adam_fused_acc(*b, *HYP)
    _same_update(a, b)


def test_adam_acc_with_stats_bitwise_equals_adam_fused_clip():
    a = _adam_inputs(10000)
    b = _acc_inputs(a)
    _ext().adam_fused_clip(*a, *HYP, _stats(1.0))
    _ext().adam_fused_acc(*b, *HYP, _stats(1.0))
    _same_update(a, b)
    # and with a real clip scale
    a = _adam_inputs(10000)
    b = _acc_inputs(a)
    _ext().adam_fused_clip(*a, *HYP, _stats(0.37))
    _ext().adam_fused_acc(*b, *HYP, _stats(0.37))
    _same_update(a, b)


@pytest.mark.parametrize("n", [4, 10000])
def test_adam_dev_acc_bitwise_equals_adam_fused_dev(n):
    a = _adam_inputs(n)
    b = _acc_inputs(a)
    sa, ca = _dev_state(2)
    sb, cb = _dev_state(2)
    _ext().adam_fused_dev(*a, sa, ca, *DEV)
    _ext().adam_fused_dev_acc(*b, sb, cb, *DEV)
    _same_update(a, b)
    assert torch.equal(sa, sb) and torch.equal(ca, cb) and sb.item() == 3


def test_adam_dev_acc_with_stats_bitwise_equals_adam_fused_dev_clip():
    a = _adam_inputs(10000)
    b = _acc_inputs(a)
    sa, ca = _dev_state(2)
    sb, cb = _dev_state(2)
    _ext().adam_fused_dev_clip(*a, sa, ca, *DEV, _stats(1.0))
    _ext().adam_fused_dev_acc(*b, sb, cb, *DEV, _stats(1.0))
    _same_update(a, b)
    assert torch.equal(sa, sb) and torch.equal(ca, cb)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("n", [1, 7, 65])
def test_adam_acc_ragged_lengths_match_reference(n, dev):
    """n % 4 != 0 takes the scalar tail, which the bf16 kernels contract
    differently; held against the reference at the tolerance of
    tests/test_gpu_kernels.py::test_adam_fused."""
    master, m, v, grad, param = _adam_inputs(n)
    acc = grad.float()
    mast, mm, vv = master.clone(), m.clone(), v.clone()
    if dev:
        st, cf = _dev_state(2)
        _ext().adam_fused_dev_acc(master, m, v, acc, param, st, cf, *DEV)
        lr = R.noam_lr(3, 64, 100)
        assert st.item() == 3
    else:
        _ext().adam_fused_acc(master, m, v, acc, param, *HYP)
        lr = 1e-3
    R.adam_step_reference(mast, grad.float(), mm, vv, 3, lr, 0.9, 0.98, 1e-9)
    assert_close(master, mast, 1e-4, "master")
    assert_close(m, mm, 1e-4, "m")
    assert_close(v, vv, 1e-4, "v")
    assert_close(param, mast.bfloat16(), 0.01, "param")
    assert not acc.any()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("n", [7, 10000, 10003])
def test_adam_acc_veto_stores_nothing_but_zeroes_accumulator(n, dev):
    a = _acc_inputs(_adam_inputs(n))
    a[3][n // 2] = float("inf")
    before = [t.clone() for t in a]
    # scale is NaN on purpose: a vetoed step must not use it
    if dev:
        st, cf = _dev_state(2)
        _ext().adam_fused_dev_acc(*a, st, cf, *DEV,
                                  _stats(float("nan"), 1.0))
        assert st.item() == 3      # the schedule keeps moving
    else:
        _ext().adam_fused_acc(*a, *HYP, _stats(float("nan"), 1.0))
    for i, name in ((0, "master"), (1, "m"), (2, "v"), (4, "param")):
        assert torch.equal(_bits(a[i]), _bits(before[i])), name
    assert torch.equal(_bits(a[3]), _bits(torch.zeros_like(a[3])))


def test_adam_acc_binding_checks():
    a = _acc_inputs(_adam_inputs(64))
    with pytest.raises(RuntimeError):   # bf16 gradient is the other kernel
        _ext().adam_fused_acc(a[0], a[1], a[2], a[3].bfloat16(), a[4], *HYP)
    with pytest.raises(RuntimeError):   # length
        _ext().adam_fused_acc(a[0], a[1], a[2], a[3][:60], a[4], *HYP)
    with pytest.raises(RuntimeError):   # misaligned accumulator
        buf = torch.zeros(65, device="cuda")
        _ext().adam_fused_acc(a[0], a[1], a[2], buf[1:], a[4], *HYP)
    with pytest.raises(RuntimeError):   # stats too small
        _ext().adam_fused_acc(*a, *HYP, torch.zeros(3, device="cuda"))


# ---------------------------------------------------------------------------
# model level: accumulated fp32 gradient vs the CPU fp32 full-batch gradient
# ---------------------------------------------------------------------------

def _models(**kw):
    """The configuration of tests/test_gpu_model.py::_models."""
    from transformer_amd.models import Transformer
    args = dict(num_layers=2, d_model=256, num_heads=4, dff=512,
                input_vocab_size=500, target_vocab_size=600, rate=0.0,
                max_position=128)
    args.update(kw)
    torch.manual_seed(0)
    cpu = Transformer(**args)
    torch.manual_seed(0)
    gpu = Transformer(**args).to("cuda", torch.bfloat16)
    gpu.load_state_dict({k: v.to("cuda", torch.bfloat16)
                         for k, v in cpu.state_dict().items()})
    return cpu, gpu


@pytest.mark.parametrize("B", [4, 3])   # N=2: chunks 2,2 and 2,1
def test_accumulated_gradient_matches_cpu(B):
    """The accumulated fp32 gradient, read before the apply, meets the bound
    test_model_backward_matches_cpu applies to the unsplit bf16 gradient
    (rel-max < 0.25, scale clamped at 1e-3), against the CPU fp32 model's
    FULL-batch gradient.  Prints error(split) / error(unsplit) per
    parameter; the worst ratio is recorded in
    profiles/grad_accum_parity.md (evidence, not a threshold)."""
    from transformer_amd import ops
    from transformer_amd.runtime import NoamAdam
    cpu, gpu = _models()
    torch.manual_seed(1)
    inp = torch.randint(1, 500, (B, 16))
    tar = torch.randint(1, 600, (B, 16))
    lc, _ = cpu((inp, tar[:, :-1]), training=True)
    R.masked_cross_entropy(lc, tar[:, 1:], B).backward()
    names = [n for n, _ in cpu.named_parameters()]
    cgrads = {n: p.grad.float() for n, p in cpu.named_parameters()}

    opt = NoamAdam(gpu, 256, warmup_steps=50, accum_steps=2)
    gparams = dict(gpu.named_parameters())
    ginp, gtar = inp.cuda(), tar.cuda()

    def backward(lo, hi):
        lg, _ = gpu((ginp[lo:hi], gtar[lo:hi, :-1].contiguous()),
                    training=True)
        loss = ops.masked_cross_entropy(lg, gtar[lo:hi, 1:].contiguous(), B)
        opt.zero_grad()
        loss.backward()

    backward(0, B)
    unsplit = {n: gparams[n]._flat_grad.float().cpu() for n in names}
    rows = -(-B // 2)
    for lo in range(0, B, rows):
        backward(lo, min(lo + rows, B))
        opt.accumulate()
    slices = {id(p): (off, p.numel(), p.shape)
              for p, off in zip(opt.flat.params, opt.flat.offsets)}
    worst = 0.0
    for n in names:
        off, cnt, shape = slices[id(gparams[n])]
        got = opt.acc[off:off + cnt].view(shape).cpu()
        ref = cgrads[n]
        scale = ref.abs().max().clamp(min=1e-3)
        err = float((ref - got).abs().max() / scale)
        err1 = float((ref - unsplit[n]).abs().max() / scale)
        ratio = err / err1 if err1 > 0 else float("nan")
        if ratio == ratio:
            worst = max(worst, ratio)
        print(f"{n}: split {err:.4f} unsplit {err1:.4f} ratio {ratio:.3f}")
        assert err < 0.25, f"{n}: accumulated grad rel err {err:.3f}"
    print(f"B={B} worst error(split)/error(unsplit) = {worst:.3f}")
    opt.discard_accum()


# ---------------------------------------------------------------------------
# training: Train.train_step with N=4, eager and captured
# ---------------------------------------------------------------------------

class Tok:
    vocab_size = 298


@pytest.mark.parametrize("captured", [False, True])
def test_training_with_accumulation(tmp_path, monkeypatch, captured):
    """The criterion of test_train_step_and_determinism (loss after 30 steps
    below 0.7x the first) on one B=8 batch split 4 ways; every counter says
    30 optimizer steps, not 120."""
    from transformer_amd.models import Transformer
    from transformer_amd.runtime.train_loop import Train
    torch.manual_seed(0)
    model = Transformer(num_layers=2, d_model=256, num_heads=4, dff=512,
                        input_vocab_size=300, target_vocab_size=300,
                        rate=0.0, max_position=64).to("cuda", torch.bfloat16)
    tr = Train(1, captured, model, Tok(), Tok(), 8, None, None, 2,
               str(tmp_path / "ck"), 256, warmup_steps=50,
               grad_accum_steps=4)
    opt = tr.optimizer
    calls = {"adam": 0, "accum": 0}
    e = _ext()
    for name, key in (("adam_fused_acc", "adam"),
                      ("adam_fused_dev_acc", "adam"),
                      ("grad_accum", "accum")):
        real = getattr(e, name)

        def counted(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(e, name, counted)
    inp = torch.randint(1, 300, (8, 24), device="cuda")
    tar = torch.randint(1, 300, (8, 24), device="cuda")
    losses = [float(tr.train_step((inp, tar))) for _ in range(30)]
    assert losses[-1] < losses[0] * 0.7, losses[::5]
    assert opt.step_count == 30
    assert not opt.acc.any()
    if captured:
        cap = tr._captured
        step_t, _ = opt.graph_state()
        assert int(step_t.item()) == 30
        # the kernels were recorded, not called, after warmup + capture:
        # (2 warmup + 1 capture) of each graph, whatever the step count
        assert calls == {"adam": 3, "accum": 3}
        assert int(cap.micro_t.item()) == 30 * 4 + 2
    else:
        assert calls == {"adam": 30, "accum": 120}
    assert tr.train_loss.result() == pytest.approx(sum(losses) / 30, rel=1e-6)


# ---------------------------------------------------------------------------
# captured specifics
# ---------------------------------------------------------------------------

def _tiny(rate, seed=7, max_position=32):
    from transformer_amd.models import Transformer
    torch.manual_seed(seed)
    return Transformer(num_layers=2, d_model=64, num_heads=2, dff=128,
                       input_vocab_size=130, target_vocab_size=130,
                       rate=rate, max_position=max_position).cuda().bfloat16()


def _cap(model, B, n, shape, tar_shape=None, **kw):
    from transformer_amd import ops
    from transformer_amd.runtime import NoamAdam
    from transformer_amd.runtime.graph import CapturedAccumTrainStep
    opt = NoamAdam(model, 64, use_flat=True, accum_steps=n, **kw)
    loss_fn = lambda real, pred: ops.masked_cross_entropy(pred, real, B, 0.0)
    cap = CapturedAccumTrainStep(model, opt, loss_fn, shape,
                                 tar_shape or shape, torch.device("cuda"))
    return opt, cap, loss_fn


def test_micro_replays_draw_different_dropout_masks():
    """Two micro replays of the same input inside ONE optimizer step: the
    Adam step tensor has not moved between them, so only the micro graph's
    own counter can have changed the masks."""
    model = _tiny(rate=0.1)
    opt, cap, _ = _cap(model, 4, 2, (2, 16), warmup_steps=100)
    torch.manual_seed(5)
    src = torch.randint(1, 120, (2, 16), device="cuda")
    tar = torch.randint(1, 120, (2, 16), device="cuda")
    step_t, _ = opt.graph_state()
    l1 = cap.micro(src, tar).item()
    t1 = int(cap.micro_t.item())
    l2 = cap.micro(src, tar).item()
    assert int(cap.micro_t.item()) == t1 + 1
    assert int(step_t.item()) == 0 == opt.step_count
    assert math.isfinite(l1) and math.isfinite(l2)
    assert l1 != l2, (l1, l2)
    cap.apply()
    assert int(step_t.item()) == 1 == opt.step_count
    assert not opt.acc.any()


def test_first_micro_replay_after_apply_sees_fresh_transposes():
    """warmup_steps=1: the first update moves every weight by about the
    learning rate (0.125), so a dX GEMM contracting against W^T of the OLD
    weights is off by O(1).  2048 rows per micro-batch put every d_model- and
    dff-wide dX on the cached-W^T backend.  After one captured apply, one
    micro replay must leave in the accumulator what an eager backward of the
    same batch on the same model computes: same kernels, same shapes, only
    atomic order differs, hence the pair bound."""
    model = _tiny(rate=0.0, max_position=512)
    B, S = 8, 256                     # 2048 encoder and decoder rows
    opt, cap, loss_fn = _cap(model, 2 * B, 2, (B, S), (B, S + 1),
                             warmup_steps=1)
    torch.manual_seed(5)
    src = torch.randint(1, 120, (B, S), device="cuda")
    tar = torch.randint(1, 120, (B, S + 1), device="cuda")
    w0 = opt.flat.flat_w.clone()
    cap.micro(src, tar)
    cap.micro(src, tar)
    cap.apply()                       # weights move in-graph
    assert (opt.flat.flat_w.float() - w0.float()).abs().max() > 0.05
    cap.micro(src, tar)               # first micro replay after the apply
    torch.cuda.synchronize()
    got = opt.acc.clone()

    logits, _ = model((src, tar[:, :-1].contiguous()), training=True)
    loss = loss_fn(tar[:, 1:].contiguous(), logits)
    opt.zero_grad()
    loss.backward()
    _check_pair(got, opt.flat.flat_g, "accumulator vs eager backward")
    assert got.abs().max() > 0
    opt.discard_accum()


def test_accum_recapture_is_state_neutral():
    model = _tiny(rate=0.1, seed=11, max_position=64)
    opt, cap, loss_fn = _cap(model, 4, 2, (2, 8), warmup_steps=100,
                             max_grad_norm=1.0, skip_nonfinite=True)
    src = torch.randint(1, 120, (4, 8), device="cuda")
    tar = torch.randint(1, 120, (4, 8), device="cuda")
    for _ in range(3):
        loss, c, t = cap(src, tar)
        assert math.isfinite(loss) and 0 <= c <= t == 4 * 7
    snap = (opt.master.clone(), opt.m.clone(), opt.v.clone(),
            opt.flat.flat_w.clone(), opt.step_count, opt.skipped_steps)
    assert snap[4] == 3 and not opt.acc.any()
    from transformer_amd.runtime.graph import CapturedAccumTrainStep
    cap2 = CapturedAccumTrainStep(model, opt, loss_fn, (2, 16), (2, 16),
                                  torch.device("cuda"))
    torch.cuda.synchronize()
    assert torch.equal(opt.master, snap[0]), "master moved in recapture"
    assert torch.equal(opt.m, snap[1]), "m moved in recapture"
    assert torch.equal(opt.v, snap[2]), "v moved in recapture"
    assert torch.equal(opt.flat.flat_w, snap[3]), "weights moved"
    assert not opt.acc.any(), "accumulator not zero after recapture"
    assert opt.step_count == snap[4] and opt.skipped_steps == snap[5]
    step_t, _ = opt.graph_state()
    assert int(step_t.item()) == opt.step_count
    assert not cap2.sums.any()
    assert cap2.fits(src, tar) and not cap2.fits(src.repeat(2, 1),
                                                 tar.repeat(2, 1))


def test_captured_step_is_vetoed_and_accumulator_cleared():
    """An inf in the accumulator: the apply graph skips the update on the
    device and still leaves the accumulator zero for the next step."""
    model = _tiny(rate=0.0)
    opt, cap, _ = _cap(model, 4, 2, (2, 16), warmup_steps=100,
                       skip_nonfinite=True)
    src = torch.randint(1, 120, (4, 16), device="cuda")
    tar = torch.randint(1, 120, (4, 16), device="cuda")
    cap(src, tar)
    before = [t.clone() for t in (opt.master, opt.m, opt.v, opt.flat.flat_w)]
    cap.micro(src[:2], tar[:2])
    opt.acc[opt.flat.offsets[1] + 3] = float("inf")
    cap.micro(src[2:], tar[2:])
    cap.apply()
    cap.sums.zero_()
    for t, ref in zip((opt.master, opt.m, opt.v, opt.flat.flat_w), before):
        assert torch.equal(t, ref)
    assert opt.skipped_steps == 1 and opt.step_count == 2
    assert torch.equal(_bits(opt.acc), _bits(torch.zeros_like(opt.acc)))
    cap(src, tar)
    assert opt.skipped_steps == 1 and not torch.equal(opt.m, before[1])
