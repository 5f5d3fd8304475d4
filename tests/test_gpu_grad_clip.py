"""Device-side gradient guard: the two-stage global-norm reduction
(grad_clip.hip), the clipped/skippable Adam kernels (adam.hip) and their use
from NoamAdam eagerly and inside a captured hipGraph.

Inf and NaN below are ordinary data values; nothing here provokes a fault."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

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


def _norm_call(g, max_norm=0.0, skip=False, stats=None):
    e = _ext()
    ws = torch.empty(e.grad_norm_blocks(g.numel()), device="cuda")
    if stats is None:
        stats = torch.zeros(4, device="cuda")
    e.grad_norm_clip(g, ws, stats, max_norm, skip)
    return stats


def _ref_norm(g):
    return float(g.double().pow(2).sum().sqrt())


def _wrap_size():
    # just past one full sweep of the capped grid, plus an odd tail, so the
    # grid-stride loop takes a second (partial) trip
    return _ext().grad_norm_max_blocks() * 256 * 8 + 8 * 37 + 5


# ---------------------------------------------------------------------------
# norm kernel
# ---------------------------------------------------------------------------

# Tolerance 1e-5 relative on the norm.  All summands are >= 0, so the fp32
# error of the sum is bounded by (longest add chain) * 2^-24 relative, and
# the norm's by half that.  Longest chain here: per-lane accumulator
# (<= 2 grid-stride trips + 1 head/tail add) + 3 (8 lanes) + 6 (wave) +
# 2 (4 waves) = 14 adds; stage 2 sums the partials in double.  14 * 2^-24
# = 8.3e-7, far inside 1e-5.
NORM_RTOL = 1e-5

SIZES = [1, 7, 8, 9, 63, 64, 65, 2047, 10000]


@pytest.fixture(scope="module")
def big():
    """One shared random bf16 buffer; tests slice it and never modify it."""
    torch.manual_seed(0)
    return torch.randn(_wrap_size() + 8, device="cuda", dtype=torch.bfloat16)


@pytest.mark.parametrize("n", SIZES)
def test_norm_matches_fp64(big, n):
    g = big[:n]
    st = _norm_call(g)
    assert st[0].item() == pytest.approx(_ref_norm(g), rel=NORM_RTOL)
    assert st[1].item() == 1.0 and st[2].item() == 0.0 and st[3].item() == 0.0


def test_norm_grid_stride_wrap(big):
    n = _wrap_size()
    assert _ext().grad_norm_blocks(n) == _ext().grad_norm_max_blocks()
    assert _ext().grad_norm_blocks(n * 4) == _ext().grad_norm_max_blocks()
    g = big[:n]
    assert _norm_call(g)[0].item() == pytest.approx(_ref_norm(g),
                                                    rel=NORM_RTOL)


@pytest.mark.parametrize("off", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("n", [1, 5, 9, 65, 10000])
def test_norm_misaligned_base(big, off, n):
    g = big[off:off + n]
    assert g.data_ptr() % 16 == 2 * off
    assert _norm_call(g)[0].item() == pytest.approx(_ref_norm(g),
                                                    rel=NORM_RTOL)


def test_norm_misaligned_wrap(big):
    g = big[1:1 + _wrap_size()]
    assert _norm_call(g)[0].item() == pytest.approx(_ref_norm(g),
                                                    rel=NORM_RTOL)


@pytest.mark.parametrize("n", [9, 10000, None])
def test_norm_is_deterministic(big, n):
    g = big[1:1 + (n or _wrap_size())]
    a, b = _norm_call(g), _norm_call(g)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_norm_exact_on_small_integers():
    # 3-4-12 triple spread over head, body and tail of a misaligned slice
    g = torch.zeros(40, device="cuda", dtype=torch.bfloat16)
    g[1], g[20], g[39] = 3.0, 4.0, 12.0
    assert _norm_call(g[1:])[0].item() == 13.0


def test_binding_checks(big):
    e = _ext()
    st = torch.zeros(4, device="cuda")
    ws = torch.empty(e.grad_norm_blocks(10000), device="cuda")
    with pytest.raises(RuntimeError):  # dtype
        e.grad_norm_clip(big[:10000].float(), ws, st, 0.0, False)
    with pytest.raises(RuntimeError):  # contiguity
        e.grad_norm_clip(big[:20000:2], ws, st, 0.0, False)
    with pytest.raises(RuntimeError):  # stats too small
        e.grad_norm_clip(big[:10000], ws, st[:3], 0.0, False)
    with pytest.raises(RuntimeError):  # workspace too small
        e.grad_norm_clip(big[:10000], ws[:1], st, 0.0, False)
    with pytest.raises(RuntimeError):  # device
        e.grad_norm_clip(big[:10000].cpu(), ws, st, 0.0, False)


# ---------------------------------------------------------------------------
# scale rule
# ---------------------------------------------------------------------------

def test_scale_is_bitwise_one_within_bound(big):
    g = big[:10000]
    norm = _norm_call(g)[0].item()
    for max_norm in (0.0, -1.0, norm, norm * 1.5, 1e30):
        st = _norm_call(g, max_norm)
        assert st[1:2].view(torch.int32).item() == 0x3F800000, max_norm


@pytest.mark.parametrize("frac", [0.999, 0.5, 1e-3])
def test_scale_when_clipping(big, frac):
    g = big[:10000]
    norm = _norm_call(g)[0].item()
    max_norm = norm * frac
    st = _norm_call(g, max_norm)
    assert st[0].item() == norm
    assert st[1].item() == pytest.approx(max_norm / (norm + 1e-6), rel=1e-6)
    assert st[1].item() < 1.0


# ---------------------------------------------------------------------------
# non-finite detection
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_sets_flag_and_counts(big, bad):
    n = 2048 * 3 + 8 * 5 + 3      # several blocks
    stats = torch.zeros(4, device="cuda")
    count = 0
    # aligned base: no head, tail of n % 8 = 3 (n-3 is its first element);
    # base 3: head of 5 (element 0 is in it), tail of (n - 5) % 8 = 6
    for base in (0, 3):
        clean = big[base:base + n]
        for pos in (0, n - 1, n - 3, 1):
            g = clean.clone()
            g[pos] = bad
            _norm_call(g, 1.0, True, stats)
            count += 1
            assert stats[2].item() == 1.0, (base, pos)
            assert stats[3].item() == count, (base, pos)
            # a finite gradient clears the flag and leaves the total alone
            _norm_call(clean, 1.0, True, stats)
            assert stats[2].item() == 0.0 and stats[3].item() == count
            # skipping disabled: never flagged
            _norm_call(g, 1.0, False, stats)
            assert stats[2].item() == 0.0 and stats[3].item() == count


def test_fp32_overflow_is_nonfinite():
    """Documented rule: a finite gradient whose fp32 sum of squares
    overflows (norm > ~1.8e19) counts as non-finite."""
    g = torch.zeros(100, device="cuda", dtype=torch.bfloat16)
    g[50] = 1.5e19                 # 2.25e38 < FLT_MAX: still finite
    st = _norm_call(g, 1.0, True)
    assert st[2].item() == 0.0
    assert st[0].item() == pytest.approx(float(g[50]), rel=NORM_RTOL)
    g[50] = 3e19                   # 9e38 > FLT_MAX
    assert _norm_call(g, 1.0, True)[2].item() == 1.0


# ---------------------------------------------------------------------------
# clipped Adam
# ---------------------------------------------------------------------------

def _adam_inputs(n):
    torch.manual_seed(0)
    master = torch.randn(n, device="cuda")
    m = torch.randn(n, device="cuda").abs() * 0.01
    v = torch.randn(n, device="cuda").abs() * 0.01
    grad = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    return [master, m, v, grad, master.bfloat16()]


def _stats(scale, skipped=0.0):
    return torch.tensor([1.0, scale, skipped, 0.0], device="cuda")


HYP = (1e-3, 0.9, 0.98, 1e-9, 3)     # lr, b1, b2, eps, step
DEV = (64.0, 100.0, 0.9, 0.98, 1e-9)  # d_model, warmup, b1, b2, eps


def _dev_state(step0=2):
    return (torch.tensor([step0], dtype=torch.int64, device="cuda"),
            torch.zeros(3, device="cuda"))


@pytest.mark.parametrize("scale", [1.0, 0.37, 1e-3])
def test_adam_clip_matches_reference(scale):
    master, m, v, grad, param = _adam_inputs(10003)  # ragged tail
    mast, mm, vv = master.clone(), m.clone(), v.clone()
    _ext().adam_fused_clip(master, m, v, grad, param, *HYP, _stats(scale))
    R.adam_step_reference(mast, grad.float() * scale, mm, vv, 3, 1e-3, 0.9,
                          0.98, 1e-9)
    assert_close(master, mast, 1e-4, "master")
    assert_close(m, mm, 1e-4, "m")
    assert_close(v, vv, 1e-4, "v")
    assert_close(param, mast.bfloat16(), 0.01, "param")


def test_adam_clip_scale_one_equals_adam_fused():
    """n is a multiple of 4 — as every flat parameter buffer is (64-element
    alignment) — so all elements take the kernels' vector path; the clipped
    body spells out the fused multiply-adds that path uses.  (The scalar
    tail of the unclipped kernel is contracted differently by the compiler
    and is covered against the reference above instead.)"""
    a = _adam_inputs(10000)
    b = [t.clone() for t in a]
    _ext().adam_fused(*a, *HYP)
    _ext().adam_fused_clip(*b, *HYP, _stats(1.0))
    for x, y, name in zip(a, b, ("master", "m", "v", "grad", "param")):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("bad", [None, float("inf"), float("nan")])
def test_adam_clip_skip_stores_nothing(bad):
    a = _adam_inputs(10003)
    if bad is not None:
        a[3][17] = bad
    before = [t.clone() for t in a]
    # scale is NaN here on purpose: a skipped step must not even read it
    _ext().adam_fused_clip(*a, *HYP, _stats(float("nan"), 1.0))
    for x, y in zip(a, before):
        assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16
                                  else torch.int32),
                           y.view(torch.int16 if y.dtype == torch.bfloat16
                                  else torch.int32))


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_adam_dev_clip_matches_reference(scale):
    master, m, v, grad, param = _adam_inputs(10003)
    mast, mm, vv = master.clone(), m.clone(), v.clone()
    st, cf = _dev_state(2)
    _ext().adam_fused_dev_clip(master, m, v, grad, param, st, cf, *DEV,
                               _stats(scale))
    assert st.item() == 3
    lr = R.noam_lr(3, 64, 100)
    assert cf[0].item() == pytest.approx(lr, rel=1e-5)
    R.adam_step_reference(mast, grad.float() * scale, mm, vv, 3, lr, 0.9,
                          0.98, 1e-9)
    assert_close(master, mast, 1e-4, "master")
    assert_close(m, mm, 1e-4, "m")
    assert_close(v, vv, 1e-4, "v")
    assert_close(param, mast.bfloat16(), 0.01, "param")


def test_adam_dev_clip_scale_one_equals_adam_fused_dev():
    a = _adam_inputs(10000)
    b = [t.clone() for t in a]
    sa, ca = _dev_state(2)
    sb, cb = _dev_state(2)
    _ext().adam_fused_dev(*a, sa, ca, *DEV)
    _ext().adam_fused_dev_clip(*b, sb, cb, *DEV, _stats(1.0))
    for x, y, name in zip(a, b, ("master", "m", "v", "grad", "param")):
        assert torch.equal(x, y), name
    assert torch.equal(sa, sb) and torch.equal(ca, cb)


def test_adam_dev_clip_skip_advances_step_only():
    a = _adam_inputs(10003)
    a[3][0] = float("inf")
    before = [t.clone() for t in a]
    st, cf = _dev_state(2)
    _ext().adam_fused_dev_clip(*a, st, cf, *DEV, _stats(1.0, 1.0))
    for x, y in zip(a, before):
        assert torch.equal(x.float().nan_to_num(), y.float().nan_to_num())
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    assert st.item() == 3          # the schedule keeps moving
    assert cf[0].item() == pytest.approx(R.noam_lr(3, 64, 100), rel=1e-5)


# ---------------------------------------------------------------------------
# NoamAdam on the device: eager and captured
# ---------------------------------------------------------------------------

def _tiny_model(rate=0.0, seed=7):
    from transformer_amd.models import Transformer
    torch.manual_seed(seed)
    return Transformer(num_layers=2, d_model=64, num_heads=2, dff=128,
                       input_vocab_size=130, target_vocab_size=130,
                       rate=rate, max_position=32).cuda().bfloat16()


def _fill_param_grads(opt, poison=None):
    """Random gradient in the parameter regions only — the alignment
    padding of flat_g stays zero, as in training."""
    torch.manual_seed(1)
    opt.flat.flat_g.zero_()
    for p, off in zip(opt.flat.params, opt.flat.offsets):
        opt.flat.flat_g[off:off + p.numel()].normal_()
    if poison is not None:
        opt.flat.flat_g[opt.flat.offsets[1] + 3] = poison


def test_defaults_allocate_no_guard_state():
    from transformer_amd.runtime import NoamAdam
    opt = NoamAdam(_tiny_model(), 64, use_flat=True)
    assert not opt.guarded and opt._gn_stats is None
    assert opt.skipped_steps == 0


def test_step_captured_alone_in_graph():
    from transformer_amd.runtime import NoamAdam
    model = _tiny_model()
    opt = NoamAdam(model, 64, warmup_steps=100, use_flat=True,
                   max_grad_norm=1.0, skip_nonfinite=True)
    step_t, _ = opt.graph_state()
    _fill_param_grads(opt)
    ref_norm = _ref_norm(opt.flat.flat_g)

    # one eager call on a side stream before capturing, then undo it
    snap = [t.clone() for t in (opt.master, opt.m, opt.v, opt.flat.flat_w)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.step_captured()
    torch.cuda.current_stream().wait_stream(s)
    for dst, src in zip((opt.master, opt.m, opt.v, opt.flat.flat_w), snap):
        dst.copy_(src)
    step_t.zero_()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step_captured()   # norm pass -> coefs -> clipped Adam: a chain

    graph.replay()            # 1: finite gradient, update applied
    torch.cuda.synchronize()
    assert opt.last_grad_norm() == pytest.approx(ref_norm, rel=NORM_RTOL)
    assert opt.last_grad_norm() > 1.0
    assert float(opt.m.double().norm()) == pytest.approx(0.1, rel=1e-4)
    assert not torch.equal(opt.master, snap[0])
    assert opt.skipped_steps == 0 and step_t.item() == 1

    after1 = [t.clone() for t in (opt.master, opt.m, opt.v, opt.flat.flat_w)]
    _fill_param_grads(opt, poison=float("inf"))
    graph.replay()            # 2: vetoed on the device
    torch.cuda.synchronize()
    for t, ref in zip((opt.master, opt.m, opt.v, opt.flat.flat_w), after1):
        assert torch.equal(t, ref)
    assert opt.skipped_steps == 1
    assert step_t.item() == 2  # schedule in lock-step with the host count

    _fill_param_grads(opt)
    graph.replay()            # 3: back to normal
    torch.cuda.synchronize()
    assert opt.skipped_steps == 1 and step_t.item() == 3
    assert not torch.equal(opt.m, after1[1])
    assert torch.isfinite(opt.master).all()


def _src_tar(B=4, S=16):
    torch.manual_seed(5)
    return (torch.randint(1, 120, (B, S), device="cuda"),
            torch.randint(1, 120, (B, S), device="cuda"))


def test_captured_train_step_clips():
    from transformer_amd import ops
    from transformer_amd.runtime import NoamAdam
    from transformer_amd.runtime.graph import CapturedTrainStep

    model = _tiny_model(rate=0.0)
    opt = NoamAdam(model, 64, warmup_steps=100, use_flat=True,
                   max_grad_norm=1.0)
    B, S = 4, 16
    cap = CapturedTrainStep(model, opt, lambda real, pred:
                            ops.masked_cross_entropy(pred, real, B, 0.0),
                            (B, S), (B, S), torch.device("cuda"))
    src, tar = _src_tar(B, S)
    loss = cap(src, tar).item()
    assert math.isfinite(loss)
    norm = opt.last_grad_norm()
    assert norm > 1.0
    assert norm == pytest.approx(_ref_norm(opt.flat.flat_g), rel=NORM_RTOL)
    # ||m|| = 0.1 * scale * ||g||: per-element fp32 rounding plus the 1e-5
    # bound on the norm
    assert float(opt.m.double().norm()) == pytest.approx(0.1 * 1.0, rel=1e-4)
    assert opt.skipped_steps == 0 and opt.step_count == 1


def test_eager_train_step_clips(tmp_path):
    from transformer_amd.runtime.train_loop import Train

    class Tok:
        vocab_size = 128

    tr = Train(1, False, _tiny_model(rate=0.0), Tok(), Tok(), 4, None, None,
               2, str(tmp_path / "ck"), 64, warmup_steps=100,
               clip_grad_norm=1.0, skip_nonfinite_grads=True)
    tr.train_step(_src_tar())
    opt = tr.optimizer
    assert opt.last_grad_norm() > 1.0
    assert float(opt.m.double().norm()) == pytest.approx(0.1 * 1.0, rel=1e-4)
    assert opt.skipped_steps == 0 and opt.step_count == 1
