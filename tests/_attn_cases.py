"""Cases, fp64 reference, element-wise limits and an fp32 emulation of the
training attention kernels (ops/csrc/attention.hip: attn_fwd, attn_bwd modes
0/1/2 and the _seg variants).

Shared by tests/test_gpu_attn_elementwise.py (the HIP kernels) and
tests/test_attn_bounds.py (the emulation, on the CPU).  Plain torch; the
extension is not imported.  Inputs are bf16 tensors made on the CPU from a
seeded generator; the reference and every limit are fp64 on those values.

Reference: visibility vis[i,j] = live_key[j] and (not causal or j <= i), or
the id rule of reference.create_segment_mask; hidden logits are -inf
(selection, not the additive -1e9).  Query rows with no visible key are
EXCLUDED from the O / LSE / dQ comparison (the plain kernels' additive rule
gives them a uniform average by design); their dO is zero in the case itself,
so they add nothing to dK / dV.

Limits.  u = 2^-8 (f2bfbits is round-to-nearest-even), the fp32 summation
order costs 1e-5 * sum|terms|.  With A = scale * |q||k|^T:

  d32   = 2^-24 * (dh + 8) * A + 2^-20   fp32 score accumulation + fast exp
  delta = u + d32                        P is rounded to bf16 before PV and l
  lim_O = u|O| + sum_j P delta |v_j - O| / (1 - dmax) + 1e-5 * P|v|
            from O^ - O = sum_j P_j e_j (v_j - O) / (1 + sum_j P_j e_j): the
            numerator and l use the same rounded P
  lim_L = sum_j P delta / (1 - dmax) + 1e-5 * (1 + |lse|)
  lim_dV = u|dV| + 1.01 * (P (delta + lim_L))^T |dO| + 1e-5 * P^T |dO|
            the backward's p = exp(s - lse_kernel), rounded to bf16
  rho   = d32 + lim_L                    p is not rounded on the dS path
  errD  = sum_c |dO| lim_O + 1e-5 * sum_c |dO O|
  errS  = scale * P * (rho |dP - D| + errD + 1e-5 |dO||v|^T) + u|dS|
  lim_dQ = u|dQ| + 1.01 * errS |k| + 1e-5 * |dS||k|
  lim_dK = u|dK| + 1.01 * errS^T |q| + 1e-5 * |dS|^T |q|

1.01 covers the second-order products of terms each at most 2^-7.  P is 0 at
hidden keys, so their dK / dV limits are 0: exact zeros are demanded."""

import functools
import math
import zlib

import torch

from _gpu_bounds import U, _check_lim

OUTPUTS = ("O", "LSE", "dQ", "dK", "dV")

# segment layouts of tests/test_gpu_seq_packing.py: a length-1 segment, one
# holding a whole 64-key tile, boundaries off every multiple of 16; a full
# row; an all-pad row.  The rows after the first three keep the id-0 rows of
# a case under 1/8 and put boundaries on the tile edges.
SELF_ROWS, SELF_S = [[3, 1, 150, 30], [200], []], 200
SELF_MORE = [[200], [100, 100], [64, 64, 72], [1, 199], [63, 65, 72],
             [128, 72]]
CROSS_T, CROSS_S, SQ, SK = ([[5, 40, 20], [70], []],
                            [[60, 7, 70], [150], []], 70, 150)
CROSS_T_MORE = [[70], [35, 35], [1, 69], [16, 16, 38], [64, 6], [70]]
CROSS_S_MORE = [[150], [64, 86], [149, 1], [32, 32, 86], [128, 22], [1]]
LONG_ROWS, LONG_S = [[300, 7, 500, 64, 129, 70]], 1100


def seg_ids(rows, S):
    """rows: per batch row a list of segment lengths -> (B,S) int32 ids."""
    out = torch.zeros(len(rows), S, dtype=torch.int32)
    for b, lens in enumerate(rows):
        o = 0
        for n_seg, n in enumerate(lens, start=1):
            out[b, o:o + n] = n_seg
            o += n
        assert o <= S
    return out


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

def _spec(name, Sq, Sk=None, dh=64, causal=False, B=2, H=3, pad=None,
          q_seg=None, kv_seg=None, sharp=None, layout="plain", trv=1,
          excluded=False, bwd=True):
    """pad: list of (batch row, first, last+1) key ranges that are padding.
    layout: plain | qkv (mode 1) | kv (mode 2) | cache (forward only, k/v
    slices of a longer buffer).  excluded: the case names rows without a
    visible key."""
    return dict(name=name, Sq=Sq, Sk=Sq if Sk is None else Sk, dh=dh,
                causal=causal, B=B, H=H, pad=pad or [], q_seg=q_seg,
                kv_seg=kv_seg, sharp=sharp, layout=layout, trv=trv,
                excluded=excluded, bwd=bwd)


def _all_specs():
    out = []
    # self attention: every side of the 16-row fragment and the 64-key tile
    for S in (1, 15, 16, 17, 33, 63, 64, 65, 129):
        for dh in ((32, 64, 128) if S in (17, 65, 129) else (64,)):
            for causal in (False, True):
                for npad in (0, 1, 5):
                    if npad >= S:
                        continue
                    pad = [(0, S - npad, S)] if npad else None
                    out.append(_spec(
                        f"self-S{S}-dh{dh}-c{int(causal)}-pad{npad}", S,
                        dh=dh, causal=causal, pad=pad))
    for Sq, Sk in ((1, 65), (37, 129), (65, 1), (70, 33)):
        for dh in (64, 128):
            out.append(_spec(f"cross-{Sq}x{Sk}-dh{dh}", Sq, Sk, dh=dh))
    # pad patterns at S = 129
    out.append(_spec("pad-hole", 129, pad=[(0, 70, 76), (1, 70, 76)]))
    out.append(_spec("pad-middle-tile", 129, pad=[(0, 64, 128), (1, 64, 128)]))
    out.append(_spec("pad-leading-tile", 129, pad=[(0, 0, 64), (1, 0, 64)]))
    out.append(_spec("pad-leading-tile-causal", 520, causal=True, B=1,
                     pad=[(0, 0, 64)], excluded=True))
    # sharp logits
    out.append(_spec("sharp-q3-S100", 100, causal=True, sharp="q3"))
    out.append(_spec("sharp-spike-S512", 512, B=1, H=1, sharp="spike"))
    # the plain 64-row backward tiles (Sq, Sk >= 1024) and their edge
    out.append(_spec("qt64-S1030-causal-pad6", 1030, causal=True, B=1, H=1,
                     pad=[(0, 1024, 1030)]))
    out.append(_spec("qt64-1024x1090", 1024, 1090, B=1, H=1))
    out.append(_spec("qt32-edge-1024x1023", 1024, 1023, B=1, H=1))
    # layouts
    out.append(_spec("mode1-qkv-S65", 65, causal=True, pad=[(0, 60, 65)],
                     layout="qkv"))
    out.append(_spec("mode2-kv-37x129", 37, 129, pad=[(0, 124, 129)],
                     layout="kv"))
    out.append(_spec("cache-slice-37x129", 37, 129, pad=[(0, 124, 129)],
                     layout="cache", bwd=False))
    # segments
    seg = seg_ids(SELF_ROWS + SELF_MORE, SELF_S)
    for dh in (64, 128):
        for causal in (False, True):
            out.append(_spec(f"seg-self-dh{dh}-c{int(causal)}", SELF_S, dh=dh,
                             causal=causal, B=seg.shape[0], H=2, q_seg=seg,
                             kv_seg=seg, excluded=True))
    qs = seg_ids(CROSS_T + CROSS_T_MORE, SQ)
    ks = seg_ids(CROSS_S + CROSS_S_MORE, SK)
    for dh in (64, 128):
        out.append(_spec(f"seg-cross-dh{dh}", SQ, SK, dh=dh, B=qs.shape[0],
                         H=2, q_seg=qs, kv_seg=ks, excluded=True))
    seg = seg_ids(LONG_ROWS, LONG_S)
    out.append(_spec("seg-qt64-S1100-causal", LONG_S, causal=True, B=1, H=1,
                     q_seg=seg, kv_seg=seg, excluded=True))
    out.append(_spec("seg-mode1-qkv", SELF_S, causal=True, H=2,
                     B=3, q_seg=seg_ids(SELF_MORE[:3], SELF_S),
                     kv_seg=seg_ids(SELF_MORE[:3], SELF_S), layout="qkv"))
    return out


_SPECS = {s["name"]: s for s in _all_specs()}
CASES = list(_SPECS)
# forward-only runs with both values of trv: a ragged tile, dh 128 causal,
# Sq != Sk, dh 32
TRV_CASES = ["self-S65-dh64-c0-pad1", "self-S129-dh128-c1-pad0",
             "cross-37x129-dh64", "self-S17-dh32-c0-pad5"]
IDENTITY_CASES = ["self-S17-dh64-c1-pad5", "cross-37x129-dh64",
                  "seg-cross-dh64"]


def visibility(c):
    """(B,Sq,Sk) bool."""
    B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
    if c["q_seg"] is not None:
        qs, ks = c["q_seg"].long(), c["kv_seg"].long()
        vis = (qs[:, :, None] == ks[:, None, :]) & (qs[:, :, None] != 0)
    else:
        vis = (c["kv_pad"] == 0)[:, None, :].expand(B, Sq, Sk).clone()
    if c["causal"]:
        i = torch.arange(Sq)[:, None]
        j = torch.arange(Sk)[None, :]
        vis = vis & (j <= i)
    return vis


@functools.lru_cache(maxsize=None)
def attn_case(name):
    s = dict(_SPECS[name])
    B, H, Sq, Sk, dh = s["B"], s["H"], s["Sq"], s["Sk"], s["dh"]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    q, k, v, do = rn(B, Sq, H, dh), rn(B, Sk, H, dh), rn(B, Sk, H, dh), \
        rn(B, Sq, H, dh)
    if s["sharp"] == "q3":
        q = q * 3
    elif s["sharp"] == "spike":     # test_attn_defer_max_spike_forces_rescale
        q, k = q * 0.5, k * 0.5
        k[:, 350] = 4.0
        q[..., :8] = 2.0
    kv_pad = torch.zeros(B, Sk, dtype=torch.uint8)
    for b, lo, hi in s["pad"]:
        kv_pad[b, lo:hi] = 1
    s.update(kv_pad=kv_pad, scale=1.0 / math.sqrt(dh))
    vis = visibility(s)
    inc = vis.any(-1)                               # (B,Sq)
    n_exc = int((~inc).sum())
    assert 8 * n_exc <= B * Sq, (name, n_exc)
    assert s["excluded"] or n_exc == 0, (name, n_exc)
    do = do * inc[:, :, None, None]
    s.update(q=q.bfloat16(), k=k.bfloat16(), v=v.bfloat16(),
             do=do.bfloat16(), vis=vis, inc=inc)
    return s


# ---------------------------------------------------------------------------
# fp64 reference and limits
# ---------------------------------------------------------------------------

def _bshd(t):
    """(B,H,S,dh) -> (B,S,H,dh)."""
    return t.permute(0, 2, 1, 3).contiguous()


@functools.lru_cache(maxsize=None)
def attn_ref(name):
    """dict of fp64 O, LSE, dQ, dK, dV in the kernels' layouts ((B,S,H,dh),
    LSE (B,H,Sq)) and their limits lim_*."""
    c = attn_case(name)
    scale, dh = c["scale"], c["dh"]
    # (B,H,S,dh)
    q, k, v, do = (c[n].double().permute(0, 2, 1, 3)
                   for n in ("q", "k", "v", "do"))
    vis, inc = c["vis"][:, None], c["inc"][:, None]     # (B,1,Sq,Sk), (B,1,Sq)
    kT, vT = k.transpose(-1, -2), v.transpose(-1, -2)
    s = torch.where(vis, scale * (q @ kT), -math.inf)
    lse = torch.where(inc, torch.logsumexp(s, -1), 0.0)
    P = torch.exp(s - lse[..., None])
    O = P @ v
    D = (do * O).sum(-1)
    dP = do @ vT
    dS = scale * P * (dP - D[..., None])
    dV = P.transpose(-1, -2) @ do
    dQ = dS @ k
    dK = dS.transpose(-1, -2) @ q

    A = scale * (q.abs() @ kT.abs())
    d32 = 2.0 ** -24 * (dh + 8) * A + 2.0 ** -20
    delta = U + d32
    dmax = float(delta[vis.expand_as(delta)].max())
    Pd = P * delta
    lim_L = Pd.sum(-1) / (1 - dmax) + 1e-5 * (1 + lse.abs())
    dev = torch.empty_like(O)       # sum_j P delta |v_jc - O_ic|
    step = max(1, (1 << 22) // max(1, Pd.numel()))
    for c0 in range(0, dh, step):
        sl = slice(c0, c0 + step)
        # (B,H,Sq,Sk,step)
        diff = (v[:, :, None, :, sl] - O[:, :, :, None, sl]).abs()
        dev[..., sl] = (Pd[..., None] * diff).sum(-2)
    lim_O = U * O.abs() + dev / (1 - dmax) + 1e-5 * (P @ v.abs())
    ado = do.abs()
    lim_dV = U * dV.abs() \
        + 1.01 * ((P * (delta + lim_L[..., None])).transpose(-1, -2) @ ado) \
        + 1e-5 * (P.transpose(-1, -2) @ ado)
    rho = d32 + lim_L[..., None]
    errD = (ado * lim_O).sum(-1) + 1e-5 * (do * O).abs().sum(-1)
    errS = scale * P * (rho * (dP - D[..., None]).abs() + errD[..., None]
                        + 1e-5 * (ado @ vT.abs())) + U * dS.abs()
    lim_dQ = U * dQ.abs() + 1.01 * (errS @ k.abs()) + 1e-5 * (dS.abs() @ k.abs())
    lim_dK = U * dK.abs() + 1.01 * (errS.transpose(-1, -2) @ q.abs()) \
        + 1e-5 * (dS.abs().transpose(-1, -2) @ q.abs())
    r = dict(O=_bshd(O), LSE=lse, dQ=_bshd(dQ), dK=_bshd(dK), dV=_bshd(dV),
             lim_O=_bshd(lim_O), lim_LSE=lim_L, lim_dQ=_bshd(lim_dQ),
             lim_dK=_bshd(lim_dK), lim_dV=_bshd(lim_dV))
    for t in r.values():
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all())
    return r


def check_output(name, which, got, tag=None):
    """One of OUTPUTS against the fp64 reference.  got: CPU tensor in the
    kernel's layout.  Everything must be finite; O / LSE / dQ are compared at
    the rows that see a key, and in the segment kernels O and dQ are exact
    zeros at the others."""
    c, r = attn_case(name), attn_ref(name)
    tag = f"{tag or name} {which}"
    ref, lim = r[which], r["lim_" + which]
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape))
    assert bool(torch.isfinite(got.float()).all()), f"{tag}: non-finite output"
    inc = c["inc"]
    if which in ("O", "dQ"):
        if c["q_seg"] is not None:
            assert bool((got[~inc] == 0).all()), f"{tag}: rows without a key"
        got, ref, lim = got[inc], ref[inc], lim[inc]
    elif which == "LSE":
        got, ref, lim = (t.permute(0, 2, 1)[inc] for t in (got, ref, lim))
    _check_lim(got, ref, lim, tag)


def check_all(name, outs, tag=None, which=OUTPUTS):
    for w in which:
        check_output(name, w, outs[w], tag)


# ---------------------------------------------------------------------------
# fp32 emulation of the kernels
# ---------------------------------------------------------------------------

PERTURBS = ("causal_plus_1", "drop_last_live", "pad_key_live",
            "tail_key_live", "lse_stale", "D_from_unrounded_O_wrong_row",
            "scale_missing")


def _bf(t):
    return t.bfloat16().float()


def attn_emulate(name, perturb=None):
    """The kernels' arithmetic in plain fp32 torch, in their order: fp32
    scores with -inf selection, row max, p = exp(s - m) rounded to bf16, l
    from the rounded p, O = bf16(pV / l), lse = m + log l; backward with
    exp(s - lse), a bf16 P for dV, a bf16 dS that includes scale, D from the
    bf16 O.  Returns a dict of OUTPUTS (bf16, LSE fp32).

    perturb makes it wrong the way a subtly wrong kernel would be."""
    assert perturb is None or perturb in PERTURBS
    c = attn_case(name)
    B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
    f32 = torch.float32
    scale = torch.tensor(c["scale"], dtype=f32)
    q, k, v, do = (c[n].float().permute(0, 2, 1, 3)
                   for n in ("q", "k", "v", "do"))
    vis = c["vis"].clone()
    live = (c["kv_pad"] == 0) if c["q_seg"] is None \
        else (c["kv_seg"] != 0)                         # (B,Sk)
    ii = torch.arange(Sq)[:, None]
    jj = torch.arange(Sk)[None, :]
    if perturb == "causal_plus_1":
        assert c["causal"]
        vis |= (jj == ii + 1)[None] & live[:, None, :]
    elif perturb == "drop_last_live":
        for b in range(B):
            vis[b, :, int(live[b].nonzero().max())] = False
    elif perturb == "pad_key_live":
        for b in range(B):
            if not bool(live[b].all()):
                j = int((~live[b]).nonzero().min())
                vis[b, :, j] = (j <= ii[:, 0]) if c["causal"] \
                    else torch.ones(Sq, dtype=torch.bool)
    elif perturb == "tail_key_live":
        # the key at index Sk of a ragged tile: zero vectors, logit 0
        assert Sk % 64 and not c["causal"]
        z = torch.zeros_like(k[:, :, :1])
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
        vis = torch.cat([vis, torch.ones(B, Sq, 1, dtype=torch.bool)], 2)
    vis = vis[:, None]                                  # (B,1,Sq,Sk)
    inc = vis.any(-1)                                   # (B,1,Sq)
    s = torch.where(vis, (q @ k.transpose(-1, -2)) * scale, -math.inf)
    m = torch.where(inc, s.max(-1).values, 0.0)
    p = _bf(torch.exp(s - m[..., None]))
    l = torch.where(inc, p.sum(-1), 1.0)
    o = ((p @ v) / l[..., None]).bfloat16()
    lse = m + torch.log(l)
    assert s.dtype == f32 and lse.dtype == f32

    lse_b = lse
    if perturb == "lse_stale":      # without the last key tile
        k0 = (Sk - 1) // 64 * 64
        assert k0 > 0
        head = s[..., :k0]
        has = torch.isfinite(head).any(-1)
        stale = torch.logsumexp(torch.where(has[..., None], head, 0.0), -1)
        lse_b = torch.where(has, stale, lse)
    p2 = torch.where(vis, torch.exp(s - lse_b[..., None]), 0.0)
    D = (do * o.float()).sum(-1)
    if perturb == "D_from_unrounded_O_wrong_row":
        D = torch.roll(D, -1, dims=-1)
    dP = do @ v.transpose(-1, -2)
    dS = _bf(p2 * (dP - D[..., None]) * scale)
    dV = _bf(p2).transpose(-1, -2) @ do
    dQ = dS @ k
    if perturb == "scale_missing":
        dQ = dQ / scale
    dK = dS.transpose(-1, -2) @ q
    assert dS.dtype == f32 and dV.dtype == f32
    return dict(O=_bshd(o), LSE=lse, dQ=_bshd(dQ.bfloat16()),
                dK=_bshd(dK[:, :, :Sk].bfloat16()),
                dV=_bshd(dV[:, :, :Sk].bfloat16()))


def perturb_applies(name, perturb):
    """Whether a perturbation changes something that a check can tell from
    rounding.  The limits are sums of magnitudes over a row's keys, each
    term with a slack of about u, so the weight of ONE key among n of equal
    weight (1/n of the row) is inside the slack once n reaches 1/u = 256:
    the one-key and one-tile mistakes of l / lse are asked of Sk < 256."""
    c = attn_case(name)
    plain = c["q_seg"] is None
    padded = bool(c["kv_pad"].any())
    if perturb == "causal_plus_1":
        return c["causal"] and c["Sk"] > 1
    if perturb == "drop_last_live":
        # every row keeps another key: two live keys, and under causal the
        # rows that see the last live key see an earlier one too
        return plain and int((c["kv_pad"] == 0).sum(-1).min()) >= 2 and \
            not c["excluded"]
    if perturb == "pad_key_live":
        return plain and padded
    if perturb == "tail_key_live":
        return plain and c["Sk"] % 64 != 0 and not c["causal"] and \
            c["Sk"] < 1 / U
    if perturb == "lse_stale":
        # the last key tile must hold a share of a row's weight that the
        # limits can see: non-causal rows (every row meets the last tile),
        # its keys live
        k0 = (c["Sk"] - 1) // 64 * 64
        return k0 > 0 and not c["causal"] and c["bwd"] and \
            c["Sk"] < 1 / U and bool(c["vis"][:, :, k0:].any())
    if perturb == "D_from_unrounded_O_wrong_row":
        return c["Sq"] >= 2 and c["bwd"]
    if perturb == "scale_missing":
        # with one visible key dP = D: dS and dQ are exact zeros
        return c["bwd"] and int(c["vis"].sum(-1).max()) >= 2
    raise ValueError(perturb)
