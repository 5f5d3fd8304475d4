"""Which hand-written GEMM runs each forward / dX / dW product, and the
per-step cache of transposed weights the dX path contracts against.

Every choice here is measured per shape (docs/PERF.md round 2,
tools/gemm_bench.py); hipBLASLt survives only as the TFMX_FWD_GEMM=blaslt /
TFMX_DX=blaslt A/B arms.  ops/functional.py calls these from its autograd
wrappers and re-exports the public names.
"""

from __future__ import annotations

import os

import torch

from . import ext


class _WeightTransposeCache:
    """W[N,K]^T copies, one (K, Np) buffer per registered weight, refreshed
    together in ONE transpose_batch launch per optimizer step.

    `version` is bumped by NoamAdam.step (bump_weight_version); the first
    lookup after a bump relaunches transpose_batch over the descriptor
    `table` (one row per 64x64 tile of every registered weight).  A captured
    step records that launch, so graph replays refresh too (graph.py bumps
    before capture).

    Lifetime rule: a captured hipGraph holds the ADDRESS of the table it
    recorded.  When the registry grows the table is rebuilt, and every
    earlier table stays alive in `tables_keep` for the life of the process —
    freeing one would let a replay read freed memory.  Building a table does
    a host->device copy, which is illegal during capture, so
    CapturedTrainStep calls prepare() between warmup and capture."""

    def __init__(self):
        self.version = 0
        self.entries: dict = {}   # id(weight) -> [version, buf, weight]
        self.table = None         # current transpose_batch descriptor table
        self.tables_keep: list = []

    def bump(self):
        self.version += 1

    def _build_table(self, device):
        rows = []
        for ver, buf, w in self.entries.values():
            M, N = w.shape
            ldo = buf.stride(0)
            for bm in range(0, M, 64):
                for bn in range(0, N, 64):
                    rows.append([w.data_ptr(), buf.data_ptr(), M, N, ldo,
                                 bm, bn])
        t = torch.tensor(rows, dtype=torch.int64).to(device)
        self.tables_keep.append(t)
        return t

    def prepare(self):
        if self.entries and self.table is None:
            dev = next(iter(self.entries.values()))[1].device
            self.table = self._build_table(dev)

    def refresh(self, E):
        """Relaunch transpose_batch NOW and mark every entry current,
        instead of waiting for the first stale lookup.  A captured
        optimizer-apply graph records this right after its Adam kernel, so
        the micro-batch graphs replayed after it find fresh transposes and
        record no refresh of their own.  The table must exist already when
        this runs under capture (prepare())."""
        if not self.entries:
            return
        if self.table is None:
            dev = next(iter(self.entries.values()))[1].device
            self.table = self._build_table(dev)
        E.transpose_batch(self.table)
        for e in self.entries.values():
            e[0] = self.version

    def get(self, E, w, gran=64):
        """W[N,K]^T in a (K, Np) buffer, Np = N rounded up to `gran` (pad
        columns zero) — the NT B-operand for dX.  gran=256 matches
        ce_fused's padded dlogits contraction (the ragged-vocab head); the
        generic path uses 64 (the GEMM K-step) so the contraction equals
        dY's width."""
        ent = self.entries.get(id(w))
        npad = (w.shape[0] + gran - 1) // gran * gran
        if ent is None or ent[1].shape[1] != npad:
            buf = torch.zeros(w.shape[1], npad, device=w.device,
                              dtype=w.dtype)
            self.entries[id(w)] = [self.version, buf, w]
            self.table = None  # registry changed; rebuild lazily
            E.transpose2d_into(w, buf)
            return buf
        if ent[0] != self.version:
            if self.table is None:
                self.table = self._build_table(w.device)
            E.transpose_batch(self.table)
            for e in self.entries.values():
                e[0] = self.version
        return ent[1]


_WT_CACHE = _WeightTransposeCache()
_wt_padded = _WT_CACHE.get


def bump_weight_version():
    """The weights changed (optimizer step): cached transposes are stale."""
    _WT_CACHE.bump()


def prepare_weight_caches():
    """Build the transpose_batch descriptor table eagerly (it involves a
    host->device copy, which is illegal inside hipGraph capture) — called
    by CapturedTrainStep between warmup and capture."""
    _WT_CACHE.prepare()


def refresh_weight_caches():
    """Refresh every cached transpose eagerly (see
    _WeightTransposeCache.refresh)."""
    _WT_CACHE.refresh(ext())


# GEMM backend (round 2): every training-shape GEMM runs hand-written.
# Forward goes to the gemm256/128 NT dispatch (measured best hand path:
# 600-1040 TF; the uni counted-vmcnt schedule variants measured slower —
# see gemm_uni.hip header); dX and the wide dW go to the gemm_uni TR-mode
# kernels (tr16 transpose-read operands).  hipBLASLt remains only as the
# TFMX_FWD_GEMM=blaslt A/B arm; TFMX_FWD_GEMM=uni forces uni NT forward.
_FWD_BACKEND = os.environ.get("TFMX_FWD_GEMM", "hand")

_CAPTURE_HINT = False


def set_capture_hint(on: bool):
    """Inside a hipGraph (GraphedDecoder) launch overhead is replayed
    away and the library kernels win even at M=B rows (0.705 vs 0.788
    ms/token); eager small-M calls keep the cheap-launch hand-written
    kernel.  Set around warmup+capture so both trace the same path."""
    global _CAPTURE_HINT
    _CAPTURE_HINT = on


def _fwd_gemm(E, x, w, b, activation):
    epi = 1 if activation == "relu" else 0
    if _FWD_BACKEND == "blaslt" and b is not None and \
            (x.shape[0] > 1024 or _CAPTURE_HINT):
        # A/B arm: hipBLASLt fused bias/ReLU epilogues (round-1 default)
        if activation == "relu":
            if hasattr(torch, "_addmm_activation"):
                return torch._addmm_activation(b, x, w.t())
            return torch.relu(torch.nn.functional.linear(x, w, b))
        return torch.nn.functional.linear(x, w, b)
    if _FWD_BACKEND == "uni" and E.gemm_uni_viable(x.shape[0], w.shape[0],
                                                   x.shape[1]):
        return E.gemm_uni_nt(x, w, b, epi)
    # default: gemm256/128 dispatch (best-measured hand-written NT path;
    # launch is cheaper than the library's at small M, decode/serving)
    return E.gemm_nt(x, w, b if b is not None else torch.Tensor(), epi)


def _dw_gemm(dy, x, out=None):
    """dW[N,K] = dY^T @ X — plain GEMM, hand-written both ways: the wide
    logits head goes to the deep-pipelined TRxTR gemm_uni_tn (both
    operands tr16 transpose-read), the d_model-sized heads to the
    split-contraction gemm_dw kernel (tools/gemm_bench.py)."""
    E = ext()
    npad = (dy.shape[1] + 255) // 256 * 256
    if dy.shape[1] >= 8192 and dy.shape[0] % 64 == 0 \
            and (dy.shape[1] % 256 == 0 or dy.stride(0) >= npad) \
            and x.shape[1] % 128 == 0:
        N = dy.shape[1]
        main = (N // 256) * 256
        if main != N and main > 0:
            if out is None:
                out = torch.empty(N, x.shape[1], device=dy.device,
                                  dtype=dy.dtype)
            # Grid-quantization cliff: ceil(N/256) tiles puts the grid a
            # couple of blocks past 256 (one per CU at this kernel's LDS),
            # and the stragglers cost a whole second pass.  Compute the
            # 256-aligned main span at exactly one block wave, then the
            # ragged vocab tail (a few rows, full contraction) split-K so
            # it also fills the chip for its instant of work.
            E.gemm_uni_tn(dy[:, :main], x, out[:main], 1)
            E.gemm_uni_tn(dy[:, main:], x, out[main:], 64)
            return out
        return E.gemm_uni_tn(dy, x, out)
    # gemm_dw writes DISJOINT per-slice fp32 partials (no atomics, no
    # zeroing — the fp32-atomic epilogue measured at the chip's atomic
    # rate); it sizes its own torch::empty workspace via the caching
    # allocator, so no Python-side workspace is needed.
    return E.gemm_dw(dy.contiguous(), x, out, None, None)


def _dw_db_gemm(dy, x, has_bias, w_out=None, b_out=None, db=None):
    """dW and (optionally) db together.  gemm_dw CAN fuse db into its dY
    stream, but the fused variant costs 138 vs 116 VGPRs — one whole
    workgroup of block-level overlap per CU — and measured slower
    end-to-end than a separate colsum pass, so db is a pass of its own
    (the row-streaming colsum) unless the caller hands in a finished
    `db`: the relu backward sums dz in the kernel that writes it."""
    E = ext()
    dw = _dw_gemm(dy, x, out=w_out)
    if db is None and has_bias:
        db = E.colsum(dy, b_out)
    return dw, db


# dX backend: "wt" contracts against a per-step cached transposed weight
# through the fast NT path; "uni" reads W red-major via tr16 (no
# transpose); "blaslt" is the library A/B arm.  Default = measured winner.
_DX_BACKEND = os.environ.get("TFMX_DX", "wt")


def _dense2d(t):
    """Row-strided dense (stride(1)==1) passes through — ce_fused's padded
    dlogits view must NOT be copied back to contiguous."""
    return t if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) \
        else t.contiguous()


def _dx_gemm(E, dy, w):
    """dX[M,K] = dY[M,N] @ W[N,K] — hand-written: either NT against the
    cached W^T (refreshed once per optimizer step) or NTxTR with W read
    red-major via tr16.  The ragged-vocab head's dY arrives as ce_fused's
    zero-padded row-strided view; the contraction widens to the 256-aligned
    pad (zero columns) against the padded-transposed weight."""
    N = w.shape[0]
    M = dy.shape[0]
    if _DX_BACKEND == "blaslt":
        return torch.matmul(dy, w)
    npad = (N + 255) // 256 * 256
    padded = (npad != N and dy.stride(1) == 1 and dy.stride(0) == npad
              and dy.storage_offset() == 0)
    if padded and E.gemm_uni_viable(M, w.shape[1], npad):
        full = dy.as_strided((M, npad), (npad, 1))
        return E.gemm_nt(full, _wt_padded(E, w, 256), torch.Tensor(), 0)
    if _DX_BACKEND == "wt" and N % 64 == 0 and M >= 2048:
        return E.gemm_nt(_dense2d(dy), _wt_padded(E, w), torch.Tensor(), 0)
    if N % 64 == 0 and E.gemm_uni_viable(M, w.shape[1], N):
        return E.gemm_uni_nn(dy, w)
    return torch.matmul(dy, w)  # small/odd shapes (not a training shape)


def _dx_epilogue_ok(E, M, n_out, k):
    """Whether the dX GEMM (M, n_out, k) would run on the gemm256 kernel —
    the only one carrying the relu-mask / residual-add epilogues — through
    the cached-W^T backend.  Opt-in, TFMX_FFN_BWD=fused (A/B arm, read per
    call).  Since the epilogue reads aux in 8/16-byte row-contiguous pieces
    both fused GEMMs beat GEMM + separate pass per op (docs/PERF.md); the
    default is still split because tests/test_gpu_fused_backward.py pins
    the unset arm to two _dx_gemm calls — flipping it goes with a rewrite
    of that test."""
    return (os.environ.get("TFMX_FFN_BWD", "split") == "fused"
            and _DX_BACKEND == "wt" and M >= 2048
            and n_out % 64 == 0 and k % 64 == 0
            and E.gemm256_viable(M, n_out, k))
