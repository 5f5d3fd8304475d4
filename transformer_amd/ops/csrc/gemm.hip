// MFMA bf16 GEMM (NT / NN / TN layouts) + small helper kernels.
//
// Implements SURVEY.md §2.3 K1/K7/K8/K12: every linear layer of the model
// (packed QKV, attention out-proj, FFN with fused ReLU, the V≈32k logits
// head) runs through these kernels:
//   gemm_nt: C[M,N] = A[M,K] @ B[N,K]^T (+bias)(+ReLU)   — forward
//   gemm_nn: C[M,N] = A[M,K] @ B[K,N]                    — dX = dY @ W
//   gemm_tn: C[M,N] = A[K,M]^T @ B[K,N]                  — dW = dY^T @ X
// bf16 inputs, fp32 MFMA accumulate, bf16 out.  The NN/TN variants read the
// "transposed" operand through an LDS-bounce staging (global->linear scratch
// coalesced, scratch->swizzled tile conflict-free), so linear backward needs
// NO physical transpose kernels or extra HBM round-trips.
//
// CDNA4 design (see /opt/skills guides): 128x128 output tile per 4-wave
// (256-thread) workgroup, BK=64 K-steps staged through LDS with an
// XOR bank-swizzle (byte ^= (row&7)<<4) so ds_read_b128 fragment reads are
// ≤2-way conflicting; mfma_f32_16x16x32_bf16 with 4x4 fragments per wave
// (64x64 per wave); bias/ReLU fused in the epilogue; XCD-aware workgroup
// remap for L2 affinity (8 XCDs with private L2s).
#include "common.h"

#include <cstdint>
#include <cstring>
#include <map>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define BM 128
#define BN 128
#define BK 64
#define NTHREADS 256
// scratch row stride (elems) for transposed staging: 68 dwords per row keeps
// rows 16B-aligned and spreads the step-2 column reads over the banks.
#define SCR_LD 136

// LDS tiles are [128 rows][64 cols] bf16 = 128 B per row.  Byte-offset
// swizzle spreads the 16-lane ds_read_b128 groups over 8 slots (T2 recipe).
DEV_INLINE int lds_off(int row, int col_bytes) {
  return row * (BK * 2) + (col_bytes ^ ((row & 7) << 4));
}

// Stage one [128][BK] bf16 tile from global (row-major, stride ldg elems)
// into LDS via registers + swizzled ds_write_b128.  Each of the 256 threads
// writes 4 16-byte chunks.  Guards rows >= nrows and cols >= ncols (zeros).
template <bool ALIGNED>
DEV_INLINE void stage_tile(const short* __restrict__ g, int ldg, int nrows,
                           int ncols, short* lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int idx = p * NTHREADS + t;          // 1024 chunks of 8 elems
    int row = idx >> 3;                  // /8 chunks per row
    int c8 = (idx & 7) << 3;             // starting col
    s16x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (row < nrows) {
      const short* src = g + (long)row * ldg + c8;
      if (ALIGNED && c8 + 8 <= ncols) {
        s16x8 vv = *(const s16x8*)src;
        lo = {vv[0], vv[1], vv[2], vv[3]};
        hi = {vv[4], vv[5], vv[6], vv[7]};
      } else if ((ldg & 1) == 0 && c8 + 8 <= ncols) {
        // 4-byte-aligned rows (even leading dim): s16x2 loads, 4x fewer
        // transactions than scalar (hits e.g. the V=32770 logits backward)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s16x2 p = *(const s16x2*)(src + 2 * j);
          if (j < 2) { lo[2 * j] = p[0]; lo[2 * j + 1] = p[1]; }
          else { hi[2 * (j - 2)] = p[0]; hi[2 * (j - 2) + 1] = p[1]; }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (c8 + j < ncols) lo[j] = src[j];
          if (c8 + 4 + j < ncols) hi[j] = src[4 + j];
        }
      }
    }
    int off = lds_off(row, c8 * 2);
    *(s16x4*)((char*)lds + off) = lo;
    *(s16x4*)((char*)lds + off + 8) = hi;
  }
}

// Transposed staging, step 1 (global -> linear scratch, coalesced):
// scratch[c][r] = g[c*ldg + r] for c<64 contraction rows, r<128 tile rows.
// g points at the (k0, tilerow0) corner of the region.
template <bool ALIGNED>
DEV_INLINE void stage_tr_scr(const short* __restrict__ g, int ldg, int nrows,
                             int ncols, short* scr) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int idx = p * NTHREADS + t;   // 1024 chunks of 8 elems
    int c = idx >> 4;             // contraction row 0..63
    int r8 = (idx & 15) << 3;     // tile-row 0..120
    s16x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (c < ncols) {
      const short* src = g + (long)c * ldg + r8;
      if (ALIGNED && r8 + 8 <= nrows) {
        s16x8 vv = *(const s16x8*)src;
        lo = {vv[0], vv[1], vv[2], vv[3]};
        hi = {vv[4], vv[5], vv[6], vv[7]};
      } else if ((ldg & 1) == 0 && r8 + 8 <= nrows) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s16x2 pr = *(const s16x2*)(src + 2 * j);
          if (j < 2) { lo[2 * j] = pr[0]; lo[2 * j + 1] = pr[1]; }
          else { hi[2 * (j - 2)] = pr[0]; hi[2 * (j - 2) + 1] = pr[1]; }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (r8 + j < nrows) lo[j] = src[j];
          if (r8 + 4 + j < nrows) hi[j] = src[4 + j];
        }
      }
    }
    *(s16x4*)&scr[c * SCR_LD + r8] = lo;
    *(s16x4*)&scr[c * SCR_LD + r8 + 4] = hi;
  }
}

// Transposed staging, step 2 (scratch -> swizzled tile): tile[r][c] =
// scr[c][r].  Per wave-instruction: rows rbase..rbase+7 (j = lane&7) x
// column-pairs cbase..cbase+7 (i = lane>>3) as b32 writes — conflict-free
// writes, 2-way scratch reads (SCR_LD = 68 dwords spreads 8c+r/2).
DEV_INLINE void stage_tr_tile(const short* __restrict__ scr, short* lds) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = lane & 7, i = lane >> 3;
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    int task = p * 4 + wid;            // 64 (rbase, cbase) wave-tasks
    int r = ((task & 15) << 3) + j;    // tile row
    int c2 = ((task >> 4) << 3) + i;   // column pair index (of 32)
    s16x2 v = {scr[(2 * c2) * SCR_LD + r], scr[(2 * c2 + 1) * SCR_LD + r]};
    *(s16x2*)((char*)lds + lds_off(r, 4 * c2)) = v;
  }
}

DEV_INLINE bf16x8 read_frag(const short* lds, int row, int kbase) {
  int off = lds_off(row, kbase * 2);
  s16x8 v0 = *(const s16x8*)((const char*)lds + off);
  return (bf16x8)v0;
}

// global_load_lds staging (guide §5 step-3 / rule 21): LDS image stays the
// SWIZZLED layout, built with a lane-linear LDS destination by inverse-
// swizzling the per-lane SOURCE address.  16 wave-instructions stage a
// [128][64] bf16 tile.  Requires a full tile (no row/col guards).
DEV_INLINE void stage_tile_glds(const short* __restrict__ g, int ldg,
                                short* lds) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int chunk = p * 4 + wid;            // 16 chunks of 1 KiB
    const int idx = chunk * 64 + lane;        // 16-B unit index
    const int row = idx >> 3;
    const int colb = ((idx & 7) << 4) ^ ((row & 7) << 4);  // inverse swizzle
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(g + (long)row * ldg +
                                                        (colb >> 1)),
        (__attribute__((address_space(3))) void*)((char*)lds + chunk * 1024),
        16, 0, 0);
  }
}

// SPLITK=false: writes bf16 C directly with fused bias/ReLU.
// SPLITK=true (blockIdx.y = K-slice): fp32 atomicAdd partials into CW;
// bias/epilogue applied by gemm_finalize_kernel after all slices land.
// Split-K keeps the chip full on deep-K small-MN GEMMs (the dW shapes:
// e.g. 512x512xK=16384 is only 16 workgroups unsplit).
//
// TA/TB select transposed staging for A/B: the operand is stored
// contraction-major (element (tile_row r, contraction c) at g[c*ld + r]).
template <int EPILOGUE, bool TA, bool TB, bool ALIGNED_A, bool ALIGNED_B,
          bool SPLITK>
__global__ __launch_bounds__(NTHREADS)
void gemm_kernel(const short* __restrict__ A, const short* __restrict__ B,
                 const short* __restrict__ bias, short* __restrict__ C,
                 float* __restrict__ CW, int M, int N, int K, int lda, int ldb,
                 int has_bias, int nbm, int nbn, int k_per_slice) {
  // Dynamic LDS: [a_tile BM*BK][b_tile BN*BK][scratch iff TA||TB].
  // Single-buffered tiles: measured FASTER than a 64 KiB double buffer at
  // this occupancy — block-level overlap already hides the glds latency
  // (guide §5 regime note).
  extern __shared__ short smem[];
  short* a_lds = smem;
  short* b_lds = smem + BM * BK;
  short* scr = smem + BM * BK + BN * BK;  // only sized when TA||TB

  // XCD-aware bijective remap (guide T1): contiguous grid chunk per XCD.
  int nwg = nbm * nbn;
  int wg = blockIdx.x;
  {
    int q = nwg / 8, r = nwg % 8, x = wg % 8, o = wg / 8;
    wg = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + o;
  }
  const int bm0 = (wg / nbn) * BM;
  const int bn0 = (wg % nbn) * BN;

  const int wid = threadIdx.x >> 6;      // wave 0..3 -> 2x2
  const int lane = threadIdx.x & 63;
  const int wr = (wid >> 1) * 64;        // wave row offset in tile
  const int wc = (wid & 1) * 64;
  const int fr = lane & 15;              // fragment row/col lane index
  const int kg = lane >> 4;              // k-group 0..3

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0, 0, 0, 0};

  const int mrows = min(BM, M - bm0);
  const int nrows = min(BN, N - bn0);
  // glds fast path (NT only): full output tile and K a multiple of BK.
  const bool glds = !TA && !TB && ALIGNED_A && ALIGNED_B && mrows == BM &&
                    nrows == BN && (K % BK) == 0;
  int k_lo = 0, k_hi = K;
  if (SPLITK) {
    k_lo = blockIdx.y * k_per_slice;
    k_hi = min(K, k_lo + k_per_slice);
  }

#define MFMA_TILE(a_lds_, b_lds_)                                          \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                       \
    bf16x8 af[4], bf_[4];                                                  \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
        af[i] = read_frag(a_lds_, wr + i * 16 + fr, ks * 32 + kg * 8);     \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                          \
        bf_[j] = read_frag(b_lds_, wc + j * 16 + fr, ks * 32 + kg * 8);    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                      \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(           \
                af[i], bf_[j], acc[i][j], 0, 0, 0);                        \
  }

  if (glds) {
    for (int k0 = k_lo; k0 < k_hi; k0 += BK) {
      stage_tile_glds(A + (long)bm0 * lda + k0, lda, a_lds);
      stage_tile_glds(B + (long)bn0 * ldb + k0, ldb, b_lds);
      __syncthreads();              // drains the LDS-DMA queue (vmcnt 0)
      MFMA_TILE(a_lds, b_lds);
      __syncthreads();
    }
  } else {
    for (int k0 = k_lo; k0 < k_hi; k0 += BK) {
      int kc = min(BK, K - k0);
      if (!TA)
        stage_tile<ALIGNED_A>(A + (long)bm0 * lda + k0, lda, mrows, kc, a_lds);
      if (!TB)
        stage_tile<ALIGNED_B>(B + (long)bn0 * ldb + k0, ldb, nrows, kc, b_lds);
      if (TA) {
        stage_tr_scr<ALIGNED_A>(A + (long)k0 * lda + bm0, lda, mrows, kc, scr);
        __syncthreads();
        stage_tr_tile(scr, a_lds);
      }
      if (TB) {
        if (TA) __syncthreads();  // a_lds staging read scr; wait before reuse
        stage_tr_scr<ALIGNED_B>(B + (long)k0 * ldb + bn0, ldb, nrows, kc, scr);
        __syncthreads();
        stage_tr_tile(scr, b_lds);
      }
      __syncthreads();
      MFMA_TILE(a_lds, b_lds);
      __syncthreads();
    }
  }
#undef MFMA_TILE

  // Epilogue: C/D lane map is col = lane&15, row = (lane>>4)*4 + r.
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int grow_base = bm0 + wr + i * 16 + kg * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int gcol = bn0 + wc + j * 16 + fr;
      if (gcol >= N) continue;
      float bv = (!SPLITK && has_bias && bias) ? bfbits2f(bias[gcol]) : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int grow = grow_base + r;
        if (grow >= M) continue;
        if (SPLITK) {
          atomicAdd(&CW[(long)grow * N + gcol], acc[i][j][r]);
        } else {
          float v = acc[i][j][r] + bv;
          if (EPILOGUE == 1) v = fmaxf(v, 0.0f);
          C[(long)grow * N + gcol] = f2bfbits(v);
        }
      }
    }
  }
}

// finalize for the split-K path: C = epi(CW + bias) in bf16
template <int EPILOGUE>
__global__ void gemm_finalize_kernel(const float* __restrict__ cw,
                                     const short* __restrict__ bias,
                                     short* __restrict__ c, long mn, int N,
                                     int has_bias) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= mn) return;
  float v = cw[i];
  if (has_bias && bias) v += bfbits2f(bias[i % N]);
  if (EPILOGUE == 1) v = fmaxf(v, 0.0f);
  c[i] = f2bfbits(v);
}

// ---------------------------------------------------------------------------
// transpose2d: [M,N] bf16 -> [N,M].  64x64 tiles, padded LDS, short4 IO.
// (No longer on the linear-backward hot path — kept as a utility op.)
// ---------------------------------------------------------------------------
DEV_INLINE void transpose_tile(const short* __restrict__ in,
                               short* __restrict__ out, int M, int N,
                               long ldo, int bm, int bn,
                               short tile[64][64 + 8]) {
  int t = threadIdx.x;
  const bool interior = (bm + 64 <= M) && (bn + 64 <= N);
  if (interior) {
    // vectorized: 512 short8 chunks, 2 per thread
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      int idx = p * 256 + t;
      int r = idx >> 3, c8 = (idx & 7) << 3;
      *(s16x8*)&tile[r][c8] = *(const s16x8*)(in + (long)(bm + r) * N + bn + c8);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      int idx = p * 256 + t;
      int r = idx >> 3, c8 = (idx & 7) << 3;  // output row r (= col of in)
      s16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = tile[c8 + j][r];
      *(s16x8*)(out + (bn + r) * ldo + bm + c8) = v;
    }
  } else {
    for (int p = 0; p < 16; ++p) {
      int idx = p * 256 + t;
      int r = idx >> 6, c = idx & 63;
      int gr = bm + r, gc = bn + c;
      tile[r][c] = (gr < M && gc < N) ? in[(long)gr * N + gc] : (short)0;
    }
    __syncthreads();
    for (int p = 0; p < 16; ++p) {
      int idx = p * 256 + t;
      int r = idx >> 6, c = idx & 63;
      int gr = bn + r, gc = bm + c;
      if (gr < N && gc < M) out[gr * ldo + gc] = tile[c][r];
    }
  }
}

__global__ __launch_bounds__(256)
void transpose2d_kernel(const short* __restrict__ in, short* __restrict__ out,
                        int M, int N, long ldo) {
  __shared__ short tile[64][64 + 8];  // +8 elems (16 B) row pad vs conflicts
  int tb = blockIdx.x, nbx = (N + 63) >> 6;
  transpose_tile(in, out, M, N, ldo, (tb / nbx) << 6, (tb % nbx) << 6, tile);
}

// Batched transpose over a device descriptor table: ONE launch per step
// refreshes every cached transposed weight (the per-weight transpose2d
// launches were ~67/step = 0.35 ms of launch floor).  desc row (int64 x7):
// [src_ptr, dst_ptr, M, N, ldo, bm, bn] — one row per 64x64 tile.
__global__ __launch_bounds__(256)
void transpose_batch_kernel(const long* __restrict__ desc) {
  __shared__ short tile[64][64 + 8];
  const long* d = desc + (long)blockIdx.x * 7;
  transpose_tile((const short*)d[0], (short*)d[1], (int)d[2], (int)d[3],
                 d[4], (int)d[5], (int)d[6], tile);
}

// colsum: db[N] = sum_m dy[M,N] (fp32 accumulate, bf16 out).
// colsum_kernel is the column-parallel form: one thread per column, 2-byte
// loads.  It runs where colsum_rows_kernel (below) cannot — rows that are
// not 16-byte aligned —, below 512 columns, and as the TFMX_COLSUM=cols
// A/B arm.
// Two-stage: (col-chunk, row-chunk) blocks fill the chip, fp32 atomics
// into a workspace, then cast.  The workspace is CACHED per (device, N)
// and re-zeroed by the cast kernel, so the zero-fill launch happens once
// per shape, not once per call (~130 fill launches/step saved).  A
// disjoint-partials scheme (no atomics) was tried and measured SLOWER:
// its gy-deep serial reduction ran on a 2-8 block grid.
#define COLSUM_ROWS 128
// Single launch: partial atomics + last-arriver finalize (cast to bf16 and
// re-zero the cached workspace) — the separate cast kernel was ~67
// launch-floor dispatches per step.  acc holds N fp32 + 1 counter word.
__global__ __launch_bounds__(256)
void colsum_kernel(const short* __restrict__ dy, float* __restrict__ acc,
                   short* __restrict__ out, int M, int N, long lda) {
  int n = blockIdx.x * 256 + threadIdx.x;
  if (n < N) {
    long m0 = (long)blockIdx.y * COLSUM_ROWS;
    long m1 = min((long)M, m0 + COLSUM_ROWS);
    // 4 independent accumulators for memory-level parallelism
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    long m = m0;
    for (; m + 4 <= m1; m += 4) {
      s0 += bfbits2f(dy[m * lda + n]);
      s1 += bfbits2f(dy[(m + 1) * lda + n]);
      s2 += bfbits2f(dy[(m + 2) * lda + n]);
      s3 += bfbits2f(dy[(m + 3) * lda + n]);
    }
    for (; m < m1; ++m) s0 += bfbits2f(dy[m * lda + n]);
    atomicAdd(&acc[n], (s0 + s1) + (s2 + s3));
  }
  if (last_arriver((unsigned*)(acc + N), gridDim.x * gridDim.y)) {
    for (int i = threadIdx.x; i < N; i += 256) {
      out[i] = f2bfbits(acc[i]);
      acc[i] = 0.f;  // workspace stays zeroed for the next call
    }
    if (threadIdx.x == 0)
      __hip_atomic_store((unsigned*)(acc + N), 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Row-streaming column sum (the ln_bwd_fused_kernel recipe): a lane owns 8
// adjacent columns per 512-column chunk (c = panel + k*512 + lane*8, one
// 16-byte load each) and keeps their sums in fp32 registers while the
// block's waves walk the rows grid-stride, the next row's loads issued
// before this row's adds.  Grid: x = column panels of NCH chunks, y = row
// groups of NW waves.  A block combines its waves by a register tree
// through LDS (index c + c/8, no LDS atomics), adds ONE fp32 atomic per
// column into the cached workspace (start segment rotated by row group),
// and the last arriver casts to bf16 and re-zeroes: same workspace
// contract as colsum_kernel.  Needs dy 16-byte aligned and lda % 8 == 0;
// the 8-column group that crosses N (at most one lane per row) is read by
// guarded scalar loads, so nothing past (M-1)*lda + N - 1 is touched.
// RELU: y and dz are (M, N) with the same lda; writes dz = y > 0 ? dy : 0
// (relu_bwd_kernel's predicate and bits) and sums the written value.
template <bool RELU, int NCH, int NW>
__global__ __launch_bounds__(NW * 64)
void colsum_rows_kernel(const short* __restrict__ dy,
                        const short* __restrict__ y, short* __restrict__ dz,
                        float* __restrict__ acc, short* __restrict__ out,
                        int M, int N, long lda) {
  constexpr int LW = NCH * 576;  // one wave's accumulators, padded
  __shared__ float red[(NW / 2) * LW];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int panel = blockIdx.x * (NCH * WAVE * 8);

  int nv[NCH];  // valid columns of the lane's group: 8, 1..7 (tail) or 0
  float a[NCH][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = panel + k * (WAVE * 8) + lane * 8;
    nv[k] = min(8, max(0, N - c));
#pragma unroll
    for (int j = 0; j < 8; ++j) a[k][j] = 0.f;
  }

  auto load8 = [&](const short* __restrict__ p, int n) {
    s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n == 8) {
      v = *(const s16x8*)p;
    } else {
#pragma unroll
      for (int j = 0; j < 7; ++j)
        if (j < n) v[j] = p[j];
    }
    return v;
  };
  s16x8 dv[NCH], yv[NCH], dvn[NCH], yvn[NCH];
  auto load_row = [&](int row, s16x8 (&d)[NCH], s16x8 (&x)[NCH]) {
    const long base = (long)row * lda + panel + lane * 8;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      d[k] = load8(dy + base + k * (WAVE * 8), nv[k]);
      if (RELU) x[k] = load8(y + base + k * (WAVE * 8), nv[k]);
    }
  };
  const int row0 = blockIdx.y * NW + wave, rstep = gridDim.y * NW;
  if (row0 < M) load_row(row0, dvn, yvn);
  for (int row = row0; row < M; row += rstep) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      dv[k] = dvn[k];
      if (RELU) yv[k] = yvn[k];
    }
    if (row + rstep < M) load_row(row + rstep, dvn, yvn);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      if (RELU) {
        s16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = (bfbits2f(yv[k][j]) > 0.f) ? dv[k][j] : (short)0;
        short* q = dz + (long)row * lda + panel + k * (WAVE * 8) + lane * 8;
        if (nv[k] == 8) {
          *(s16x8*)q = o;
        } else {
#pragma unroll
          for (int j = 0; j < 7; ++j)
            if (j < nv[k]) q[j] = o[j];
        }
        dv[k] = o;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) a[k][j] += bfbits2f(dv[k][j]);
    }
  }

  // Block combine: binary tree over the waves, registers to registers (the
  // upper half of the live waves parks, the lower half adds).
  auto park = [&](float* dst) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      if (nv[k] > 0) {
        const int li = (lane + k * WAVE) * 9;
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[li + j] = a[k][j];
      }
    }
  };
#pragma unroll
  for (int half = NW / 2; half >= 1; half >>= 1) {
    if (wave >= half && wave < 2 * half) park(red + (wave - half) * LW);
    __syncthreads();
    if (wave < half) {
      const float* src = red + wave * LW;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        if (nv[k] > 0) {
          const int li = (lane + k * WAVE) * 9;
#pragma unroll
          for (int j = 0; j < 8; ++j) a[k][j] += src[li + j];
        }
      }
    }
    __syncthreads();
  }
  if (wave == 0) park(red);
  __syncthreads();
  // cross-block: one fp32 atomic per column of the panel per block
  const int pw = min(NCH * WAVE * 8, N - panel);
  const int rot = (int)((blockIdx.y * 64u) % (unsigned)pw);
  for (int i = threadIdx.x; i < pw; i += NW * 64) {
    int c = i + rot;
    if (c >= pw) c -= pw;
    atomicAdd(&acc[panel + c], red[c + (c >> 3)]);
  }
  unsigned* cnt = (unsigned*)(acc + N);
  if (last_arriver(cnt, gridDim.x * gridDim.y)) {
    for (int i = threadIdx.x; i < N; i += NW * 64) {
      out[i] = f2bfbits(acc[i]);
      acc[i] = 0.f;
    }
    if (threadIdx.x == 0)
      __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// relu_bwd: dz = dy * (y > 0)
__global__ void relu_bwd_kernel(const short* __restrict__ dy,
                                const short* __restrict__ y,
                                short* __restrict__ dz, long n) {
  long i = (long)(blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i + 8 <= n) {
    s16x8 dv = *(const s16x8*)(dy + i);
    s16x8 yv = *(const s16x8*)(y + i);
    s16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = (bfbits2f(yv[j]) > 0.f) ? dv[j] : (short)0;
    *(s16x8*)(dz + i) = o;
  } else {
    for (long j = i; j < n; ++j)
      dz[j] = (bfbits2f(y[j]) > 0.f) ? dy[j] : (short)0;
  }
}

__global__ void smoke_add_kernel(const short* a, const short* b, short* c,
                                 long n) {
  long i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) c[i] = f2bfbits(bfbits2f(a[i]) + bfbits2f(b[i]));
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
#define CHECK_BF16_2D(t)                                                      \
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kBFloat16 && t.dim() == 2 && \
                  t.is_contiguous(),                                          \
              #t " must be contiguous 2-D bf16 on GPU")

namespace {

// Shared launcher: out dims MxN, contraction K; lda/ldb per TA/TB semantics.
template <bool TA, bool TB>
torch::Tensor gemm_launch(torch::Tensor a, torch::Tensor b, torch::Tensor bias,
                          int64_t epilogue, int M, int N, int K, int lda,
                          int ldb, c10::optional<torch::Tensor> out_opt) {
  bool has_bias = bias.defined() && bias.numel() > 0;
  if (has_bias)
    TORCH_CHECK(bias.is_cuda() && bias.dtype() == torch::kBFloat16 &&
                bias.numel() == N, "bias must be bf16[N]");
  torch::Tensor c;
  if (out_opt.has_value()) {
    c = *out_opt;
    TORCH_CHECK(c.is_cuda() && c.dtype() == torch::kBFloat16 &&
                c.is_contiguous() && c.numel() == (long)M * N,
                "out must be contiguous bf16 with M*N elements");
  } else {
    c = torch::empty({M, N}, a.options());
  }
  int nbm = cdiv(M, BM), nbn = cdiv(N, BN);
  int nwg = nbm * nbn;
  // split-K when the unsplit grid underfills the 256-CU chip and K is deep
  int sk = 1;
  if (nwg < 256 && K >= 4 * BK) {
    sk = std::min({(512 + nwg - 1) / nwg, K / BK, 32});
    sk = std::max(sk, 1);
  }
  int k_per_slice = (cdiv(K, BK) + sk - 1) / sk * BK;
  sk = cdiv(K, k_per_slice);
  dim3 grid(nwg, sk);
  auto stream = at::hip::getCurrentHIPStream();
  bool ala = (lda % 8 == 0);
  bool alb = (ldb % 8 == 0);
  size_t smem = (BM * BK + BN * BK + ((TA || TB) ? 64 * SCR_LD : 0)) *
                sizeof(short);
  torch::Tensor cw;
  float* cwp = nullptr;
  if (sk > 1) {
    cw = torch::zeros({M, N}, a.options().dtype(torch::kFloat32));
    cwp = cw.data_ptr<float>();
  }
  auto launch = [&](auto epi, auto aa, auto ab, auto splitk) {
    gemm_kernel<decltype(epi)::value, TA, TB, decltype(aa)::value,
                decltype(ab)::value, decltype(splitk)::value>
        <<<grid, NTHREADS, smem, stream>>>(
            (const short*)a.data_ptr(), (const short*)b.data_ptr(),
            has_bias ? (const short*)bias.data_ptr() : nullptr,
            (short*)c.data_ptr(), cwp, M, N, K, lda, ldb, has_bias, nbm, nbn,
            k_per_slice);
  };
  using T = std::true_type;
  using F = std::false_type;
  using E0 = std::integral_constant<int, 0>;
  using E1 = std::integral_constant<int, 1>;
  auto dis_al = [&](auto epi, auto splitk) {
    if (ala) { if (alb) launch(epi, T{}, T{}, splitk);
               else launch(epi, T{}, F{}, splitk); }
    else { if (alb) launch(epi, F{}, T{}, splitk);
           else launch(epi, F{}, F{}, splitk); }
  };
  if (sk > 1) {
    if (epilogue == 1) dis_al(E1{}, T{}); else dis_al(E0{}, T{});
    long mn = (long)M * N;
    auto fin = [&](auto epi) {
      gemm_finalize_kernel<decltype(epi)::value>
          <<<(mn + 1023) / 1024, 1024, 0, stream>>>(
              cwp, has_bias ? (const short*)bias.data_ptr() : nullptr,
              (short*)c.data_ptr(), mn, N, has_bias);
    };
    if (epilogue == 1) fin(E1{}); else fin(E0{});
  } else {
    if (epilogue == 1) dis_al(E1{}, F{}); else dis_al(E0{}, F{});
  }
  return c;
}

}  // namespace

// Implemented in gemm256.hip: deep-pipelined 256x256 kernel + viability.
bool gemm256_viable(int M, int N, int K, int lda, int ldb);
torch::Tensor gemm256_nt(torch::Tensor a, torch::Tensor w, torch::Tensor bias,
                         int64_t epilogue, c10::optional<torch::Tensor> out,
                         c10::optional<torch::Tensor> aux);

// C[M,N] = A[M,K] @ W[N,K]^T (+bias)(+ReLU) — forward layout.
torch::Tensor gemm_nt(torch::Tensor a, torch::Tensor w, torch::Tensor bias,
                      int64_t epilogue, c10::optional<torch::Tensor> out) {
  CHECK_BF16_2D(a);
  CHECK_BF16_2D(w);
  const int M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "gemm_nt: K mismatch");
  if (gemm256_viable(M, N, K, K, K))
    return gemm256_nt(a, w, bias, epilogue, out, c10::nullopt);
  return gemm_launch<false, false>(a, w, bias, epilogue, M, N, K, K, K, out);
}

// The 128x128 path with no 256-template dispatch (A/B benchmarking).
torch::Tensor gemm128_nt(torch::Tensor a, torch::Tensor w, torch::Tensor bias,
                         int64_t epilogue, c10::optional<torch::Tensor> out) {
  CHECK_BF16_2D(a);
  CHECK_BF16_2D(w);
  const int M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "gemm_nt: K mismatch");
  return gemm_launch<false, false>(a, w, bias, epilogue, M, N, K, K, K, out);
}

// C[M,N] = A[M,K] @ B[K,N] — dX = dY @ W without transposing W.
torch::Tensor gemm_nn(torch::Tensor a, torch::Tensor b,
                      c10::optional<torch::Tensor> out) {
  CHECK_BF16_2D(a);
  CHECK_BF16_2D(b);
  const int M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "gemm_nn: K mismatch");
  return gemm_launch<false, true>(a, b, torch::Tensor(), 0, M, N, K, K, N,
                                  out);
}

// C[M,N] = A[K,M]^T @ B[K,N] — dW = dY^T @ X without physical transposes.
torch::Tensor gemm_tn(torch::Tensor a, torch::Tensor b,
                      c10::optional<torch::Tensor> out) {
  CHECK_BF16_2D(a);
  CHECK_BF16_2D(b);
  const int K = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "gemm_tn: contraction mismatch");
  return gemm_launch<true, true>(a, b, torch::Tensor(), 0, M, N, K, M, N,
                                 out);
}

torch::Tensor transpose2d(torch::Tensor a) {
  CHECK_BF16_2D(a);
  int M = a.size(0), N = a.size(1);
  auto out = torch::empty({N, M}, a.options());
  int nb = cdiv(M, 64) * cdiv(N, 64);
  auto stream = at::hip::getCurrentHIPStream();
  transpose2d_kernel<<<nb, 256, 0, stream>>>(
      (const short*)a.data_ptr(), (short*)out.data_ptr(), M, N, M);
  return out;
}

// Transpose into a caller buffer whose rows may be longer than M (pad
// columns untouched) — used for the padded-transposed logits weight that
// feeds the NT dX path when the vocab is not a multiple of 64.
void transpose2d_into(torch::Tensor a, torch::Tensor out) {
  CHECK_BF16_2D(a);
  int M = a.size(0), N = a.size(1);
  TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kBFloat16 &&
              out.dim() == 2 && out.stride(1) == 1 && out.size(0) == N &&
              out.stride(0) >= M, "transpose2d_into: bad out");
  int nb = cdiv(M, 64) * cdiv(N, 64);
  auto stream = at::hip::getCurrentHIPStream();
  transpose2d_kernel<<<nb, 256, 0, stream>>>(
      (const short*)a.data_ptr(), (short*)out.data_ptr(), M, N,
      (long)out.stride(0));
}

// One launch, whole registry: desc built by ops/functional._wt_padded.
void transpose_batch(torch::Tensor desc) {
  TORCH_CHECK(desc.is_cuda() && desc.dtype() == torch::kInt64 &&
              desc.dim() == 2 && desc.size(1) == 7 && desc.is_contiguous(),
              "transpose_batch: bad descriptor table");
  auto stream = at::hip::getCurrentHIPStream();
  transpose_batch_kernel<<<(unsigned)desc.size(0), 256, 0, stream>>>(
      desc.data_ptr<long>());
}

// Cached fp32 workspace (N floats + the arrival counter) per (device, N),
// shared by colsum_kernel and both colsum_rows_kernel forms: each finds
// it zero and leaves it zero.
static float* colsum_ws(const torch::Tensor& like, int N) {
  static std::map<std::pair<int, int>, torch::Tensor> ws_cache;
  auto key = std::make_pair((int)like.get_device(), N);
  auto it = ws_cache.find(key);
  if (it == ws_cache.end())
    it = ws_cache.emplace(key, torch::zeros(
        {N + 1}, like.options().dtype(torch::kFloat32))).first;  // +counter
  return it->second.data_ptr<float>();
}

static torch::Tensor colsum_dest(c10::optional<torch::Tensor>& o,
                                 const torch::Tensor& like, int N) {
  if (!o.has_value()) return torch::empty({N}, like.options());
  TORCH_CHECK(o->is_cuda() && o->dtype() == torch::kBFloat16 &&
              o->is_contiguous() && o->numel() == N, "colsum: bad out");
  return *o;
}

// The row kernel's loads are 16 bytes wide.  TFMX_COLSUM (A/B arms, read
// per call): cols keeps colsum_kernel everywhere, rows takes the row
// kernel wherever its loads are possible.  Unset, a plain colsum narrower
// than one 512-column chunk keeps colsum_kernel: with part of every wave
// idle the row kernel measured no faster there (N = 64 and 192 against
// 512, docs/PERF.md).  relu_bwd_db asks with narrow_ok: its one pass
// replaces two at any width.
static bool colsum_rows_ok(const void* p, long lda, bool narrow_ok) {
  const char* arm = getenv("TFMX_COLSUM");
  if (arm && strcmp(arm, "cols") == 0) return false;
  if (((uintptr_t)p & 15) != 0 || lda % 8 != 0) return false;
  return narrow_ok || (arm && strcmp(arm, "rows") == 0);
}

#define CSR_NW 8  // waves per block of colsum_rows_kernel
// Panels of 1, 2 or 4 chunks (N <= 2048, <= 8192, wider).  Row groups: two
// blocks per CU over all panels, but at least COLSUM_ROWS rows per block,
// so a column never takes more atomics (and their order is never a larger
// share of the rounding) than with colsum_kernel.
template <bool RELU>
static void colsum_rows_launch(const short* dy, const short* y, short* dz,
                               float* acc, short* out, int M, int N,
                               long lda, hipStream_t stream) {
  const int nch = N <= 2048 ? 1 : N <= 8192 ? 2 : 4;
  const int panels = cdiv(N, nch * 512);
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int groups = std::max(1, std::min(cdiv(M, COLSUM_ROWS),
                                          cdiv(2 * cus, panels)));
  dim3 grid(panels, groups);
  auto launch = [&](auto nchc) {
    constexpr int NCH = decltype(nchc)::value;
    colsum_rows_kernel<RELU, NCH, CSR_NW><<<grid, CSR_NW * 64, 0, stream>>>(
        dy, y, dz, acc, out, M, N, lda);
  };
  if (nch == 1) launch(std::integral_constant<int, 1>{});
  else if (nch == 2) launch(std::integral_constant<int, 2>{});
  else launch(std::integral_constant<int, 4>{});
}

torch::Tensor colsum(torch::Tensor a, c10::optional<torch::Tensor> out_opt) {
  TORCH_CHECK(a.is_cuda() && a.dtype() == torch::kBFloat16 && a.dim() == 2 &&
              a.stride(1) == 1, "colsum: bad a");
  int M = a.size(0), N = a.size(1);
  const long lda = a.stride(0);
  float* acc = colsum_ws(a, N);
  torch::Tensor out = colsum_dest(out_opt, a, N);
  auto stream = at::hip::getCurrentHIPStream();
  if (M > 0 && N > 0 && colsum_rows_ok(a.data_ptr(), lda, N >= 512)) {
    colsum_rows_launch<false>((const short*)a.data_ptr(), nullptr, nullptr,
                              acc, (short*)out.data_ptr(), M, N, lda, stream);
    return out;
  }
  dim3 grid(cdiv(N, 256), cdiv(M, COLSUM_ROWS));
  colsum_kernel<<<grid, 256, 0, stream>>>(
      (const short*)a.data_ptr(), acc, (short*)out.data_ptr(), M, N, lda);
  return out;
}

torch::Tensor relu_bwd(torch::Tensor dy, torch::Tensor y);

// (dz, db) = (dy * (y > 0), colsum(dz)): the row kernel writes dz while it
// sums it, so dz is not read back.  Shapes its 16-byte path cannot take
// (N % 8 != 0, misaligned) run relu_bwd + colsum.
std::vector<torch::Tensor> relu_bwd_db(torch::Tensor dy, torch::Tensor y,
                                       c10::optional<torch::Tensor> db_out) {
  TORCH_CHECK(dy.is_cuda() && dy.dtype() == torch::kBFloat16 &&
              dy.dim() == 2 && dy.is_contiguous() && y.is_contiguous() &&
              y.sizes() == dy.sizes(), "relu_bwd_db: bad inputs");
  const int M = dy.size(0), N = dy.size(1);
  if (!(M > 0 && N > 0 && colsum_rows_ok(dy.data_ptr(), N, true) &&
        ((uintptr_t)y.data_ptr() & 15) == 0)) {
    auto dz = relu_bwd(dy, y);
    return {dz, colsum(dz, db_out)};
  }
  auto dz = torch::empty_like(dy);
  torch::Tensor db = colsum_dest(db_out, dy, N);
  colsum_rows_launch<true>(
      (const short*)dy.data_ptr(), (const short*)y.data_ptr(),
      (short*)dz.data_ptr(), colsum_ws(dy, N), (short*)db.data_ptr(), M, N,
      N, at::hip::getCurrentHIPStream());
  return {dz, db};
}

torch::Tensor relu_bwd(torch::Tensor dy, torch::Tensor y) {
  TORCH_CHECK(dy.is_cuda() && dy.dtype() == torch::kBFloat16 &&
              dy.is_contiguous() && y.is_contiguous() &&
              dy.numel() == y.numel());
  auto out = torch::empty_like(dy);
  long n = dy.numel();
  long blocks = ((n + 7) / 8 + 255) / 256;
  auto stream = at::hip::getCurrentHIPStream();
  relu_bwd_kernel<<<blocks, 256, 0, stream>>>(
      (const short*)dy.data_ptr(), (const short*)y.data_ptr(),
      (short*)out.data_ptr(), n);
  return out;
}

torch::Tensor smoke_add(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.is_cuda() && a.dtype() == torch::kBFloat16);
  auto c = torch::empty_like(a);
  long n = a.numel();
  auto stream = at::hip::getCurrentHIPStream();
  smoke_add_kernel<<<(n + 255) / 256, 256, 0, stream>>>(
      (const short*)a.data_ptr(), (const short*)b.data_ptr(),
      (short*)c.data_ptr(), n);
  return c;
}
