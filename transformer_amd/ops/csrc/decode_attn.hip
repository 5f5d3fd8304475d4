// Single-query decode attention: one query row per (batch, head), split-KV
// over the grid, fused KV append, partials combined in the same launch.
//
// Why not MFMA: with one query row per head the matrix instructions have a
// single live M row (63/64 of a 64-row tile is dead work), and the rows of
// different batch entries cannot be batched into one tile because each has
// its own K.  Decode attention is a streaming read of the cache, so the
// scores and PV are VALU fp32 FMAs on bf16 data loaded 16 bytes per lane.
//
// Work split.  grid = (B*H, NSPLIT), 4 waves per block.  NSPLIT is a host
// constant (from Lmax/Sk, B*H and the CU count only: the launch is graph-
// capturable), but the chunk of keys a split owns is derived HERE from the
// row's device-side length, in units of 64 keys, so the work rebalances as
// the sequence grows.  A split past the end owns nothing and contributes an
// empty partial (l = 0).
//
// Lane layout.  LPK = dh/8 lanes form a key group: lane `sub` of a group
// holds columns [8*sub, 8*sub+8) of q (fp32 registers) and loads the same
// columns of K and V, so a wave's load covers 64/LPK whole contiguous
// (H,dh)-rows' worth of this head.  A group dots its 8 elements per lane,
// finishes the dot with log2(LPK) xor-shuffles, and keeps a private online-
// softmax state (m, l, acc[8]) over the keys it visits: nothing crosses
// groups inside the loop.  Afterwards states merge across the groups of a
// wave by xor-shuffles, across waves through LDS, across splits through the
// fp32 workspace.  m, l and acc are fp32 throughout; P is never rounded.
//
// Append (self-attention).  The new key has index n_old = kv_len[b].  The
// one split whose chunk holds that index stores the new K/V row into the
// cache with 16-byte vector stores; whoever attends the new key reads it
// from qkv, never from the cache, so no block reads a location another
// block of the launch writes.  kv_len >= Lmax: nothing is stored, the row
// attends its Lmax cached keys plus the new one.  kv_len is not modified.
//
// Combine.  Each split stores (m, l, acc[dh]) to ws, fences, and takes a
// ticket (one word per (b,h), common.h last_arriver).  The last arriver
// merges the live partials in split order (fixed -> deterministic), stores
// bf16 o and re-zeroes its ticket, so a graph replay needs no memset.
// NSPLIT == 1 touches neither workspace nor ticket.
//
// Workspace: [tickets: B*H words, padded to 4][partials: B*H*NSPLIT*(dh+4)
// floats].  Calls on one stream may share it (they are stream-ordered);
// it must NOT be shared by calls on different streams.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#define DA_WAVES 4
#define DA_THREADS (DA_WAVES * WAVE)
#define DA_ALIGN 64          // chunk granularity in keys
#define DA_MAX_SPLIT 128
#define DA_NEG_BIG (-1e9f)   // additive pad rule of attention.hip
#define DA_M_INIT (-1e30f)   // finite: exp(m - m') never sees inf - inf
#define DA_MAX_BEAM 8

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The acc[8] updates below are the shape the vectorizer turns into packed
// fp32 VALU ops; this file's device code is built without them (plain
// v_fma_f32 / v_mul_f32), whatever the build's global flags are.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// (m, l, acc) <- merge with (m2, l2, a2).  Symmetric in its two states up
// to the commutativity of +, so both partners of an xor-shuffle agree.
DEV_INLINE void da_merge(float& m, float& l, float (&acc)[8], float m2,
                         float l2, const float (&a2)[8]) {
  const float mn = fmaxf(m, m2);
  const float wa = __expf(m - mn), wb = __expf(m2 - mn);
  l = l * wa + l2 * wb;
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = acc[c] * wa + a2[c] * wb;
  m = mn;
}

DEV_INLINE void da_store_o(short* op, float l, const float (&acc)[8]) {
  const float inv = 1.0f / l;
  s16x8 ov;
#pragma unroll
  for (int c = 0; c < 8; ++c) ov[c] = f2bfbits(acc[c] * inv);
  *(s16x8*)op = ov;
}

// SELF: q = qkv (B,1,3,H,dh) contiguous (q_bs = 3*H*dh), kv = cache,
//       L = Lmax, kv_len (B,) int32, pad unused.
// else: q (B,1,H,dh) with batch stride q_bs, kv (B,Sk,2,H,dh), L = Sk,
//       pad (B,Sk) bytes or null.
//
// BEAM (SELF only): b is hypothesis row r of B*K, K rows per sentence, and
// cached key j < n_old is read from row (r/K)*K + min(org[r*Lt + j], K-1) of
// the cache.  The split's 64-key-aligned chunk of the row's table is staged
// in LDS first (16-byte loads, one barrier): measured against one byte load
// per key it is 0.1-0.2 us slower at 64 keys and faster from 256 keys on
// (docs/PERF.md).  The new key and the append are row r's own.
// org, K and Lt are read under BEAM only.
template <int DH, bool SELF, bool BEAM = false>
__global__ __launch_bounds__(DA_THREADS)
void decode_attn_kernel(const short* __restrict__ q, short* kv,
                        const int* __restrict__ kv_len,
                        const unsigned char* __restrict__ pad, float* ws,
                        short* __restrict__ o, int H, int L, float scale,
                        long q_bs, long kv_bs, long kv_rs, long kv_vs,
                        const unsigned char* __restrict__ org, int K, int Lt) {
  constexpr int LPK = DH / 8;            // lanes per key
  constexpr int GPW = WAVE / LPK;        // key groups per wave
  constexpr int KPB = GPW * DA_WAVES;    // keys per block pass
  constexpr int UNR = DH == 32 ? 2 : DH / 32;   // >= 64 keys per iteration
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int split = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int sub = lane % LPK, grp = wave * GPW + lane / LPK;

  int n_old = 0, n = L;
  if constexpr (SELF) {
    n_old = min(max(kv_len[b], 0), L);
    n = n_old + 1;
  }
  const int chunk = cdiv(cdiv(n, nsplit), DA_ALIGN) * DA_ALIGN;
  const int start = min(split * chunk, n);
  const int end = min(start + chunk, n);

  const long hd = (long)H * DH;
  // the new row's K in qkv (V follows at +hd); only dereferenced under SELF
  const short* newk = q + (long)b * q_bs + hd + h * DH;

  if constexpr (SELF) {
    // exactly one split owns key n_old; a full row (n_old == L) stores nothing
    if (n_old < L && split == n_old / chunk && tid < 2 * LPK) {
      const int which = tid / LPK, c8 = (tid % LPK) * 8;
      short* dst = kv + (long)b * kv_bs + (long)n_old * kv_rs +
                   which * kv_vs + h * DH + c8;
      *(s16x8*)dst = *(const s16x8*)(newk + which * hd + c8);
    }
  }

  float qf[8];
  {
    const s16x8 qv = *(const s16x8*)(q + (long)b * q_bs + h * DH + sub * 8);
#pragma unroll
    for (int c = 0; c < 8; ++c) qf[c] = bfbits2f(qv[c]);
  }
  const short* kb = kv + (long)b * kv_bs + h * DH + sub * 8;
  // BEAM: column base of the sentence's first row
  const short* kb0 = kb;
  if constexpr (BEAM) kb0 = kv + (long)(b / K * K) * kv_bs + h * DH + sub * 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_org[];
  if constexpr (BEAM) {
    const unsigned char* orow = org + (long)b * Lt;
    // table bytes [start, min(end, n_old)) in 16-byte vectors: start is a
    // multiple of 64 and the last vector ends by roundup16(n_old) <= Lt
    const int nb = min(end, n_old) - start;
    for (int v = tid * 16; v < nb; v += DA_THREADS * 16)
      *(i32x4*)(s_org + v) = *(const i32x4*)(orow + start + v);
    __syncthreads();
  }

  float m = DA_M_INIT, l = 0.f, acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.f;

  for (int j0 = start + grp; j0 < end; j0 += KPB * UNR) {
    s16x8 kr[UNR], vr[UNR];
    float x[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * KPB;
      const bool live = j < end;
      const int jc = live ? j : j0;      // j0 < end: always a valid key
      const short* kp = kb + (long)jc * kv_rs;
      if constexpr (BEAM) {
        // entries at j >= n_old are never read; the clamp keeps a garbage
        // entry inside the sentence's rows
        const int og = jc < n_old ? min((int)s_org[jc - start], K - 1) : 0;
        kp = kb0 + (long)og * kv_bs + (long)jc * kv_rs;
      }
      const short* vp = kp + kv_vs;
      if (SELF && jc == n_old) {         // the new key: from qkv, not cache
        kp = newk + sub * 8;
        vp = kp + hd;
      }
      kr[u] = *(const s16x8*)kp;
      vr[u] = *(const s16x8*)vp;
      x[u] = live ? 0.f : -INFINITY;
      if (!SELF && pad != nullptr && pad[(long)b * L + jc]) x[u] += DA_NEG_BIG;
    }
    float mn = m;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) s += qf[c] * bfbits2f(kr[u][c]);
#pragma unroll
      for (int off = LPK / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
      x[u] = s * scale + x[u];           // scaled score (+ -1e9 | -inf)
      mn = fmaxf(mn, x[u]);
    }
    const float alpha = __expf(m - mn);
    l *= alpha;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] *= alpha;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const float p = __expf(x[u] - mn);
      l += p;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += p * bfbits2f(vr[u][c]);
    }
    m = mn;
  }

  // groups of a wave -> one state per wave (all lanes end up holding it)
#pragma unroll
  for (int off = LPK; off < WAVE; off <<= 1) {
    float a2[8];
    const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
#pragma unroll
    for (int c = 0; c < 8; ++c) a2[c] = __shfl_xor(acc[c], off);
    da_merge(m, l, acc, m2, l2, a2);
  }

  // waves -> block, in wave order, by the first LPK threads
  __shared__ float s_ml[DA_WAVES][2];
  __shared__ __attribute__((aligned(16))) float s_acc[DA_WAVES][DH];
  if (lane < LPK) {
    if (lane == 0) { s_ml[wave][0] = m; s_ml[wave][1] = l; }
#pragma unroll
    for (int c = 0; c < 8; ++c) s_acc[wave][lane * 8 + c] = acc[c];
  }
  __syncthreads();
  if (tid < LPK) {
#pragma unroll
    for (int w = 1; w < DA_WAVES; ++w) {
      float a2[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) a2[c] = s_acc[w][tid * 8 + c];
      da_merge(m, l, acc, s_ml[w][0], s_ml[w][1], a2);
    }
  }

  short* op = o + (long)bh * DH + tid * 8;   // valid for tid < LPK
  if (nsplit == 1) {
    if (tid < LPK) da_store_o(op, l, acc);
    return;
  }

  constexpr int PS = DH + 4;                 // partial stride in floats
  float* parts = ws + cdiv((int)gridDim.x, 4) * 4 + (long)bh * nsplit * PS;
  if (tid < LPK) {
    float* p = parts + (long)split * PS;
    if (tid == 0) { p[0] = m; p[1] = l; }
    *(f32x4*)(p + 4 + tid * 8) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)(p + 8 + tid * 8) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    __threadfence();   // release the partial to the other XCDs' view
  }
  unsigned* ticket = (unsigned*)ws + bh;
  if (!last_arriver(ticket, nsplit)) return;
  if (tid < LPK) {
    const int nlive = min(nsplit, cdiv(n, chunk));   // >= 1: n >= 1
    m = DA_M_INIT; l = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    for (int s = 0; s < nlive; ++s) {
      const float* p = parts + (long)s * PS;
      const f32x4 lo = *(const f32x4*)(p + 4 + tid * 8);
      const f32x4 hi = *(const f32x4*)(p + 8 + tid * 8);
      const float a2[8] = {lo[0], lo[1], lo[2], lo[3],
                           hi[0], hi[1], hi[2], hi[3]};
      da_merge(m, l, acc, p[0], p[1], a2);
    }
    da_store_o(op, l, acc);
  }
  if (tid == 0)
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Cross-attention for beams: a block owns one (sentence, head) and serves
// the K queries of its hypotheses from ONE pass over the sentence's single
// copy of the encoder K/V.  q (B*K,1,H,dh) with row stride q_bs, kv
// (B,Sk,2,H,dh), pad (B,Sk) or null, o (B*K,1,H,dh) contiguous.
//
// Same lane layout as above (LPK lanes per key, 16-byte loads), but each
// lane holds NQ queries' columns and NQ private (m, l, acc[8]) states: a
// loaded K vector feeds NQ dots, a loaded V vector NQ accumulator updates.
// Queries >= K are dead: their q load is clamped to row K-1 and their state
// is computed like a live one (a branch per query would split the loop body
// into NQ blocks and serialise the queries' dependent chains: dot, shuffles,
// exp) but never merged across waves or stored.
//
// Merge.  Groups of a wave by xor-shuffle per query; every wave then parks
// its NQ states in LDS and thread (query, sub) = (tid / LPK, tid % LPK),
// tid < K*LPK, merges the four in wave order: no register array is indexed
// by a runtime query.  Splits: partials [(b,h)][split][query](m, l, acc[dh])
// behind the tickets, one ticket per (b,h), merged in split order by the
// last arriver, which re-zeroes the ticket.  The ticket region is sized for
// B*K*H words so that the self-attention beam kernel (one ticket per
// (row, h)) can share the workspace.
template <int DH, int NQ>
__global__ __launch_bounds__(DA_THREADS)
void decode_attn_cross_beam_kernel(const short* __restrict__ q,
                                   const short* __restrict__ kv,
                                   const unsigned char* __restrict__ pad,
                                   float* ws, short* __restrict__ o, int H,
                                   int L, int K, float scale, long q_bs,
                                   long kv_bs, long kv_rs, long kv_vs) {
  constexpr int LPK = DH / 8;
  constexpr int GPW = WAVE / LPK;
  constexpr int KPB = GPW * DA_WAVES;
  constexpr int UNR1 = DH == 32 ? 2 : DH / 32;       // the one-query unroll
  constexpr int UNR = NQ <= 4 ? UNR1 : (UNR1 > 1 ? UNR1 / 2 : 1);
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int split = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int sub = lane % LPK, grp = wave * GPW + lane / LPK;

  const int chunk = cdiv(cdiv(L, nsplit), DA_ALIGN) * DA_ALIGN;
  const int start = min(split * chunk, L);
  const int end = min(start + chunk, L);

  float qf[NQ][8], m[NQ], l[NQ], acc[NQ][8];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const long row = (long)b * K + min(i, K - 1);
    const s16x8 qv = *(const s16x8*)(q + row * q_bs + h * DH + sub * 8);
    m[i] = DA_M_INIT; l[i] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) { qf[i][c] = bfbits2f(qv[c]); acc[i][c] = 0.f; }
  }
  const short* kb = kv + (long)b * kv_bs + h * DH + sub * 8;

  for (int j0 = start + grp; j0 < end; j0 += KPB * UNR) {
    s16x8 kr[UNR], vr[UNR];
    float xb[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = j0 + u * KPB;
      const bool live = j < end;
      const int jc = live ? j : j0;      // j0 < end: always a valid key
      const short* kp = kb + (long)jc * kv_rs;
      kr[u] = *(const s16x8*)kp;
      vr[u] = *(const s16x8*)(kp + kv_vs);
      xb[u] = live ? 0.f : -INFINITY;
      if (pad != nullptr && pad[(long)b * L + jc]) xb[u] += DA_NEG_BIG;
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      float x[UNR], mn = m[i];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) s += qf[i][c] * bfbits2f(kr[u][c]);
#pragma unroll
        for (int off = LPK / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
        x[u] = s * scale + xb[u];        // scaled score (+ -1e9 | -inf)
        mn = fmaxf(mn, x[u]);
      }
      const float alpha = __expf(m[i] - mn);
      l[i] *= alpha;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[i][c] *= alpha;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const float p = __expf(x[u] - mn);
        l[i] += p;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] += p * bfbits2f(vr[u][c]);
      }
      m[i] = mn;
    }
  }

  // groups of a wave -> one state per wave and query, parked in LDS
  __shared__ float s_ml[DA_WAVES][NQ][2];
  __shared__ __attribute__((aligned(16))) float s_acc[DA_WAVES][NQ][DH];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
#pragma unroll
    for (int off = LPK; off < WAVE; off <<= 1) {
      float a2[8];
      const float m2 = __shfl_xor(m[i], off), l2 = __shfl_xor(l[i], off);
#pragma unroll
      for (int c = 0; c < 8; ++c) a2[c] = __shfl_xor(acc[i][c], off);
      da_merge(m[i], l[i], acc[i], m2, l2, a2);
    }
    if (lane < LPK) {
      if (lane == 0) { s_ml[wave][i][0] = m[i]; s_ml[wave][i][1] = l[i]; }
#pragma unroll
      for (int c = 0; c < 8; ++c) s_acc[wave][i][lane * 8 + c] = acc[i][c];
    }
  }
  __syncthreads();

  // waves -> block, in wave order, by thread (query mq, columns 8*ms..)
  const int mq = tid / LPK, ms = tid % LPK;
  const bool merger = tid < K * LPK;
  float M = DA_M_INIT, S = 0.f, A[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) A[c] = 0.f;
  if (merger) {
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w) {
      float a2[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) a2[c] = s_acc[w][mq][ms * 8 + c];
      da_merge(M, S, A, s_ml[w][mq][0], s_ml[w][mq][1], a2);
    }
  }

  short* op = o + (((long)b * K + mq) * H + h) * DH + ms * 8;   // if merger
  if (nsplit == 1) {
    if (merger) da_store_o(op, S, A);
    return;
  }

  constexpr int PS = DH + 4;                 // partial stride in floats
  float* parts = ws + cdiv((int)gridDim.x * K, 4) * 4 +
                 (long)bh * nsplit * K * PS + (long)mq * PS;
  if (merger) {
    float* p = parts + (long)split * K * PS;
    if (ms == 0) { p[0] = M; p[1] = S; }
    *(f32x4*)(p + 4 + ms * 8) = f32x4{A[0], A[1], A[2], A[3]};
    *(f32x4*)(p + 8 + ms * 8) = f32x4{A[4], A[5], A[6], A[7]};
    __threadfence();   // release the partial to the other XCDs' view
  }
  unsigned* ticket = (unsigned*)ws + bh;
  if (!last_arriver(ticket, nsplit)) return;
  if (merger) {
    const int nlive = min(nsplit, cdiv(L, chunk));   // >= 1: L >= 1
    M = DA_M_INIT; S = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) A[c] = 0.f;
    for (int s = 0; s < nlive; ++s) {
      const float* p = parts + (long)s * K * PS;
      const f32x4 lo = *(const f32x4*)(p + 4 + ms * 8);
      const f32x4 hi = *(const f32x4*)(p + 8 + ms * 8);
      const float a2[8] = {lo[0], lo[1], lo[2], lo[3],
                           hi[0], hi[1], hi[2], hi[3]};
      da_merge(M, S, A, p[0], p[1], a2);
    }
    da_store_o(op, S, A);
  }
  if (tid == 0)
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---- host wrappers ---------------------------------------------------------

#define DA_DISPATCH_DH(DH_VAL, ...)                                \
  switch (DH_VAL) {                                                \
    case 32: { constexpr int DHC = 32; __VA_ARGS__; break; }       \
    case 64: { constexpr int DHC = 64; __VA_ARGS__; break; }       \
    case 128: { constexpr int DHC = 128; __VA_ARGS__; break; }     \
    default: TORCH_CHECK(false, "decode_attn: head dim must be 32/64/128, got ", DH_VAL); \
  }

// NSPLIT from host-side constants only: about 256 keys per split and one
// block per CU at most.  Measured (tools/decode_attn_bench.py, docs/PERF.md):
// a split costs a partial store, a device-scope fence and a ticket, so the
// first rule tried (64 keys per split, two blocks per CU) lost to fewer
// splits at every shape of the sweep.
static int da_nsplit(int BH, int L) {
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int by_len = (L + 128) / 256, by_cu = std::max(1, cus / BH);
  return std::max(1, std::min(std::min(by_len, by_cu), DA_MAX_SPLIT));
}

static long da_ws_floats(int BH, int DH, int nsplit) {
  return (long)cdiv(BH, 4) * 4 + (long)BH * nsplit * (DH + 4);
}

int64_t decode_attn_nsplit(int64_t BH, int64_t L) {
  TORCH_CHECK(BH > 0 && L > 0, "decode_attn_nsplit: BH and L must be > 0");
  return da_nsplit((int)BH, (int)L);
}

// Tickets (zeroed) + partials for any call with these B, H, dh and a key
// window of at most L.  Allocate ONCE, outside graph capture; share across
// the layers of a step, never across streams.
torch::Tensor decode_attn_workspace(int64_t B, int64_t H, int64_t dh,
                                    int64_t L) {
  TORCH_CHECK(B > 0 && H > 0 && L > 0, "decode_attn_workspace: bad shape");
  const int BH = (int)(B * H);
  return torch::zeros({da_ws_floats(BH, (int)dh, da_nsplit(BH, (int)L))},
                      torch::TensorOptions().dtype(torch::kFloat32)
                          .device(torch::kCUDA, at::cuda::current_device()));
}

// (B,L,2,H,dh) bf16 with contiguous (H,dh) and 16-byte-aligned rows
static void check_da_kv(const torch::Tensor& t, int B, int H, int DH,
                        const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kBFloat16 && t.dim() == 5,
              name, " must be 5-D bf16 on GPU");
  TORCH_CHECK(t.size(0) == B && t.size(2) == 2 && t.size(3) == H &&
              t.size(4) == DH && t.size(1) > 0,
              name, " must be (B,L,2,H,dh) matching the query");
  TORCH_CHECK(t.stride(4) == 1 && t.stride(3) == DH,
              name, " must have contiguous (head, dh) trailing layout");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
              t.stride(2) % 8 == 0 && (uintptr_t)t.data_ptr() % 16 == 0,
              name, " rows must be 16-byte aligned");
}

static int check_da_ws(const torch::Tensor& ws, int BH, int DH, int L,
                       int64_t nsplit_arg) {
  TORCH_CHECK(nsplit_arg >= 0 && nsplit_arg <= DA_MAX_SPLIT,
              "decode_attn: nsplit must be in [0, ", DA_MAX_SPLIT, "]");
  const int nsplit = nsplit_arg ? (int)nsplit_arg : da_nsplit(BH, L);
  if (nsplit > 1) {
    TORCH_CHECK(ws.defined() && ws.is_cuda() &&
                ws.dtype() == torch::kFloat32 && ws.is_contiguous() &&
                (uintptr_t)ws.data_ptr() % 16 == 0,
                "decode_attn: ws must be a contiguous fp32 GPU tensor");
    TORCH_CHECK(ws.numel() >= da_ws_floats(BH, DH, nsplit),
                "decode_attn: ws too small (", ws.numel(), " < ",
                da_ws_floats(BH, DH, nsplit),
                "); allocate it with decode_attn_workspace");
  }
  return nsplit;
}

torch::Tensor decode_attn_self(torch::Tensor qkv, torch::Tensor kv_cache,
                               torch::Tensor kv_len, torch::Tensor ws,
                               double scale, int64_t nsplit_arg) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dtype() == torch::kBFloat16 &&
              qkv.dim() == 5 && qkv.size(1) == 1 && qkv.size(2) == 3 &&
              qkv.is_contiguous() && (uintptr_t)qkv.data_ptr() % 16 == 0,
              "qkv must be contiguous (B,1,3,H,dh) bf16 on GPU");
  const int B = qkv.size(0), H = qkv.size(3), DH = qkv.size(4);
  check_da_kv(kv_cache, B, H, DH, "kv_cache");
  TORCH_CHECK(kv_len.is_cuda() && kv_len.dtype() == torch::kInt32 &&
              kv_len.dim() == 1 && kv_len.size(0) == B &&
              kv_len.is_contiguous(),
              "kv_len must be a contiguous int32 (B,) GPU tensor");
  const int L = kv_cache.size(1);
  const int nsplit = check_da_ws(ws, B * H, DH, L, nsplit_arg);
  auto o = torch::empty({B, 1, H, DH}, qkv.options());
  auto stream = at::hip::getCurrentHIPStream();
  DA_DISPATCH_DH(DH, {
    decode_attn_kernel<DHC, true><<<dim3(B * H, nsplit), DA_THREADS, 0,
                                    stream>>>(
        (const short*)qkv.data_ptr(), (short*)kv_cache.data_ptr(),
        kv_len.data_ptr<int>(), nullptr,
        nsplit > 1 ? ws.data_ptr<float>() : nullptr, (short*)o.data_ptr(), H,
        L, (float)scale, (long)3 * H * DH, kv_cache.stride(0),
        kv_cache.stride(1), kv_cache.stride(2), nullptr, 0, 0);
  });
  return o;
}

torch::Tensor decode_attn_cross(torch::Tensor q, torch::Tensor kv,
                                torch::Tensor kv_pad, torch::Tensor ws,
                                double scale, int64_t nsplit_arg) {
  TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16 && q.dim() == 4 &&
              q.size(1) == 1, "q must be (B,1,H,dh) bf16 on GPU");
  const int B = q.size(0), H = q.size(2), DH = q.size(3);
  TORCH_CHECK(q.stride(3) == 1 && q.stride(2) == DH,
              "q must have contiguous (head, dh) trailing layout");
  TORCH_CHECK(q.stride(0) % 8 == 0 && (uintptr_t)q.data_ptr() % 16 == 0,
              "q rows must be 16-byte aligned");
  check_da_kv(kv, B, H, DH, "kv");
  const int Sk = kv.size(1);
  const unsigned char* pad = nullptr;
  if (kv_pad.defined() && kv_pad.numel() > 0) {
    TORCH_CHECK(kv_pad.is_cuda() && kv_pad.dtype() == torch::kUInt8 &&
                kv_pad.is_contiguous() && kv_pad.dim() == 2 &&
                kv_pad.size(0) == B && kv_pad.size(1) == Sk,
                "kv_pad must be a contiguous uint8 (B,Sk) GPU tensor");
    pad = kv_pad.data_ptr<unsigned char>();
  }
  const int nsplit = check_da_ws(ws, B * H, DH, Sk, nsplit_arg);
  auto o = torch::empty({B, 1, H, DH}, q.options());
  auto stream = at::hip::getCurrentHIPStream();
  DA_DISPATCH_DH(DH, {
    decode_attn_kernel<DHC, false><<<dim3(B * H, nsplit), DA_THREADS, 0,
                                     stream>>>(
        (const short*)q.data_ptr(), (short*)kv.data_ptr(), nullptr, pad,
        nsplit > 1 ? ws.data_ptr<float>() : nullptr, (short*)o.data_ptr(), H,
        Sk, (float)scale, q.stride(0), kv.stride(0), kv.stride(1),
        kv.stride(2), nullptr, 0, 0);
  });
  return o;
}

// ---- beam search: origin-table self-attention, shared-K/V cross-attention --

static long da_beam_ws_floats(int BH, int K, int DH, int nsplit) {
  return (long)cdiv(BH * K, 4) * 4 + (long)BH * K * nsplit * (DH + 4);
}

// One workspace for decode_attn_self_beam (B*K rows, one ticket and NSPLIT
// partials per (row, head)) and decode_attn_cross_beam (one ticket and
// NSPLIT*K partials per (sentence, head)) at key windows up to L: both keep
// B*K*H ticket words in front, so stream-ordered calls may share it.
torch::Tensor decode_attn_beam_workspace(int64_t B, int64_t K, int64_t H,
                                         int64_t dh, int64_t L) {
  TORCH_CHECK(B > 0 && H > 0 && L > 0 && K >= 1 && K <= DA_MAX_BEAM,
              "decode_attn_beam_workspace: bad shape");
  const int BH = (int)(B * H);
  const int ns = std::max(da_nsplit(BH, (int)L), da_nsplit(BH * (int)K, (int)L));
  return torch::zeros({da_beam_ws_floats(BH, (int)K, (int)dh, ns)},
                      torch::TensorOptions().dtype(torch::kFloat32)
                          .device(torch::kCUDA, at::cuda::current_device()));
}

static int check_da_beam_ws(const torch::Tensor& ws, int BH, int K, int DH,
                            int nsplit) {
  if (nsplit > 1) {
    TORCH_CHECK(ws.defined() && ws.is_cuda() &&
                ws.dtype() == torch::kFloat32 && ws.is_contiguous() &&
                (uintptr_t)ws.data_ptr() % 16 == 0,
                "decode_attn: ws must be a contiguous fp32 GPU tensor");
    TORCH_CHECK(ws.numel() >= da_beam_ws_floats(BH, K, DH, nsplit),
                "decode_attn: beam ws too small (", ws.numel(), " < ",
                da_beam_ws_floats(BH, K, DH, nsplit),
                "); allocate it with decode_attn_beam_workspace");
  }
  return nsplit;
}

static int da_pick_nsplit(int BH, int L, int64_t nsplit_arg) {
  TORCH_CHECK(nsplit_arg >= 0 && nsplit_arg <= DA_MAX_SPLIT,
              "decode_attn: nsplit must be in [0, ", DA_MAX_SPLIT, "]");
  return nsplit_arg ? (int)nsplit_arg : da_nsplit(BH, L);
}

// Precondition (device-side, not checked here): the K rows of a sentence
// have equal kv_len.  Then row r writes only position n_old of itself while
// the rows of its sentence read only positions < n_old: no block reads what
// another block of the launch writes.
torch::Tensor decode_attn_self_beam(torch::Tensor qkv, torch::Tensor kv_cache,
                                    torch::Tensor kv_len, torch::Tensor origin,
                                    int64_t K, torch::Tensor ws, double scale,
                                    int64_t nsplit_arg) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dtype() == torch::kBFloat16 &&
              qkv.dim() == 5 && qkv.size(1) == 1 && qkv.size(2) == 3 &&
              qkv.is_contiguous() && (uintptr_t)qkv.data_ptr() % 16 == 0,
              "qkv must be contiguous (B*K,1,3,H,dh) bf16 on GPU");
  const int R = qkv.size(0), H = qkv.size(3), DH = qkv.size(4);
  TORCH_CHECK(K >= 1 && K <= DA_MAX_BEAM && R % K == 0,
              "decode_attn_self_beam: need 1 <= K <= ", DA_MAX_BEAM,
              " and a row count that is a multiple of K");
  check_da_kv(kv_cache, R, H, DH, "kv_cache");
  TORCH_CHECK(kv_len.is_cuda() && kv_len.dtype() == torch::kInt32 &&
              kv_len.dim() == 1 && kv_len.size(0) == R &&
              kv_len.is_contiguous(),
              "kv_len must be a contiguous int32 (B*K,) GPU tensor");
  const int L = kv_cache.size(1);
  TORCH_CHECK(origin.is_cuda() && origin.dtype() == torch::kUInt8 &&
              origin.dim() == 2 && origin.is_contiguous() &&
              origin.size(0) == R && origin.size(1) >= L &&
              origin.size(1) % 16 == 0 &&
              (uintptr_t)origin.data_ptr() % 16 == 0,
              "origin must be a contiguous, 16-byte-aligned uint8 (B*K,Lt) "
              "GPU tensor with Lt >= Lmax and Lt % 16 == 0");
  const int Lt = origin.size(1);
  const int nsplit = da_pick_nsplit(R * H, L, nsplit_arg);
  check_da_beam_ws(ws, R / (int)K * H, (int)K, DH, nsplit);
  auto o = torch::empty({R, 1, H, DH}, qkv.options());
  auto stream = at::hip::getCurrentHIPStream();
  // dynamic LDS: the largest table chunk a split can own, in bytes
  const int smem = cdiv(cdiv(L + 1, nsplit), DA_ALIGN) * DA_ALIGN;
  TORCH_CHECK(smem <= 60 * 1024, "decode_attn_self_beam: ", smem,
              " keys per split exceed the LDS table chunk; raise nsplit");
  DA_DISPATCH_DH(DH, {
    decode_attn_kernel<DHC, true, true><<<dim3(R * H, nsplit), DA_THREADS,
                                          smem, stream>>>(
        (const short*)qkv.data_ptr(), (short*)kv_cache.data_ptr(),
        kv_len.data_ptr<int>(), nullptr,
        nsplit > 1 ? ws.data_ptr<float>() : nullptr, (short*)o.data_ptr(), H,
        L, (float)scale, (long)3 * H * DH, kv_cache.stride(0),
        kv_cache.stride(1), kv_cache.stride(2),
        origin.data_ptr<unsigned char>(), (int)K, Lt);
  });
  return o;
}

#define DA_CROSS_BEAM_LAUNCH(NQ)                                              \
  DA_DISPATCH_DH(DH, {                                                        \
    decode_attn_cross_beam_kernel<DHC, NQ><<<dim3(B * H, nsplit), DA_THREADS, \
                                             0, stream>>>(                    \
        (const short*)q.data_ptr(), (const short*)kv.data_ptr(), pad,         \
        nsplit > 1 ? ws.data_ptr<float>() : nullptr, (short*)o.data_ptr(), H, \
        Sk, (int)K, (float)scale, q.stride(0), kv.stride(0), kv.stride(1),    \
        kv.stride(2));                                                        \
  })

torch::Tensor decode_attn_cross_beam(torch::Tensor q, torch::Tensor kv,
                                     torch::Tensor kv_pad, int64_t K,
                                     torch::Tensor ws, double scale,
                                     int64_t nsplit_arg) {
  TORCH_CHECK(K >= 1 && K <= DA_MAX_BEAM,
              "decode_attn_cross_beam: need 1 <= K <= ", DA_MAX_BEAM);
  if (K == 1) return decode_attn_cross(q, kv, kv_pad, ws, scale, nsplit_arg);
  TORCH_CHECK(q.is_cuda() && q.dtype() == torch::kBFloat16 && q.dim() == 4 &&
              q.size(1) == 1 && q.size(0) % K == 0,
              "q must be (B*K,1,H,dh) bf16 on GPU");
  const int B = q.size(0) / K, H = q.size(2), DH = q.size(3);
  TORCH_CHECK(q.stride(3) == 1 && q.stride(2) == DH,
              "q must have contiguous (head, dh) trailing layout");
  TORCH_CHECK(q.stride(0) % 8 == 0 && (uintptr_t)q.data_ptr() % 16 == 0,
              "q rows must be 16-byte aligned");
  check_da_kv(kv, B, H, DH, "kv");
  const int Sk = kv.size(1);
  const unsigned char* pad = nullptr;
  if (kv_pad.defined() && kv_pad.numel() > 0) {
    TORCH_CHECK(kv_pad.is_cuda() && kv_pad.dtype() == torch::kUInt8 &&
                kv_pad.is_contiguous() && kv_pad.dim() == 2 &&
                kv_pad.size(0) == B && kv_pad.size(1) == Sk,
                "kv_pad must be a contiguous uint8 (B,Sk) GPU tensor");
    pad = kv_pad.data_ptr<unsigned char>();
  }
  const int nsplit = da_pick_nsplit(B * H, Sk, nsplit_arg);
  check_da_beam_ws(ws, B * H, (int)K, DH, nsplit);
  auto o = torch::empty({B * K, 1, H, DH}, q.options());
  auto stream = at::hip::getCurrentHIPStream();
  if (K == 2) { DA_CROSS_BEAM_LAUNCH(2); }
  else if (K <= 4) { DA_CROSS_BEAM_LAUNCH(4); }
  else { DA_CROSS_BEAM_LAUNCH(8); }
  return o;
}
