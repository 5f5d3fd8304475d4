// Beam-search decoding: candidate selection and KV-cache reorder, one launch
// each per decode step.
//
// beam_topk.  Input: the step's bf16 logits (B*K, V) and the beams' state
// (cumulative log-prob, finished flag, length).  Output: per sentence the K
// best continuations out of K*V by  score[b,k] + log_softmax(logits[b,k])[v],
// best first, ties to the lower flat index k*V + v.  No (B*K, V) log-prob
// tensor exists: within a row the log-softmax shift is one constant, so a
// row's K largest RAW logits are a superset of what the sentence's top K can
// take from that row, and only those K need the shift applied.
//
// Work split.  grid = (nchunk, B*K): a block owns one column chunk (about
// 2048 columns, a host constant from V alone, so the launch is capturable)
// of one row.  The chunk lives in registers: 16-byte vectors on 16-byte
// boundaries of the TENSOR, not of the row.  A row starts at byte 2*V*r,
// which for odd V is only 2-byte aligned, so the first and last vector of a
// chunk are peeled by masking the lanes outside it, and a vector that would
// reach past the end of the tensor is read element by element instead.
// Lane t of slot j holds vector j*256 + t, so a wave's loads are contiguous.
//
// From its registers the block takes the chunk's softmax partial (m, l) in
// fp32 and its K largest logits by K rounds of block arg-max (value, then
// lower column): the round's winner is knocked out of the register that
// holds it.  Round 0's value is the chunk max m.  Partials go to the
// workspace; the block that arrives last at the sentence's ticket
// (common.h last_arriver, K*nchunk arrivals) merges them: per row the
// (m, l) partials in chunk order (fixed, so the result is bit-reproducible),
// then K rounds of the same block arg-max over the at most K*nchunk*K
// candidate scores, keyed (score, lower flat index).  It writes every
// output and re-zeroes its ticket, so a graph replay needs no memset.
//
// Special rows.  A finished row offers exactly one candidate (token 0, its
// score bit-unchanged, its length unchanged) and a dead row (score -inf)
// none; the logits of neither are read.  A sentence with fewer than K
// candidates pads with dead, finished slots (score -inf, parent = slot).
//
// Workspace: [tickets: B words, padded to 4][records: B*K*nchunk of
// {m, l, val[K], col[K]}].  Stream-ordered calls may share it; calls on
// different streams must not.
//
// beam_gather_kv.  dst[l][r, :n] = src[l][src_row[r], :n] for all layers in
// one launch, n = kv_len[src_row[r]] + 1 clamped to Lmax.  In a contiguous
// (rows, Lmax, 2, H, dh) cache the first n positions of a row are ONE
// contiguous span, so the copy is a flat 16-byte stream: grid = (span chunk,
// row, layer), 16 KiB per block, blocks past the row's n exit at once.  The
// layer base pointers come from a device table built once outside capture.
// src and dst are distinct cache sets (the caller swaps them afterwards):
// no block reads what another writes.  O(t) bytes per step by design.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <climits>

#define BS_THREADS 256
#define BS_WAVES (BS_THREADS / WAVE)
#define BS_SLOTS 2                       // 16-byte vectors per thread
#define BS_EPT (8 * BS_SLOTS)            // register-resident logits per thread
#define BS_MAX_CHUNK (BS_THREADS * BS_EPT - 8)   // 8 spare: the peeled head
#define BS_MAX_NCHUNK 64
#define BS_MAX_K 8
#define BS_CPT 16                        // merge candidates per thread
#define BS_M_INIT (-1e30f)               // finite: exp(m - m') never inf - inf
#define BG_UNR 4
#define BG_VECS (BS_THREADS * BG_UNR)    // 16-byte vectors per gather block

typedef int i32x4 __attribute__((ext_vector_type(4)));

// device code without packed fp32 VALU ops, as decode_attn.hip
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

DEV_INLINE bool bs_better(float v, int i, float v2, int i2) {
  return v > v2 || (v == v2 && i < i2);
}

// Block arg-max of (v, i): larger v, then lower i; every thread returns the
// winner.  One barrier per call: consecutive calls alternate `par`, and a
// buffer is rewritten only two calls later, behind the barrier of the call
// in between.
DEV_INLINE void bs_block_argmax(float& v, int& i, float (*s_v)[BS_WAVES],
                                int (*s_i)[BS_WAVES], int par) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float v2 = __shfl_xor(v, off);
    const int i2 = __shfl_xor(i, off);
    if (bs_better(v2, i2, v, i)) { v = v2; i = i2; }
  }
  if ((threadIdx.x & 63) == 0) {
    s_v[par][threadIdx.x >> 6] = v;
    s_i[par][threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = s_v[par][0]; i = s_i[par][0];
#pragma unroll
  for (int w = 1; w < BS_WAVES; ++w)
    if (bs_better(s_v[par][w], s_i[par][w], v, i)) {
      v = s_v[par][w]; i = s_i[par][w];
    }
}

__global__ __launch_bounds__(BS_THREADS)
void beam_topk_kernel(const short* __restrict__ logits,
                      const float* __restrict__ scores,
                      const unsigned char* __restrict__ finished,
                      const int* __restrict__ lens, float* ws,
                      long* __restrict__ next_tok, int* __restrict__ parent,
                      int* __restrict__ src_row, float* __restrict__ scores_o,
                      unsigned char* __restrict__ finished_o,
                      int* __restrict__ lens_o, int nsent, int K, int V,
                      int chunk, long total, int end_id) {
  const int c = blockIdx.x, nchunk = gridDim.x, r = blockIdx.y, b = r / K;
  const int tid = threadIdx.x;
  __shared__ float s_v[2][BS_WAVES];
  __shared__ int s_i[2][BS_WAVES];
  __shared__ float s_sum[BS_WAVES];
  __shared__ float s_lse[BS_MAX_K];

  const int RS = 2 + 2 * K;              // record stride in words
  float* parts = ws + cdiv(nsent, 4) * 4;
  const int c0 = min(c * chunk, V), n = min(chunk, V - c0);
  const float sprev = scores[r];
  const bool live = finished[r] == 0 && sprev > -INFINITY;

  if (live && n > 0) {                   // block-uniform
    const long e0 = (long)r * V + c0;    // element index of the chunk start
    const int a = (int)(e0 & 7);         // elements past a 16-byte boundary
    const long vb0 = e0 - a, e1 = e0 + n;
    float x[BS_EPT];
#pragma unroll
    for (int j = 0; j < BS_SLOTS; ++j) {
      const long ve = vb0 + 8L * (j * BS_THREADS + tid);
#pragma unroll
      for (int i = 0; i < 8; ++i) x[j * 8 + i] = -INFINITY;
      if (ve < e1) {
        if (ve + 8 <= total) {           // whole vector inside the tensor
          const s16x8 raw = *(const s16x8*)(logits + ve);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (ve + i >= e0 && ve + i < e1) x[j * 8 + i] = bfbits2f(raw[i]);
        } else {                         // the tensor's last, partial vector
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (ve + i >= e0 && ve + i < e1)
              x[j * 8 + i] = bfbits2f(logits[ve + i]);
        }
      }
    }
    // column of x[j*8 + i] is colbase + j*8*BS_THREADS + i
    const int colbase = c0 - a + 8 * tid;
    float* rec = parts + ((long)r * nchunk + c) * RS;
    float m = 0.f;
    for (int round = 0; round < K; ++round) {
      float bv = -INFINITY;
      int bi = INT_MAX;
#pragma unroll
      for (int e = 0; e < BS_EPT; ++e)   // ascending column: > keeps the lower
        if (x[e] > bv) {
          bv = x[e];
          bi = colbase + (e / 8) * 8 * BS_THREADS + (e % 8);
        }
      bs_block_argmax(bv, bi, s_v, s_i, round & 1);
      if (round == 0) {
        // the first winner's value is the chunk max: take (m, l) now, while
        // every element is still in place
        m = fmaxf(bv, BS_M_INIT);
        float l = 0.f;
#pragma unroll
        for (int e = 0; e < BS_EPT; ++e) l += expf(x[e] - m);
        l = wave_sum(l);
        if ((tid & 63) == 0) s_sum[tid >> 6] = l;
        __syncthreads();
        if (tid == 0) {
          rec[0] = m;
          rec[1] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        }
      }
#pragma unroll
      for (int e = 0; e < BS_EPT; ++e)
        if (colbase + (e / 8) * 8 * BS_THREADS + (e % 8) == bi)
          x[e] = -INFINITY;
      if (tid == 0) {
        rec[2 + round] = bv;
        ((int*)rec)[2 + K + round] = bv > -INFINITY ? bi : -1;
      }
    }
    if (tid == 0) __threadfence();       // release the record to other XCDs
  }

  unsigned* ticket = (unsigned*)ws + b;
  if (!last_arriver(ticket, (unsigned)(K * nchunk))) return;

  // ---- merge for sentence b -------------------------------------------------
  const int nlive = min(nchunk, cdiv(V, chunk));   // chunks that hold columns
  if (tid < K) {
    const int row = b * K + tid;
    float lse = 0.f;
    if (finished[row] == 0 && scores[row] > -INFINITY) {
      float M = BS_M_INIT, L = 0.f;
      for (int cc = 0; cc < nlive; ++cc) {         // chunk order: fixed
        const float* p = parts + ((long)row * nchunk + cc) * RS;
        const float mn = fmaxf(M, p[0]);
        L = L * expf(M - mn) + p[1] * expf(p[0] - mn);
        M = mn;
      }
      lse = M + logf(L);
    }
    s_lse[tid] = lse;
  }
  __syncthreads();

  const int NC = K * nchunk * K;         // <= BS_THREADS * BS_CPT (host check)
  float cs[BS_CPT];
  int cf[BS_CPT];
#pragma unroll
  for (int u = 0; u < BS_CPT; ++u) {
    const int ci = tid + BS_THREADS * u;
    cs[u] = -INFINITY;
    cf[u] = INT_MAX;
    if (ci < NC) {
      const int j = ci % K, cc = (ci / K) % nchunk, kk = ci / (K * nchunk);
      const int row = b * K + kk;
      const float sp = scores[row];
      if (finished[row] != 0) {
        if (cc == 0 && j == 0 && sp > -INFINITY) { cs[u] = sp; cf[u] = kk * V; }
      } else if (sp > -INFINITY && cc < nlive) {
        const float* p = parts + ((long)row * nchunk + cc) * RS;
        const int col = ((const int*)p)[2 + K + j];
        if (col >= 0) {
          cs[u] = sp + (p[2 + j] - s_lse[kk]);
          cf[u] = kk * V + col;
        }
      }
    }
  }
  for (int slot = 0; slot < K; ++slot) {
    float bv = -INFINITY;
    int bf = INT_MAX;
#pragma unroll
    for (int u = 0; u < BS_CPT; ++u)
      if (bs_better(cs[u], cf[u], bv, bf)) { bv = cs[u]; bf = cf[u]; }
    bs_block_argmax(bv, bf, s_v, s_i, slot & 1);
#pragma unroll
    for (int u = 0; u < BS_CPT; ++u)
      if (cf[u] == bf) { cs[u] = -INFINITY; cf[u] = INT_MAX; }
    if (tid == 0) {
      const int o = b * K + slot;
      if (bv > -INFINITY) {
        const int kk = bf / V, col = bf % V, prow = b * K + kk;
        const bool fin = finished[prow] != 0;
        next_tok[o] = col;
        parent[o] = kk;
        src_row[o] = prow;
        scores_o[o] = bv;
        finished_o[o] = (fin || col == end_id) ? 1 : 0;
        lens_o[o] = lens[prow] + (fin ? 0 : 1);
      } else {                           // fewer than K candidates: dead slot
        next_tok[o] = 0;
        parent[o] = slot;
        src_row[o] = o;
        scores_o[o] = -INFINITY;
        finished_o[o] = 1;
        lens_o[o] = lens[o];
      }
    }
  }
  if (tid == 0)
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// table: [src layer bases: NL][dst layer bases: NL]; pos_vecs / row_vecs:
// 16-byte vectors per cache position / per cache row.
__global__ __launch_bounds__(BS_THREADS)
void beam_gather_kv_kernel(const long* __restrict__ table,
                           const int* __restrict__ src_row,
                           const int* __restrict__ kv_len, int rows, int Lmax,
                           int pos_vecs, long row_vecs, int NL) {
  const int r = blockIdx.y, l = blockIdx.z, tid = threadIdx.x;
  const int sr = src_row[r];
  if (sr < 0 || sr >= rows) return;
  const int n = min(max(kv_len[sr], 0), Lmax - 1) + 1;
  const long nv = (long)n * pos_vecs;
  const long v0 = (long)blockIdx.x * BG_VECS + tid;
  if (v0 - tid >= nv) return;
  const i32x4* s = (const i32x4*)table[l] + (long)sr * row_vecs;
  i32x4* d = (i32x4*)table[NL + l] + (long)r * row_vecs;
  i32x4 t[BG_UNR];
#pragma unroll
  for (int u = 0; u < BG_UNR; ++u) {
    const long v = v0 + u * BS_THREADS;
    if (v < nv) t[u] = s[v];
  }
#pragma unroll
  for (int u = 0; u < BG_UNR; ++u) {
    const long v = v0 + u * BS_THREADS;
    if (v < nv) d[v] = t[u];
  }
}

// The reorder when self-attention reads through an origin table
// (decode_attn.hip, BEAM): out[r, :n] = in[src_row[r], :n], n =
// kv_before[src_row[r]] clamped to [0, Lmax], and, unless the row is full,
// out[r, n] = src_row[r] % K: the position the step just appended sits in
// the parent's physical row.  One byte per cached position: the span of a
// row is a flat 16-byte stream with a byte tail.  grid = (span chunk, row),
// 4 KiB of table per block; the block that owns byte n writes the entry.
// Bytes past the written span are not touched.
__global__ __launch_bounds__(BS_THREADS)
void beam_reindex_kernel(const unsigned char* __restrict__ in,
                         unsigned char* __restrict__ out,
                         const int* __restrict__ src_row,
                         const int* __restrict__ kv_before, int rows, int K,
                         int Lmax, int Lt) {
  const int r = blockIdx.y, tid = threadIdx.x;
  const int sr = src_row[r];
  if (sr < 0 || sr >= rows) return;
  const int n = min(max(kv_before[sr], 0), Lmax);
  const int c0 = blockIdx.x * (BS_THREADS * 16);   // this block's first byte
  if (c0 > n) return;
  const unsigned char* s = in + (long)sr * Lt;
  unsigned char* d = out + (long)r * Lt;
  const int p = c0 + tid * 16;
  if (p + 16 <= n) {
    *(i32x4*)(d + p) = *(const i32x4*)(s + p);
  } else {
    for (int i = p; i < n; ++i) d[i] = s[i];       // the tail: < 16 bytes
  }
  if (n < Lmax && n >= p && n < p + 16) d[n] = (unsigned char)(sr % K);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---- host wrappers ---------------------------------------------------------

// about 2048 columns per chunk, from V alone
static int bs_nchunk(int V) {
  return std::max(1, std::min((V + 1024) / 2048, BS_MAX_NCHUNK));
}

static int bs_chunk(int V, int nchunk) {
  return cdiv(cdiv(V, nchunk), 8) * 8;
}

static long bs_ws_floats(int B, int K, int nchunk) {
  return (long)cdiv(B, 4) * 4 + (long)B * K * nchunk * (2 + 2 * K);
}

static int bs_check_shape(int64_t B, int64_t K, int64_t V, int64_t nchunk_arg) {
  TORCH_CHECK(B > 0 && K >= 1 && K <= BS_MAX_K && V >= 1,
              "beam_topk: need B > 0, 1 <= K <= ", BS_MAX_K, ", V >= 1");
  TORCH_CHECK(B * K <= 65535, "beam_topk: B*K must be <= 65535");
  TORCH_CHECK(K * V < (int64_t)INT_MAX, "beam_topk: K*V must fit in int32");
  TORCH_CHECK(nchunk_arg >= 0 && nchunk_arg <= BS_MAX_NCHUNK,
              "beam_topk: nchunk must be in [0, ", BS_MAX_NCHUNK, "]");
  const int nchunk = nchunk_arg ? (int)nchunk_arg : bs_nchunk((int)V);
  TORCH_CHECK(bs_chunk((int)V, nchunk) <= BS_MAX_CHUNK,
              "beam_topk: V = ", V, " in ", nchunk, " chunks exceeds ",
              BS_MAX_CHUNK, " columns per chunk");
  TORCH_CHECK(K * nchunk * K <= BS_THREADS * BS_CPT,
              "beam_topk: K*nchunk*K must be <= ", BS_THREADS * BS_CPT);
  return nchunk;
}

// Zeroed tickets + records for beam_topk at these B, K, V (nchunk 0 = the
// host rule).  Allocate ONCE, outside graph capture.
torch::Tensor beam_search_workspace(int64_t B, int64_t K, int64_t V,
                                    int64_t nchunk_arg) {
  const int nchunk = bs_check_shape(B, K, V, nchunk_arg);
  return torch::zeros({bs_ws_floats((int)B, (int)K, nchunk)},
                      torch::TensorOptions().dtype(torch::kFloat32)
                          .device(torch::kCUDA, at::cuda::current_device()));
}

std::vector<torch::Tensor> beam_topk(torch::Tensor logits,
                                     torch::Tensor scores,
                                     torch::Tensor finished,
                                     torch::Tensor lens, int64_t end_id,
                                     torch::Tensor ws, int64_t nchunk_arg) {
  TORCH_CHECK(scores.is_cuda() && scores.dtype() == torch::kFloat32 &&
              scores.dim() == 2 && scores.is_contiguous(),
              "scores must be a contiguous fp32 (B,K) GPU tensor");
  const int64_t B = scores.size(0), K = scores.size(1);
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kBFloat16 &&
              logits.dim() == 2 && logits.size(0) == B * K &&
              logits.is_contiguous() &&
              (uintptr_t)logits.data_ptr() % 16 == 0,
              "logits must be a contiguous, 16-byte-aligned bf16 (B*K,V) "
              "GPU tensor");
  const int64_t V = logits.size(1);
  TORCH_CHECK(finished.is_cuda() && finished.dtype() == torch::kUInt8 &&
              finished.is_contiguous() && finished.sizes() == scores.sizes(),
              "finished must be a contiguous uint8 (B,K) GPU tensor");
  TORCH_CHECK(lens.is_cuda() && lens.dtype() == torch::kInt32 &&
              lens.is_contiguous() && lens.sizes() == scores.sizes(),
              "lens must be a contiguous int32 (B,K) GPU tensor");
  const int nchunk = bs_check_shape(B, K, V, nchunk_arg);
  TORCH_CHECK(ws.defined() && ws.is_cuda() && ws.dtype() == torch::kFloat32 &&
              ws.is_contiguous() && (uintptr_t)ws.data_ptr() % 16 == 0,
              "beam_topk: ws must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(ws.numel() >= bs_ws_floats((int)B, (int)K, nchunk),
              "beam_topk: ws too small (", ws.numel(), " < ",
              bs_ws_floats((int)B, (int)K, nchunk),
              "); allocate it with beam_search_workspace");
  auto i32 = scores.options().dtype(torch::kInt32);
  auto next_tok = torch::empty({B * K, 1}, i32.dtype(torch::kInt64));
  auto parent = torch::empty({B, K}, i32);
  auto src_row = torch::empty({B * K}, i32);
  auto scores_o = torch::empty_like(scores);
  auto finished_o = torch::empty_like(finished);
  auto lens_o = torch::empty_like(lens);
  auto stream = at::hip::getCurrentHIPStream();
  beam_topk_kernel<<<dim3(nchunk, (unsigned)(B * K)), BS_THREADS, 0, stream>>>(
      (const short*)logits.data_ptr(), scores.data_ptr<float>(),
      finished.data_ptr<unsigned char>(), lens.data_ptr<int>(),
      ws.data_ptr<float>(), (long*)next_tok.data_ptr<int64_t>(),
      parent.data_ptr<int>(), src_row.data_ptr<int>(),
      scores_o.data_ptr<float>(), finished_o.data_ptr<unsigned char>(),
      lens_o.data_ptr<int>(), (int)B, (int)K, (int)V,
      bs_chunk((int)V, nchunk), (long)(B * K * V), (int)end_id);
  return {next_tok, parent, src_row, scores_o, finished_o, lens_o};
}

// every layer of both sets: one (rows,Lmax,2,H,dh) bf16 shape, contiguous,
// 16-byte aligned, and no dst layer overlapping any src layer
static void bg_check_sets(const std::vector<torch::Tensor>& src,
                          const std::vector<torch::Tensor>& dst) {
  TORCH_CHECK(!src.empty() && src.size() == dst.size() && src.size() <= 65535,
              "beam_gather_kv: src and dst need the same layer count (>= 1)");
  const auto& s0 = src[0];
  TORCH_CHECK(s0.dim() == 5 && s0.size(2) == 2 &&
              (s0.size(3) * s0.size(4)) % 4 == 0 && s0.size(0) <= 65535,
              "beam_gather_kv: caches must be (rows,Lmax,2,H,dh) with "
              "16-byte positions");
  for (const auto* set : {&src, &dst})
    for (const auto& t : *set)
      TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kBFloat16 &&
                  t.is_contiguous() && t.sizes() == s0.sizes() &&
                  (uintptr_t)t.data_ptr() % 16 == 0,
                  "beam_gather_kv: every cache must be a contiguous, "
                  "16-byte-aligned bf16 GPU tensor of one shape");
  const uintptr_t bytes = (uintptr_t)s0.numel() * 2;
  for (const auto& s : src)
    for (const auto& d : dst) {
      const uintptr_t ps = (uintptr_t)s.data_ptr();
      const uintptr_t pd = (uintptr_t)d.data_ptr();
      TORCH_CHECK(ps + bytes <= pd || pd + bytes <= ps,
                  "beam_gather_kv: src and dst must be distinct cache sets "
                  "(the reorder is never in place)");
    }
}

// The device table of layer base pointers for one (src, dst) direction.
// Build ONCE, outside graph capture (it involves a host-to-device copy).
torch::Tensor beam_gather_table(std::vector<torch::Tensor> src,
                                std::vector<torch::Tensor> dst) {
  bg_check_sets(src, dst);
  const int64_t NL = (int64_t)src.size();
  auto host = torch::empty({2 * NL}, torch::kInt64);
  int64_t* h = host.data_ptr<int64_t>();
  for (int64_t l = 0; l < NL; ++l) {
    h[l] = (int64_t)(uintptr_t)src[l].data_ptr();
    h[NL + l] = (int64_t)(uintptr_t)dst[l].data_ptr();
  }
  return host.to(src[0].device());
}

void beam_gather_kv(std::vector<torch::Tensor> src,
                    std::vector<torch::Tensor> dst, torch::Tensor table,
                    torch::Tensor src_row, torch::Tensor kv_len) {
  bg_check_sets(src, dst);
  const int64_t NL = (int64_t)src.size();
  const int64_t rows = src[0].size(0), Lmax = src[0].size(1);
  TORCH_CHECK(table.is_cuda() && table.dtype() == torch::kInt64 &&
              table.is_contiguous() && table.numel() == 2 * NL,
              "beam_gather_kv: table must come from beam_gather_table for "
              "these cache sets");
  TORCH_CHECK(src_row.is_cuda() && src_row.dtype() == torch::kInt32 &&
              src_row.is_contiguous() && src_row.dim() == 1 &&
              src_row.size(0) == rows,
              "src_row must be a contiguous int32 (rows,) GPU tensor");
  TORCH_CHECK(kv_len.is_cuda() && kv_len.dtype() == torch::kInt32 &&
              kv_len.is_contiguous() && kv_len.dim() == 1 &&
              kv_len.size(0) == rows,
              "kv_len must be a contiguous int32 (rows,) GPU tensor");
  if (rows == 0 || Lmax == 0) return;
  const int pos_vecs = (int)(2 * src[0].size(3) * src[0].size(4) / 8);
  const long row_vecs = (long)Lmax * pos_vecs;
  const long gx = (row_vecs + BG_VECS - 1) / BG_VECS;
  TORCH_CHECK(gx <= INT_MAX, "beam_gather_kv: cache row too large");
  auto stream = at::hip::getCurrentHIPStream();
  beam_gather_kv_kernel<<<dim3((unsigned)gx, (unsigned)rows, (unsigned)NL),
                          BS_THREADS, 0, stream>>>(
      (const long*)table.data_ptr<int64_t>(), src_row.data_ptr<int>(),
      kv_len.data_ptr<int>(), (int)rows, (int)Lmax, pos_vecs, row_vecs,
      (int)NL);
}

void beam_reindex(torch::Tensor origin_in, torch::Tensor origin_out,
                  torch::Tensor src_row, torch::Tensor kv_before, int64_t K,
                  int64_t Lmax) {
  TORCH_CHECK(K >= 1 && K <= BS_MAX_K, "beam_reindex: need 1 <= K <= ",
              BS_MAX_K);
  for (const auto* t : {&origin_in, &origin_out})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kUInt8 && t->dim() == 2 &&
                t->is_contiguous() && t->sizes() == origin_in.sizes() &&
                t->size(1) % 16 == 0 && (uintptr_t)t->data_ptr() % 16 == 0,
                "beam_reindex: tables must be contiguous, 16-byte-aligned "
                "uint8 (rows,Lt) GPU tensors of one shape, Lt % 16 == 0");
  const int64_t rows = origin_in.size(0), Lt = origin_in.size(1);
  const uintptr_t pi = (uintptr_t)origin_in.data_ptr();
  const uintptr_t po = (uintptr_t)origin_out.data_ptr();
  const uintptr_t bytes = (uintptr_t)(rows * Lt);
  TORCH_CHECK(pi + bytes <= po || po + bytes <= pi,
              "beam_reindex: origin_in and origin_out must be distinct tables "
              "(the reorder is never in place)");
  TORCH_CHECK(Lmax >= 1 && Lmax <= Lt && rows % K == 0 && rows <= 65535,
              "beam_reindex: need 1 <= Lmax <= Lt and rows = B*K <= 65535");
  for (const auto* t : {&src_row, &kv_before})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kInt32 &&
                t->is_contiguous() && t->dim() == 1 && t->size(0) == rows,
                "beam_reindex: src_row and kv_before must be contiguous int32 "
                "(rows,) GPU tensors");
  if (rows == 0) return;
  const unsigned gx = (unsigned)cdiv((int)Lmax, BS_THREADS * 16);
  auto stream = at::hip::getCurrentHIPStream();
  beam_reindex_kernel<<<dim3(gx, (unsigned)rows), BS_THREADS, 0, stream>>>(
      origin_in.data_ptr<unsigned char>(),
      origin_out.data_ptr<unsigned char>(), src_row.data_ptr<int>(),
      kv_before.data_ptr<int>(), (int)rows, (int)K, (int)Lmax, (int)Lt);
}
