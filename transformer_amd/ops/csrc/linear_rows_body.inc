// The body of linear_rows_kernel and linear_rows_preln_kernel, included
// into each (an inlined function is optimised apart from its kernel's launch
// bounds and does not compile to the same code).  In scope at the include:
// template values MG, NW; constexpr bool LN, PRE; X, W, bias, Y, M, N, K,
// relu, vec, res, gamma, beta, ws, eps; with PRE also XN and tile, where X is
// the pre-norm P and res its residual: the X fragments then come from the
// LDS tile that lr_preln_tile fills.
// vec: N % 4 == 0 and bias/res/y/ws 8-(16-)byte aligned -> vector epilogue.
  constexpr int UNR = lr_unr<MG>();
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int n0 = blockIdx.x * 16;
  const int nrow = n0 + r16;                  // this lane's W row
  const bool wlive = nrow < N;
  const short* wp = W + (long)nrow * K + g * 16;
  const short* xp = X + (long)r16 * K + g * 16;

  f32x4 acc[MG];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) acc[mg] = f32x4{0.f, 0.f, 0.f, 0.f};

  const s16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int nsteps = cdiv(K, 64);
  s16x8 wv0[UNR][2];                          // PRE: W of the first steps
  if constexpr (PRE) {
    // the first W loads do not depend on the prologue: their latency hides
    // under its statistics
    lr_load_w<MG, NW>(wv0, wp, wlive, wave, g, K);
    lr_preln_tile<MG, NW>(X, res, gamma, beta, XN, tile, M, K, eps, wave,
                          lane);
  }
  for (int s0 = wave; s0 < nsteps; s0 += NW * UNR) {
    s16x8 wv[UNR][2], xv[UNR][MG][2];
    if constexpr (PRE) {
      if (s0 != wave) {
        lr_load_w<MG, NW>(wv, wp, wlive, s0, g, K);
      } else {
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
          for (int h = 0; h < 2; ++h) wv[u][h] = wv0[u][h];
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // steps past nsteps start at k >= K: the one test covers both
        const int k = (s0 + u * NW) * 64 + h * 8;    // + g*16 in wp/xp
        const bool kin = k + g * 16 + 8 <= K;
        if constexpr (!PRE)
          wv[u][h] = (kin && wlive) ? *(const s16x8*)(wp + k) : zero8;
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) {
          if constexpr (PRE)     // rows >= M are zeros in the tile
            xv[u][mg][h] =
                kin ? *(const s16x8*)(tile + (mg * 16 + r16) * (K + LR_PRE_PAD) +
                                      g * 16 + k)
                    : zero8;
          else
            xv[u][mg][h] = (kin && mg * 16 + r16 < M)
                               ? *(const s16x8*)(xp + (long)mg * 16 * K + k)
                               : zero8;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
          acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              (bf16x8l)wv[u][h], (bf16x8l)xv[u][mg][h], acc[mg], 0, 0, 0);
  }

  // waves -> block: wave mg sums group mg's partials in wave order
  __shared__ __attribute__((aligned(16))) float s_part[NW][MG][WAVE][4];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) *(f32x4*)s_part[wave][mg][lane] = acc[mg];
  __syncthreads();

  if (wave < MG) {
    const int mg = wave;
    f32x4 v = *(const f32x4*)s_part[0][mg][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += *(const f32x4*)s_part[w][mg][lane];
    const int m = mg * 16 + r16, n = n0 + g * 4;
    if (m < M && n < N) {
      const long o = (long)m * N + n;
      if (vec) {                               // n + 4 <= N: N % 4 == 0
        if (bias != nullptr) {
          const s16x4 bv = *(const s16x4*)(bias + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bfbits2f(bv[r]);
        }
        if constexpr (LN) {
          const s16x4 rv = *(const s16x4*)(res + o);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bfbits2f(rv[r]);
#pragma unroll
          for (int r = 0; r < 4; ++r) lr_ws_store(ws + 4 + o + r, v[r]);
        } else {
          s16x4 ov;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ov[r] = f2bfbits(relu ? fmaxf(v[r], 0.f) : v[r]);
          *(s16x4*)(Y + o) = ov;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (n + r >= N) break;
          float a = v[r];
          if (bias != nullptr) a += bfbits2f(bias[n + r]);
          if constexpr (LN) {
            lr_ws_store(ws + 4 + o + r, a + bfbits2f(res[o + r]));
          } else {
            Y[o + r] = f2bfbits(relu ? fmaxf(a, 0.f) : a);
          }
        }
      }
    }
  }

  if constexpr (LN) {
    // last_arriver drains each wave's write-through stores (vmcnt) before
    // the ticket, and its winner takes an agent acquire before the loads
    unsigned* ticket = (unsigned*)ws;
    if (!last_arriver(ticket, gridDim.x)) return;
    lr_ln_rows<NW>(ws + 4, gamma, beta, Y, M, N, eps, wave, lane);
    if (tid == 0)
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
