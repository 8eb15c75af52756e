// Block taps of the fine-tuning path: the final LayerNorm applied to the fp32 residual stream after each of the last n blocks, pooled
// into the clip features of get_intermediate_layers_chunks (ref: audiossl/models/atst/audio_transformer.py:257-366, get_cls_avg) or
// written as dense rows (get_intermediate_layers, :235-255), and its backward with the gradient injected into the residual stream of
// the encoder backward.  Bandwidth-bound: one wave per token row, the LnMap element layout and block-level column sums of layernorm.hip.
#include "common.h"
#include "kernels.h"
#include "profile.h"

namespace {
constexpr float LN_EPS = 1e-6f, LEN_EPS = 1e-6f;

template <int VPT> struct TapMap {
  static constexpr int W = VPT % 4 == 0 ? 4 : 2, CH = VPT / W;
  static DEVFN int col(int chunk, int lane) { return chunk * 64 * W + lane * W; }
};
template <int W> struct FVec;
template <> struct FVec<2> { typedef f32x2 f; typedef bf16x2 h; };
template <> struct FVec<4> { typedef f32x4 f; typedef bf16x4 h; };

// one row's LayerNorm statistics (two-pass, as ln_fwd_kernel): v[] holds the row in LnMap order
template <int VPT> DEVFN void row_stats(const float* v, float& mu, float& rs) {
  constexpr int C = VPT * 64;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) s += v[i];
  mu = wave_sum(s) * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) { const float d = v[i] - mu; q += d * d; }
  rs = rsqrtf(wave_sum(q) * (1.0f / C) + LN_EPS);
}

template <int VPT> DEVFN void load_row(const float* xr, int lane, float* v) {
  using MP = TapMap<VPT>; constexpr int W = MP::W;
  typedef typename FVec<W>::f fvec;
#pragma unroll
  for (int i = 0; i < MP::CH; ++i) {
    const fvec t = *reinterpret_cast<const fvec*>(xr + MP::col(i, lane));
#pragma unroll
    for (int e = 0; e < W; ++e) v[W * i + e] = t[e];
  }
}

// grid (S, n), 256 threads.  Block (s, j): LN of the rows of sequence s in tap j.
//  pooled: feat[s, j C + c] += w_s LN(x_cls) ; feat[s, (n + j) C + c] += w_s sum_{t < np_s} LN(x_t) / (plen_s + 1e-6)  (avgpool)
//  dense:  out[j, s, t, c] = LN(x_t) for t < 1 + n_tok
template <int VPT>
__global__ __launch_bounds__(256) void tap_fwd_kernel(TapFwdArgs p) {
  using MP = TapMap<VPT>; constexpr int C = VPT * 64, W = MP::W;
  typedef typename FVec<W>::f fvec;
  __shared__ float red[4][C];
  const int s = blockIdx.x, j = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float* x = p.x[j] + (size_t)s * p.RS * C;
  const int T1 = p.n_tok + 1;
  const int npatch = min(max(p.plen[s], 0), p.n_tok);
  float wt = 1.f;
  if (!p.dense) {
    wt = p.weight[s];
    if (wt == 0.f) return;                                        // a chunk whose mark is false contributes nothing (no NaN / inf in the taps)
  }
  float gm[VPT], bt[VPT], acc[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) { gm[i] = p.gamma[MP::col(i / W, lane) + i % W]; bt[i] = p.beta[MP::col(i / W, lane) + i % W]; acc[i] = 0.f; }
  const int rows = p.dense ? T1 : (p.avgpool ? 1 + npatch : 1);
  for (int t = wid; t < rows; t += 4) {
    float v[VPT], mu, rs;
    load_row<VPT>(x + (size_t)t * C, lane, v);
    row_stats<VPT>(v, mu, rs);
#pragma unroll
    for (int i = 0; i < VPT; ++i) v[i] = (v[i] - mu) * rs * gm[i] + bt[i];
    if (p.dense) {
      float* yr = p.feat + (((size_t)j * p.S + s) * T1 + t) * C;
#pragma unroll
      for (int i = 0; i < MP::CH; ++i) {
        fvec o;
#pragma unroll
        for (int e = 0; e < W; ++e) o[e] = v[W * i + e];
        *reinterpret_cast<fvec*>(yr + MP::col(i, lane)) = o;
      }
    } else if (t == 0) {                                          // the CLS row: one wave owns this feature slice
      float* fr = p.feat + (size_t)s * p.ldf + (size_t)j * C;
#pragma unroll
      for (int i = 0; i < MP::CH; ++i) {
        fvec o = *reinterpret_cast<const fvec*>(fr + MP::col(i, lane));
#pragma unroll
        for (int e = 0; e < W; ++e) o[e] += wt * v[W * i + e];
        *reinterpret_cast<fvec*>(fr + MP::col(i, lane)) = o;
      }
    } else {
#pragma unroll
      for (int i = 0; i < VPT; ++i) acc[i] += v[i];
    }
  }
  if (p.dense || !p.avgpool) return;
#pragma unroll
  for (int i = 0; i < VPT; ++i) red[wid][MP::col(i / W, lane) + i % W] = acc[i];
  __syncthreads();
  const float sc = wt / ((float)p.plen[s] + LEN_EPS);
  float* fr = p.feat + (size_t)s * p.ldf + (size_t)(p.n + j) * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) fr[c] += sc * (red[0][c] + red[1][c] + red[2][c] + red[3][c]);
}

// Backward of tap j over all M = S RS rows.  dy of a row: pooled -- CLS: dfeat[s, j C:] w_s ; patch t in [1, np_s]: dfeat[s, (n + j) C:] w_s /
// (plen_s + 1e-6) ; else 0 -- or dense dfeat[j, s, t] (t < 1 + n_tok).  dx = LN'(dy) ; cur (+)= dx ; g = bf16(row_scale cur) ;
// column sums of dy x^, dy and row_scale dx into dgamma, dbeta, dbias_up (block reduction + one atomic per column per block, as
// ln_bwd_kernel).  accumulate == 0 (the topmost tap) writes cur and g on every row, rows without a gradient included.
template <int VPT>
__global__ __launch_bounds__(256) void tap_bwd_kernel(TapBwdArgs p) {
  using MP = TapMap<VPT>; constexpr int C = VPT * 64, W = MP::W, CH = MP::CH;
  typedef typename FVec<W>::f fvec; typedef typename FVec<W>::h hvec;
  __shared__ float red[3][4][C];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int T1 = p.n_tok + 1;
  float gm[VPT], dg[VPT], db[VPT], du[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) { gm[i] = p.gamma[MP::col(i / W, lane) + i % W]; dg[i] = db[i] = du[i] = 0.f; }
  for (int row = wave; row < p.M; row += nwaves) {
    const int s = row / p.RS, t = row - s * p.RS;
    const size_t base = (size_t)row * C;
    const float* src = nullptr;
    float a = 1.f;
    if (p.dense) {
      if (t < T1) src = p.dfeat + (((size_t)p.j * p.S + s) * T1 + t) * C;
    } else {
      const float wt = p.weight[s];
      const int pl = p.plen[s], npatch = min(max(pl, 0), p.n_tok);
      if (wt != 0.f) {
        if (t == 0) { src = p.dfeat + (size_t)s * p.ldf + (size_t)p.j * C; a = wt; }
        else if (p.avgpool && t <= npatch) { src = p.dfeat + (size_t)s * p.ldf + (size_t)(p.n + p.j) * C; a = wt / ((float)pl + LEN_EPS); }
      }
    }
    const float sc = p.row_scale ? p.row_scale[row / p.rows_per_seq] : 1.0f;
    if (!src) {
      if (!p.accumulate) {                                        // topmost tap: this row has no gradient at all
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          fvec z; hvec zq;
#pragma unroll
          for (int e = 0; e < W; ++e) { z[e] = 0.f; zq[e] = f2bf(0.f); }
          *reinterpret_cast<fvec*>(p.cur + base + MP::col(i, lane)) = z;
          *reinterpret_cast<hvec*>(p.g + base + MP::col(i, lane)) = zq;
        }
      }
      continue;                                                   // accumulate: cur and g (= bf16(row_scale cur), written by the block above) stand
    }
    float v[VPT], dy[VPT], mu, rs;
    load_row<VPT>(p.x + base, lane, v);
    load_row<VPT>(src, lane, dy);
    row_stats<VPT>(v, mu, rs);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const float d = dy[k] * a;
      v[k] = (v[k] - mu) * rs;                                    // x^
      dy[k] = d * gm[k];                                          // dy gamma
      dg[k] += d * v[k]; db[k] += d;
      s1 += dy[k]; s2 += dy[k] * v[k];
    }
    const float c1 = wave_sum(s1) * (1.0f / C), c2 = wave_sum(s2) * (1.0f / C);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      fvec o; hvec gq;
      fvec rv;
#pragma unroll
      for (int e = 0; e < W; ++e) rv[e] = 0.f;
      if (p.accumulate) rv = *reinterpret_cast<const fvec*>(p.cur + base + MP::col(i, lane));
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const int k = W * i + e;
        const float dx = rs * (dy[k] - c1 - v[k] * c2);
        o[e] = rv[e] + dx;
        gq[e] = f2bf(o[e] * sc);
        du[k] += dx * sc;
      }
      *reinterpret_cast<fvec*>(p.cur + base + MP::col(i, lane)) = o;
      *reinterpret_cast<hvec*>(p.g + base + MP::col(i, lane)) = gq;
    }
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int col = MP::col(i / W, lane) + i % W;
    red[0][wid][col] = dg[i]; red[1][wid][col] = db[i]; red[2][wid][col] = du[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    atomicAdd(p.dgamma + c, red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c]);
    atomicAdd(p.dbeta + c, red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c]);
    atomicAdd(p.dbias_up + c, red[2][0][c] + red[2][1][c] + red[2][2][c] + red[2][3][c]);
  }
}
}  // namespace

int atst_tap_fwd(const TapFwdArgs& a, int C, hipStream_t st) {
  if (a.S <= 0 || a.n <= 0) return ATST_OK;
  if (a.n > TAP_MAX || a.n_tok + 1 > a.RS || (!a.dense && (!a.weight || a.ldf < (a.avgpool ? 2 : 1) * a.n * C))) return ATST_EINVAL;
  ProfScope ps(PK_LN_FWD, (double)a.S * a.n * (a.dense ? a.n_tok + 1 : a.RS) * C * (a.dense ? 8.0 : 4.0), st);
  const dim3 grid(a.S, a.n);
  if (C == 384) hipLaunchKernelGGL(tap_fwd_kernel<6>, grid, dim3(256), 0, st, a);
  else if (C == 768) hipLaunchKernelGGL(tap_fwd_kernel<12>, grid, dim3(256), 0, st, a);
  else return ATST_EINVAL;
  return (int)hipGetLastError();
}

int atst_tap_bwd(const TapBwdArgs& a, int C, hipStream_t st) {
  if (a.M <= 0) return ATST_OK;
  if (a.n_tok + 1 > a.RS || a.M != a.S * a.RS || !a.cur || !a.g || !a.dbias_up || (!a.dense && !a.weight)) return ATST_EINVAL;
  int grid = (a.M + 63) / 64; if (grid > 1024) grid = 1024;
  ProfScope ps(PK_LN_BWD, (double)a.M * C * (4.0 + 4.0 + (a.accumulate ? 4.0 : 0.0) + 4.0 + 2.0), st);
  if (C == 384) hipLaunchKernelGGL(tap_bwd_kernel<6>, dim3(grid), dim3(256), 0, st, a);
  else if (C == 768) hipLaunchKernelGGL(tap_bwd_kernel<12>, dim3(grid), dim3(256), 0, st, a);
  else return ATST_EINVAL;
  return (int)hipGetLastError();
}
