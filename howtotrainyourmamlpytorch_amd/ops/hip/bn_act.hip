// Fused task-batched BatchNorm (batch statistics, training semantics) +
// leaky-ReLU for NHWC-task-batched activations x[T, M, C] (M = NS*H*W).
//
// Replaces the reference's F.batch_norm + F.leaky_relu pair
// (meta_neural_network_architectures.py:244-247, :383) — and, because the
// whole task batch is processed at once, T x 2 ATen launches collapse into
// 3 kernels (partial sums -> finalize -> normalize+act).
//
// Per-(task, channel) statistics: mean/var over the M image positions of
// each task — matching the reference's per-task BN exactly.

#include "common.h"

using namespace maml355;

// Partial sums land in partials[T, NBLK, 2, C] (one private slice per
// block — NO global atomics) and are reduced over NBLK in fixed order by
// bn_reduce2_kernel / bn_finalize_partials_kernel.  This makes every BN
// reduction bitwise run-to-run deterministic and removes
// the global-atomic contention of the round-1 kernels.
template <typename scalar_t>
__global__ void bn_sums_vec_kernel(const scalar_t* __restrict__ x,
                                   float* __restrict__ partials,  // [T,NBLK,2,C]
                                   int T, long M, int C, int rows_per_block) {
  const int c8n = C / 8;
  const int rows_in_block = blockDim.x / c8n;
  const int c8 = threadIdx.x % c8n;
  const int rg = threadIdx.x / c8n;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  extern __shared__ float ls[];  // [rows_in_block][2][C] per-thread slices
  float s[8] = {0}, q[8] = {0};
  if (rg < rows_in_block) {
    const scalar_t* xt = x + (long)t * M * C + c8 * 8;
    const long row_end = min(row0 + rows_per_block, M);
    for (long m = row0 + rg; m < row_end; m += rows_in_block) {
      float v[8];
      load8(xt + m * C, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) { s[j] += v[j]; q[j] += v[j] * v[j]; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ls[(rg * 2 + 0) * C + c8 * 8 + j] = s[j];
      ls[(rg * 2 + 1) * C + c8 * 8 + j] = q[j];
    }
  }
  __syncthreads();
  // in-block pairwise tree reduce with FIXED pairing order (bitwise
  // deterministic, log2(rows) steps instead of a serial row loop)
  for (int n_ = rows_in_block; n_ > 1;) {
    const int step = (n_ + 1) >> 1;   // non-pow2-safe fixed pairing
    if (rg < step && rg + step < n_) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ls[(rg * 2 + 0) * C + c8 * 8 + j] +=
            ls[((rg + step) * 2 + 0) * C + c8 * 8 + j];
        ls[(rg * 2 + 1) * C + c8 * 8 + j] +=
            ls[((rg + step) * 2 + 1) * C + c8 * 8 + j];
      }
    }
    __syncthreads();
    n_ = step;
  }
  if (rg == 0) {
    float* pt = partials + (((long)t * gridDim.y + blockIdx.y) * 2) * C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pt[c8 * 8 + j] = ls[0 * C + c8 * 8 + j];
      pt[C + c8 * 8 + j] = ls[1 * C + c8 * 8 + j];
    }
  }
}

// ordered reduction of partials[T, NBLK, 2, C] -> sums[T, 2, C].  The
// loads of kAhead2 blocks are issued together and then added in ascending
// block order: still one serial chain of additions per (t, c), so the bits
// are those of the one-load-one-add loop; only the load latency overlaps.
// out0 / out1 ([T, C], may be null) receive the two rows as tensors of
// their own (the backward's dbeta_t / dgamma_t).
constexpr int kAhead2 = 16;
__global__ void bn_reduce2_kernel(const float* __restrict__ partials,
                                  float* __restrict__ sums, int T, int nblk,
                                  int C, float* __restrict__ out0,
                                  float* __restrict__ out1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * C) return;
  const int t = i / C, c = i % C;
  float s = 0.f, q = 0.f;
  for (int b0 = 0; b0 < nblk; b0 += kAhead2) {
    float vs[kAhead2], vq[kAhead2];
#pragma unroll
    for (int a = 0; a < kAhead2; ++a) {
      if (b0 + a < nblk) {
        const float* p = partials + (((long)t * nblk + b0 + a) * 2) * C;
        vs[a] = p[c];
        vq[a] = p[C + c];
      }
    }
#pragma unroll
    for (int a = 0; a < kAhead2; ++a) {
      if (b0 + a < nblk) {
        s += vs[a];
        q += vq[a];
      }
    }
  }
  sums[((long)t * 2 + 0) * C + c] = s;
  sums[((long)t * 2 + 1) * C + c] = q;
  if (out0 != nullptr) out0[i] = s;
  if (out1 != nullptr) out1[i] = q;
}

template <typename scalar_t, bool PER_TASK_AFFINE, bool ACT>
__global__ void bn_norm_act_vec_kernel(const scalar_t* __restrict__ x,
                                       scalar_t* __restrict__ y,
                                       const float* __restrict__ mean,
                                       const float* __restrict__ rstd,
                                       const float* __restrict__ gamma,
                                       const float* __restrict__ beta,
                                       int T, long M, int C, float slope,
                                       int rows_per_block) {
  const int c8n = C / 8;
  const int rows_in_block = blockDim.x / c8n;
  const int c8 = threadIdx.x % c8n;
  const int rg = threadIdx.x / c8n;
  if (rg >= rows_in_block) return;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  float mu[8], r[8], g[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c8 * 8 + j;
    const long tc = (long)t * C + c;
    mu[j] = mean[tc];
    r[j] = rstd[tc];
    g[j] = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
    b[j] = PER_TASK_AFFINE ? beta[tc] : beta[c];
  }
  const scalar_t* xt = x + (long)t * M * C + c8 * 8;
  scalar_t* yt = y + (long)t * M * C + c8 * 8;
  const long row_end = min(row0 + rows_per_block, M);
  for (long m = row0 + rg; m < row_end; m += rows_in_block) {
    float v[8];
    load8(xt + m * C, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float o = (v[j] - mu[j]) * r[j] * g[j] + b[j];
      if (ACT) o = o > 0.f ? o : o * slope;
      v[j] = o;
    }
    store8(yt + m * C, v);
  }
}

// Fused normalize + leaky-ReLU + 2x2/s2 maxpool (forward only; the
// backward composes the existing pool-bwd and BN-bwd Functions).  One
// thread per (pooled position, 8-channel group): reads the 2x2 window of
// conv output, normalizes all four, maxes, emits pooled value + argmax
// mask.  Saves a full activation-tensor write+read per conv block.
template <typename scalar_t, bool PER_TASK_AFFINE>
__global__ void bn_norm_act_pool_vec_kernel(
    const scalar_t* __restrict__ x,   // [T, NB, H, W, C]
    scalar_t* __restrict__ y,         // [T, NB, Ho, Wo, C]
    unsigned char* __restrict__ mask, // [T, NB, Ho, Wo, C]
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    int T, int NB, int H, int W, int C, int Ho, int Wo, float slope) {
  const int c8n = C / 8;
  const long total = (long)T * NB * Ho * Wo * c8n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int c8 = (int)(i % c8n);
    long r = i / c8n;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho); r /= Ho;
    const int nb = (int)(r % NB);
    const int t = (int)(r / NB);
    const int c0 = c8 * 8;
    float mu[8], rs[8], g[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long tc = (long)t * C + c0 + j;
      mu[j] = mean[tc];
      rs[j] = rstd[tc];
      g[j] = PER_TASK_AFFINE ? gamma[tc] : gamma[c0 + j];
      b[j] = PER_TASK_AFFINE ? beta[tc] : beta[c0 + j];
    }
    const long base =
        ((((long)t * NB + nb) * H + 2 * ho) * W + 2 * wo) * C + c0;
    float v[4][8];
    load8(&x[base], v[0]);
    load8(&x[base + C], v[1]);
    load8(&x[base + (long)W * C], v[2]);
    load8(&x[base + (long)W * C + C], v[3]);
    unsigned long long mpack = 0;
    float out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float best = -INFINITY;
      int arg = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a = (v[q][j] - mu[j]) * rs[j] * g[j] + b[j];
        a = a > 0.f ? a : a * slope;
        if (a > best) { best = a; arg = q; }
      }
      out[j] = best;
      mpack |= ((unsigned long long)arg) << (8 * j);
    }
    const long o = ((((long)t * NB + nb) * Ho + ho) * Wo + wo) * C + c0;
    store8(&y[o], out);
    *(unsigned long long*)&mask[o] = mpack;
  }
}

// deterministic in-block + cross-block reduction (see bn_sums_vec_kernel)
template <typename scalar_t, bool PER_TASK_AFFINE, bool ACT>
__global__ void bn_bwd_sums_vec_kernel(const scalar_t* __restrict__ dy,
                                       const scalar_t* __restrict__ x,
                                       const float* __restrict__ mean,
                                       const float* __restrict__ rstd,
                                       const float* __restrict__ gamma,
                                       const float* __restrict__ beta,
                                       float* __restrict__ partials,  // [T,NBLK,2,C]
                                       int T, long M, int C, float slope,
                                       int rows_per_block) {
  const int c8n = C / 8;
  const int rows_in_block = blockDim.x / c8n;
  const int c8 = threadIdx.x % c8n;
  const int rg = threadIdx.x / c8n;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  extern __shared__ float ls[];  // [rows_in_block][2][C]
  float s1[8] = {0}, s2[8] = {0};
  if (rg < rows_in_block) {
    float mu[8], r[8], g[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c8 * 8 + j;
      const long tc = (long)t * C + c;
      mu[j] = mean[tc];
      r[j] = rstd[tc];
      g[j] = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
      b[j] = PER_TASK_AFFINE ? beta[tc] : beta[c];
    }
    const scalar_t* xt = x + (long)t * M * C + c8 * 8;
    const scalar_t* dyt = dy + (long)t * M * C + c8 * 8;
    const long row_end = min(row0 + rows_per_block, M);
    for (long m = row0 + rg; m < row_end; m += rows_in_block) {
      float xv[8], dv[8];
      load8(xt + m * C, xv);
      load8(dyt + m * C, dv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (xv[j] - mu[j]) * r[j];
        float d = dv[j];
        if (ACT) d *= ((xh * g[j] + b[j]) > 0.f) ? 1.f : slope;
        s1[j] += d;
        s2[j] += d * xh;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ls[(rg * 2 + 0) * C + c8 * 8 + j] = s1[j];
      ls[(rg * 2 + 1) * C + c8 * 8 + j] = s2[j];
    }
  }
  __syncthreads();
  for (int n_ = rows_in_block; n_ > 1;) {
    const int step = (n_ + 1) >> 1;   // non-pow2-safe fixed pairing
    if (rg < step && rg + step < n_) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ls[(rg * 2 + 0) * C + c8 * 8 + j] +=
            ls[((rg + step) * 2 + 0) * C + c8 * 8 + j];
        ls[(rg * 2 + 1) * C + c8 * 8 + j] +=
            ls[((rg + step) * 2 + 1) * C + c8 * 8 + j];
      }
    }
    __syncthreads();
    n_ = step;
  }
  if (rg == 0) {
    float* pt = partials + (((long)t * gridDim.y + blockIdx.y) * 2) * C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pt[c8 * 8 + j] = ls[0 * C + c8 * 8 + j];
      pt[C + c8 * 8 + j] = ls[1 * C + c8 * 8 + j];
    }
  }
}

template <typename scalar_t, bool PER_TASK_AFFINE, bool ACT>
__global__ void bn_bwd_dx_vec_kernel(const scalar_t* __restrict__ dy,
                                     const scalar_t* __restrict__ x,
                                     scalar_t* __restrict__ dx,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     const float* __restrict__ gamma,
                                     const float* __restrict__ beta,
                                     const float* __restrict__ bsums,
                                     int T, long M, int C, float slope,
                                     int rows_per_block) {
  const int c8n = C / 8;
  const int rows_in_block = blockDim.x / c8n;
  const int c8 = threadIdx.x % c8n;
  const int rg = threadIdx.x / c8n;
  if (rg >= rows_in_block) return;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  const float invM = 1.f / (float)M;
  float mu[8], r[8], g[8], b[8], a1[8], a2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c8 * 8 + j;
    const long tc = (long)t * C + c;
    mu[j] = mean[tc];
    r[j] = rstd[tc];
    g[j] = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
    b[j] = PER_TASK_AFFINE ? beta[tc] : beta[c];
    a1[j] = bsums[((long)t * 2 + 0) * C + c] * invM;
    a2[j] = bsums[((long)t * 2 + 1) * C + c] * invM;
  }
  const scalar_t* xt = x + (long)t * M * C + c8 * 8;
  const scalar_t* dyt = dy + (long)t * M * C + c8 * 8;
  scalar_t* dxt = dx + (long)t * M * C + c8 * 8;
  const long row_end = min(row0 + rows_per_block, M);
  for (long m = row0 + rg; m < row_end; m += rows_in_block) {
    float xv[8], dv[8];
    load8(xt + m * C, xv);
    load8(dyt + m * C, dv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (xv[j] - mu[j]) * r[j];
      float d = dv[j];
      if (ACT) d *= ((xh * g[j] + b[j]) > 0.f) ? 1.f : slope;
      xv[j] = g[j] * r[j] * (d - a1[j] - xh * a2[j]);
    }
    store8(dxt + m * C, xv);
  }
}

// ---------------------------------------------------------------------------
// Stage 1: partial sum / sum-of-squares accumulation into sums[T, 2, C].
// Thread layout: lane -> channel (padded to 64), wave -> row group.
// Coalesced: for a fixed row m, lanes 0..C-1 read consecutive addresses.
// ---------------------------------------------------------------------------
template <typename scalar_t>
__global__ void bn_sums_kernel(const scalar_t* __restrict__ x,
                               float* __restrict__ sums,  // [T, 2, C]
                               int T, long M, int C, int rows_per_block) {
  const int cpad = ((C + WAVE - 1) / WAVE) * WAVE;
  const int lanes_per_row = cpad;
  const int rows_in_block = blockDim.x / lanes_per_row;   // e.g. 256/64 = 4
  const int c = threadIdx.x % lanes_per_row;
  const int rgroup = threadIdx.x / lanes_per_row;

  const int t = blockIdx.x;                                // task
  const long row0 = (long)blockIdx.y * rows_per_block;
  if (c >= C) return;

  const scalar_t* xt = x + (long)t * M * C;
  float s = 0.f, sq = 0.f;
  const long row_end = min(row0 + rows_per_block, M);
  for (long m = row0 + rgroup; m < row_end; m += rows_in_block) {
    const float v = to_f32(xt[m * C + c]);
    s += v;
    sq += v * v;
  }
  // reduce the rows_in_block partial sums for channel c via LDS
  extern __shared__ float lds[];  // [rows_in_block][cpad] x 2
  float* lds_s = lds;
  float* lds_q = lds + blockDim.x;
  lds_s[threadIdx.x] = s;
  lds_q[threadIdx.x] = sq;
  __syncthreads();
  if (rgroup == 0) {
    for (int r = 1; r < rows_in_block; ++r) {
      s += lds_s[r * lanes_per_row + c];
      sq += lds_q[r * lanes_per_row + c];
    }
    atomicAdd(&sums[((long)t * 2 + 0) * C + c], s);
    atomicAdd(&sums[((long)t * 2 + 1) * C + c], sq);
  }
}

// ---------------------------------------------------------------------------
// Stage 2: finalize mean / var / rstd per (t, c).
// ---------------------------------------------------------------------------
__global__ void bn_finalize_kernel(const float* __restrict__ sums, // [T,2,C]
                                   float* __restrict__ mean,       // [T,C]
                                   float* __restrict__ var,        // [T,C]
                                   float* __restrict__ rstd,       // [T,C]
                                   int T, long M, int C, float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * C) return;
  const int t = i / C, c = i % C;
  const float m = sums[((long)t * 2 + 0) * C + c] / (float)M;
  float v = sums[((long)t * 2 + 1) * C + c] / (float)M - m * m;
  v = fmaxf(v, 0.f);
  mean[i] = m;
  var[i] = v;
  rstd[i] = rsqrtf(v + eps);
}

// ---------------------------------------------------------------------------
// Stage 3: normalize + affine + leaky-ReLU, elementwise (grid-stride).
// gamma/beta are [C] (shared meta per-step params) or [T, C] (fast weights).
// ---------------------------------------------------------------------------
template <typename scalar_t, bool PER_TASK_AFFINE, bool ACT>
__global__ void bn_norm_act_kernel(const scalar_t* __restrict__ x,
                                   scalar_t* __restrict__ y,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ beta,
                                   int T, long M, int C, float slope) {
  const long total = (long)T * M * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int c = (int)(i % C);
    const int t = (int)(i / (M * (long)C));
    const long tc = (long)t * C + c;
    const float g = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
    const float b = PER_TASK_AFFINE ? beta[tc] : beta[c];
    float v = (to_f32(x[i]) - mean[tc]) * rstd[tc] * g + b;
    if (ACT) v = v > 0.f ? v : v * slope;
    y[i] = from_f32<scalar_t>(v);
  }
}

// --------------------------------------------------------------------------
// Fused backward of BN+act+maxpool (used when the backward pass itself is
// not being differentiated — outer backward / eval; the create_graph path
// composes the individual Functions instead).  The pooled incoming grad is
// expanded through the argmax mask inline, so the full-resolution `da`
// tensor is never materialized.
//   da(t,nb,h,w,c) = mask match ? dyp(t,nb,h/2,w/2,c) : 0
// then the standard BN+act backward math on da.
// --------------------------------------------------------------------------
template <typename scalar_t, bool PER_TASK_AFFINE>
DEVINL void pool_expand8(const scalar_t* __restrict__ dyp,
                         const unsigned char* __restrict__ mask,
                         long row, int NB, int H, int W, int C,
                         int c0, float* dv) {
  const int Ho = H / 2, Wo = W / 2;
  const int w = (int)(row % W);
  const int h = (int)((row / W) % H);
  const long nb = row / ((long)W * H);
  const int ho = h >> 1, wo = w >> 1;
  if (ho < Ho && wo < Wo) {
    const long o = ((nb * Ho + ho) * Wo + wo) * C + c0;
    const int arg = ((h & 1) << 1) | (w & 1);
    const unsigned long long mp = *(const unsigned long long*)&mask[o];
    float dvv[8];
    load8(&dyp[o], dvv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dv[j] = ((int)((mp >> (8 * j)) & 0xff) == arg) ? dvv[j] : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) dv[j] = 0.f;
  }
}

template <typename scalar_t, bool PER_TASK_AFFINE>
__global__ void bn_pool_bwd_sums_vec_kernel(
    const scalar_t* __restrict__ dyp,      // [T, NB, Ho, Wo, C]
    const unsigned char* __restrict__ mask,
    const scalar_t* __restrict__ x,        // [T, NB, H, W, C]
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ partials,          // [T, NBLK, 2, C]
    int T, int NB, int H, int W, int C, float slope, int rows_per_block) {
  const long M = (long)NB * H * W;
  const int c8n = C / 8;
  const int rows_in_block = blockDim.x / c8n;
  const int c8 = threadIdx.x % c8n;
  const int rg = threadIdx.x / c8n;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  extern __shared__ float ls[];  // [rows_in_block][2][C]
  float s1[8] = {0}, s2[8] = {0};
  const int c0 = c8 * 8;
  if (rg < rows_in_block) {
    float mu[8], r[8], g[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long tc = (long)t * C + c0 + j;
      mu[j] = mean[tc]; r[j] = rstd[tc];
      g[j] = PER_TASK_AFFINE ? gamma[tc] : gamma[c0 + j];
      b[j] = PER_TASK_AFFINE ? beta[tc] : beta[c0 + j];
    }
    const scalar_t* xt = x + (long)t * M * C + c0;
    const scalar_t* dypt = dyp + (long)t * NB * (H / 2) * (W / 2) * C;
    const unsigned char* mt_ = mask + (long)t * NB * (H / 2) * (W / 2) * C;
    const long row_end = min(row0 + rows_per_block, M);
    for (long m = row0 + rg; m < row_end; m += rows_in_block) {
      float xv[8], dv[8];
      load8(xt + m * C, xv);
      pool_expand8<scalar_t, PER_TASK_AFFINE>(dypt, mt_, m, NB, H, W, C, c0, dv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (xv[j] - mu[j]) * r[j];
        float d = dv[j];
        d *= ((xh * g[j] + b[j]) > 0.f) ? 1.f : slope;
        s1[j] += d;
        s2[j] += d * xh;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ls[(rg * 2 + 0) * C + c0 + j] = s1[j];
      ls[(rg * 2 + 1) * C + c0 + j] = s2[j];
    }
  }
  __syncthreads();
  for (int n_ = rows_in_block; n_ > 1;) {
    const int step = (n_ + 1) >> 1;   // non-pow2-safe fixed pairing
    if (rg < step && rg + step < n_) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ls[(rg * 2 + 0) * C + c0 + j] +=
            ls[((rg + step) * 2 + 0) * C + c0 + j];
        ls[(rg * 2 + 1) * C + c0 + j] +=
            ls[((rg + step) * 2 + 1) * C + c0 + j];
      }
    }
    __syncthreads();
    n_ = step;
  }
  if (rg == 0) {
    float* pt = partials + (((long)t * gridDim.y + blockIdx.y) * 2) * C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pt[c0 + j] = ls[0 * C + c0 + j];
      pt[C + c0 + j] = ls[1 * C + c0 + j];
    }
  }
}

template <typename scalar_t, bool PER_TASK_AFFINE>
__global__ void bn_pool_bwd_dx_vec_kernel(
    const scalar_t* __restrict__ dyp, const unsigned char* __restrict__ mask,
    const scalar_t* __restrict__ x, scalar_t* __restrict__ dx,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ bsums,
    int T, int NB, int H, int W, int C, float slope, int rows_per_block) {
  const long M = (long)NB * H * W;
  const int c8n = C / 8;
  const int rows_in_block = blockDim.x / c8n;
  const int c8 = threadIdx.x % c8n;
  const int rg = threadIdx.x / c8n;
  if (rg >= rows_in_block) return;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  const float invM = 1.f / (float)M;
  const int c0 = c8 * 8;
  float mu[8], r[8], g[8], b[8], a1[8], a2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long tc = (long)t * C + c0 + j;
    mu[j] = mean[tc]; r[j] = rstd[tc];
    g[j] = PER_TASK_AFFINE ? gamma[tc] : gamma[c0 + j];
    b[j] = PER_TASK_AFFINE ? beta[tc] : beta[c0 + j];
    a1[j] = bsums[((long)t * 2 + 0) * C + c0 + j] * invM;
    a2[j] = bsums[((long)t * 2 + 1) * C + c0 + j] * invM;
  }
  const scalar_t* xt = x + (long)t * M * C + c0;
  scalar_t* dxt = dx + (long)t * M * C + c0;
  const scalar_t* dypt = dyp + (long)t * NB * (H / 2) * (W / 2) * C;
  const unsigned char* mt_ = mask + (long)t * NB * (H / 2) * (W / 2) * C;
  const long row_end = min(row0 + rows_per_block, M);
  for (long m = row0 + rg; m < row_end; m += rows_in_block) {
    float xv[8], dv[8];
    load8(xt + m * C, xv);
    pool_expand8<scalar_t, PER_TASK_AFFINE>(dypt, mt_, m, NB, H, W, C, c0, dv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (xv[j] - mu[j]) * r[j];
      float d = dv[j];
      d *= ((xh * g[j] + b[j]) > 0.f) ? 1.f : slope;
      xv[j] = g[j] * r[j] * (d - a1[j] - xh * a2[j]);
    }
    store8(dxt + m * C, xv);
  }
}

// ---------------------------------------------------------------------------
// Backward stage 1: per-(t,c) sums  s1 = sum dy', s2 = sum dy' * xhat,
// where dy' = dy * act'(pre-act) and xhat = (x - mean) * rstd.
// ---------------------------------------------------------------------------
template <typename scalar_t, bool PER_TASK_AFFINE, bool ACT>
__global__ void bn_bwd_sums_kernel(const scalar_t* __restrict__ dy,
                                   const scalar_t* __restrict__ x,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ beta,
                                   float* __restrict__ bsums,  // [T, 2, C]
                                   int T, long M, int C, float slope,
                                   int rows_per_block) {
  const int cpad = ((C + WAVE - 1) / WAVE) * WAVE;
  const int lanes_per_row = cpad;
  const int rows_in_block = blockDim.x / lanes_per_row;
  const int c = threadIdx.x % lanes_per_row;
  const int rgroup = threadIdx.x / lanes_per_row;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  if (c >= C) return;

  const long tc = (long)t * C + c;
  const float mu = mean[tc], rs = rstd[tc];
  const float g = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
  const float b = PER_TASK_AFFINE ? beta[tc] : beta[c];
  const scalar_t* xt = x + (long)t * M * C;
  const scalar_t* dyt = dy + (long)t * M * C;
  float s1 = 0.f, s2 = 0.f;
  const long row_end = min(row0 + rows_per_block, M);
  for (long m = row0 + rgroup; m < row_end; m += rows_in_block) {
    const float xh = (to_f32(xt[m * C + c]) - mu) * rs;
    float d = to_f32(dyt[m * C + c]);
    if (ACT) {
      const float pre = xh * g + b;
      d *= (pre > 0.f) ? 1.f : slope;
    }
    s1 += d;
    s2 += d * xh;
  }
  extern __shared__ float lds[];
  float* lds_1 = lds;
  float* lds_2 = lds + blockDim.x;
  lds_1[threadIdx.x] = s1;
  lds_2[threadIdx.x] = s2;
  __syncthreads();
  if (rgroup == 0) {
    for (int r = 1; r < rows_in_block; ++r) {
      s1 += lds_1[r * lanes_per_row + c];
      s2 += lds_2[r * lanes_per_row + c];
    }
    atomicAdd(&bsums[((long)t * 2 + 0) * C + c], s1);
    atomicAdd(&bsums[((long)t * 2 + 1) * C + c], s2);
  }
}

// ---------------------------------------------------------------------------
// Backward stage 2: dx = gamma*rstd * (dy' - s1/M - xhat * s2/M)
// (dgamma = s2, dbeta = s1 are read from bsums by the wrapper.)
// ---------------------------------------------------------------------------
template <typename scalar_t, bool PER_TASK_AFFINE, bool ACT>
__global__ void bn_bwd_dx_kernel(const scalar_t* __restrict__ dy,
                                 const scalar_t* __restrict__ x,
                                 scalar_t* __restrict__ dx,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ rstd,
                                 const float* __restrict__ gamma,
                                 const float* __restrict__ beta,
                                 const float* __restrict__ bsums,
                                 int T, long M, int C, float slope) {
  const long total = (long)T * M * C;
  const float invM = 1.f / (float)M;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int c = (int)(i % C);
    const int t = (int)(i / (M * (long)C));
    const long tc = (long)t * C + c;
    const float mu = mean[tc], rs = rstd[tc];
    const float g = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
    const float b = PER_TASK_AFFINE ? beta[tc] : beta[c];
    const float xh = (to_f32(x[i]) - mu) * rs;
    float d = to_f32(dy[i]);
    if (ACT) {
      const float pre = xh * g + b;
      d *= (pre > 0.f) ? 1.f : slope;
    }
    const float s1 = bsums[((long)t * 2 + 0) * C + c];
    const float s2 = bsums[((long)t * 2 + 1) * C + c];
    dx[i] = from_f32<scalar_t>(g * rs * (d - s1 * invM - xh * s2 * invM));
  }
}

// ---------------------------------------------------------------------------
// C++ launchers (declared in bindings.cpp)
// ---------------------------------------------------------------------------
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

namespace {

constexpr int kRowsPerBlock = 256;
constexpr int kThreads = 256;

// the 8-channel vector kernels; their ordered reduce writes the sums whole
inline bool bn_vec_ok(int C) { return (C % 8 == 0) && C <= 512; }

template <typename scalar_t>
void bn_fwd_impl(const torch::Tensor& x, const torch::Tensor& gamma,
                 const torch::Tensor& beta, torch::Tensor& y,
                 torch::Tensor& sums, torch::Tensor& mean, torch::Tensor& var,
                 torch::Tensor& rstd, double eps, double slope, bool act,
                 int T, long M, int C) {
  auto stream = at::cuda::getCurrentCUDAStream();
  const bool per_task = gamma.dim() == 2;
  const bool vec = bn_vec_ok(C);
  const int cpad = ((C + WAVE - 1) / WAVE) * WAVE;
  dim3 sums_grid(T, (unsigned)((M + kRowsPerBlock - 1) / kRowsPerBlock));
  const int threads = cpad * std::max<int>(1, kThreads / cpad);
  const int lds_bytes = 2 * threads * sizeof(float);
  if (vec) {
    const int rpb = 1024;  // amortize the per-block staging rounds
    const int nb = (int)((M + rpb - 1) / rpb);
    dim3 g(T, (unsigned)nb);
    auto partials = torch::empty({T, nb, 2, C},
                                 x.options().dtype(torch::kFloat32));
    hipLaunchKernelGGL((bn_sums_vec_kernel<scalar_t>), g, dim3(256),
                       16384, stream.stream(),
                       reinterpret_cast<const scalar_t*>(x.data_ptr()),
                       partials.data_ptr<float>(), T, M, C, rpb);
    hipLaunchKernelGGL(bn_reduce2_kernel, dim3((T * C + 255) / 256), dim3(256),
                       0, stream.stream(), partials.data_ptr<float>(),
                       sums.data_ptr<float>(), T, nb, C, (float*)nullptr,
                       (float*)nullptr);
  } else
  hipLaunchKernelGGL((bn_sums_kernel<scalar_t>), sums_grid, dim3(threads),
                     lds_bytes, stream.stream(),
                     reinterpret_cast<const scalar_t*>(x.data_ptr()), sums.data_ptr<float>(), T, M, C,
                     kRowsPerBlock);
  const int fin_threads = 256;
  const int fin_blocks = (T * C + fin_threads - 1) / fin_threads;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(fin_blocks), dim3(fin_threads), 0,
                     stream.stream(), sums.data_ptr<float>(),
                     mean.data_ptr<float>(), var.data_ptr<float>(),
                     rstd.data_ptr<float>(), T, M, C, (float)eps);
  const long total = (long)T * M * C;
#define LAUNCH_NORM(PT, ACT_)                                                  \
  do {                                                                         \
    if (vec) {                                                                 \
      hipLaunchKernelGGL((bn_norm_act_vec_kernel<scalar_t, PT, ACT_>),         \
                         sums_grid, dim3(256), 0, stream.stream(),             \
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),      \
                         reinterpret_cast<scalar_t*>(y.data_ptr()),            \
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),       \
                         gamma.data_ptr<float>(), beta.data_ptr<float>(),      \
                         T, M, C, (float)slope, kRowsPerBlock);                \
    } else {                                                                   \
      hipLaunchKernelGGL((bn_norm_act_kernel<scalar_t, PT, ACT_>),             \
                         dim3(ew_grid(total, kThreads)), dim3(kThreads), 0,    \
                         stream.stream(),                                      \
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),      \
                         reinterpret_cast<scalar_t*>(y.data_ptr()),            \
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),       \
                         gamma.data_ptr<float>(), beta.data_ptr<float>(),      \
                         T, M, C, (float)slope);                               \
    }                                                                          \
  } while (0)
  if (per_task) { if (act) LAUNCH_NORM(true, true); else LAUNCH_NORM(true, false); }
  else { if (act) LAUNCH_NORM(false, true); else LAUNCH_NORM(false, false); }
#undef LAUNCH_NORM
}

template <typename scalar_t>
void bn_bwd_impl(const torch::Tensor& dy, const torch::Tensor& x,
                 const torch::Tensor& mean, const torch::Tensor& rstd,
                 const torch::Tensor& gamma, const torch::Tensor& beta,
                 torch::Tensor& bsums, torch::Tensor& dx,
                 torch::Tensor& dgamma_t, torch::Tensor& dbeta_t, double slope,
                 bool act, int T, long M, int C) {
  auto stream = at::cuda::getCurrentCUDAStream();
  const bool per_task = gamma.dim() == 2;
  const bool vec = bn_vec_ok(C);
  const int cpad = ((C + WAVE - 1) / WAVE) * WAVE;
  dim3 sums_grid(T, (unsigned)((M + kRowsPerBlock - 1) / kRowsPerBlock));
  const int threads = cpad * std::max<int>(1, kThreads / cpad);
  const int lds_bytes = 2 * threads * sizeof(float);
  const long total = (long)T * M * C;
#define LAUNCH_BWD(PT, ACT_)                                                   \
  do {                                                                         \
    if (vec) {                                                                 \
      const int nb = (int)((M + 1023) / 1024);                                 \
      dim3 gs(T, (unsigned)nb);                                                \
      auto partials = torch::empty({T, nb, 2, C},                              \
                                   x.options().dtype(torch::kFloat32));        \
      hipLaunchKernelGGL((bn_bwd_sums_vec_kernel<scalar_t, PT, ACT_>),         \
                         gs, dim3(256), 16384,                                 \
                         stream.stream(),                                      \
                         reinterpret_cast<const scalar_t*>(dy.data_ptr()),     \
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),      \
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),       \
                         gamma.data_ptr<float>(), beta.data_ptr<float>(),      \
                         partials.data_ptr<float>(), T, M, C, (float)slope,    \
                         1024);                                                \
      hipLaunchKernelGGL(bn_reduce2_kernel, dim3((T * C + 255) / 256),         \
                         dim3(256), 0, stream.stream(),                        \
                         partials.data_ptr<float>(),                           \
                         bsums.data_ptr<float>(), T, nb, C,                    \
                         dbeta_t.data_ptr<float>(),                            \
                         dgamma_t.data_ptr<float>());                          \
      hipLaunchKernelGGL((bn_bwd_dx_vec_kernel<scalar_t, PT, ACT_>),           \
                         sums_grid, dim3(256), 0, stream.stream(),             \
                         reinterpret_cast<const scalar_t*>(dy.data_ptr()),     \
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),      \
                         reinterpret_cast<scalar_t*>(dx.data_ptr()),           \
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),       \
                         gamma.data_ptr<float>(), beta.data_ptr<float>(),      \
                         bsums.data_ptr<float>(), T, M, C, (float)slope,       \
                         kRowsPerBlock);                                       \
      break;                                                                   \
    }                                                                          \
    hipLaunchKernelGGL((bn_bwd_sums_kernel<scalar_t, PT, ACT_>), sums_grid,    \
                       dim3(threads), lds_bytes, stream.stream(),              \
                       reinterpret_cast<const scalar_t*>(dy.data_ptr()),       \
                       reinterpret_cast<const scalar_t*>(x.data_ptr()),        \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                       gamma.data_ptr<float>(), beta.data_ptr<float>(),        \
                       bsums.data_ptr<float>(), T, M, C, (float)slope,         \
                       kRowsPerBlock);                                         \
    hipLaunchKernelGGL((bn_bwd_dx_kernel<scalar_t, PT, ACT_>),                 \
                       dim3(ew_grid(total, kThreads)), dim3(kThreads), 0,      \
                       stream.stream(),                                        \
                       reinterpret_cast<const scalar_t*>(dy.data_ptr()),       \
                       reinterpret_cast<const scalar_t*>(x.data_ptr()),        \
                       reinterpret_cast<scalar_t*>(dx.data_ptr()),             \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                       gamma.data_ptr<float>(), beta.data_ptr<float>(),        \
                       bsums.data_ptr<float>(), T, M, C, (float)slope);        \
  } while (0)
  if (per_task) { if (act) LAUNCH_BWD(true, true); else LAUNCH_BWD(true, false); }
  else { if (act) LAUNCH_BWD(false, true); else LAUNCH_BWD(false, false); }
#undef LAUNCH_BWD
}

}  // namespace

// x: [T, M, C] contiguous (caller flattens NS*H*W -> M), fp32 or bf16.
// gamma/beta: [C] or [T, C] fp32.
std::vector<torch::Tensor> bn_act_fwd(torch::Tensor x, torch::Tensor gamma,
                                      torch::Tensor beta, double eps,
                                      double slope, bool act) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous());
  const int T = (int)x.size(0);
  const long M = x.size(1);
  const int C = (int)x.size(2);
  auto opts = x.options().dtype(torch::kFloat32);
  // the scalar path accumulates into sums with atomics; the vector path's
  // ordered reduce overwrites it whole
  auto sums = bn_vec_ok(C) ? torch::empty({T, 2, C}, opts)
                           : torch::zeros({T, 2, C}, opts);
  auto mean = torch::empty({T, C}, opts);
  auto var = torch::empty({T, C}, opts);
  auto rstd = torch::empty({T, C}, opts);
  auto y = torch::empty_like(x);
  auto gc = gamma.contiguous().to(torch::kFloat32);
  auto bc = beta.contiguous().to(torch::kFloat32);
  if (x.scalar_type() == torch::kFloat32) {
    bn_fwd_impl<float>(x, gc, bc, y, sums, mean, var, rstd, eps, slope, act, T, M, C);
  } else if (x.scalar_type() == torch::kBFloat16) {
    bn_fwd_impl<__hip_bfloat16>(x, gc, bc, y, sums, mean, var, rstd, eps, slope, act, T, M, C);
  } else {
    TORCH_CHECK(false, "bn_act_fwd: unsupported dtype");
  }
  return {y, mean, var, rstd};
}

std::vector<torch::Tensor> bn_act_bwd(torch::Tensor dy, torch::Tensor x,
                                      torch::Tensor mean, torch::Tensor rstd,
                                      torch::Tensor gamma, torch::Tensor beta,
                                      double slope, bool act) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 3);
  auto dyc = dy.contiguous();
  const int T = (int)x.size(0);
  const long M = x.size(1);
  const int C = (int)x.size(2);
  auto opts = x.options().dtype(torch::kFloat32);
  const bool vec = bn_vec_ok(C);
  auto bsums = vec ? torch::empty({T, 2, C}, opts)
                   : torch::zeros({T, 2, C}, opts);
  // vector path: the ordered reduce writes both straight into these
  torch::Tensor dgamma_t, dbeta_t;
  if (vec) {
    dgamma_t = torch::empty({T, C}, opts);
    dbeta_t = torch::empty({T, C}, opts);
  }
  auto dx = torch::empty_like(x);
  auto gc = gamma.contiguous().to(torch::kFloat32);
  auto bc = beta.contiguous().to(torch::kFloat32);
  if (x.scalar_type() == torch::kFloat32) {
    bn_bwd_impl<float>(dyc, x, mean, rstd, gc, bc, bsums, dx, dgamma_t,
                       dbeta_t, slope, act, T, M, C);
  } else if (x.scalar_type() == torch::kBFloat16) {
    bn_bwd_impl<__hip_bfloat16>(dyc, x, mean, rstd, gc, bc, bsums, dx,
                                dgamma_t, dbeta_t, slope, act, T, M, C);
  } else {
    TORCH_CHECK(false, "bn_act_bwd: unsupported dtype");
  }
  // dbeta = bsums[:,0,:], dgamma = bsums[:,1,:]  (per task; wrapper reduces
  // over T when gamma is shared)
  if (vec) return {dx, dgamma_t, dbeta_t};
  return {dx, bsums.select(1, 1).clone(), bsums.select(1, 0).clone()};
}

// x: [T, NB, H, W, C] contiguous bf16/fp32; returns
// {y_pooled [T, NB, H/2, W/2, C], mask u8, mean, var, rstd}
// Fuses normalize+leakyReLU+maxpool into one pass over the conv output;
// requires C % 8 == 0 (callers fall back to the unfused ops otherwise).
std::vector<torch::Tensor> bn_act_pool_fwd(torch::Tensor x, torch::Tensor gamma,
                                           torch::Tensor beta, double eps,
                                           double slope,
                                           c10::optional<torch::Tensor> sums_in) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  TORCH_CHECK(C % 8 == 0 && C <= 512, "bn_act_pool_fwd needs C % 8 == 0");
  const long M = (long)NB * H * W;
  const int Ho = H / 2, Wo = W / 2;
  auto fopts = x.options().dtype(torch::kFloat32);
  const bool have_sums = sums_in.has_value() && sums_in->numel() == T * 2 * C;
  auto sums = have_sums ? sums_in->contiguous()
                        : torch::empty({T, 2, C}, fopts);
  auto mean = torch::empty({T, C}, fopts);
  auto var = torch::empty({T, C}, fopts);
  auto rstd = torch::empty({T, C}, fopts);
  auto y = torch::empty({T, NB, Ho, Wo, C}, x.options());
  auto mask = torch::empty({T, NB, Ho, Wo, C}, x.options().dtype(torch::kUInt8));
  auto gc = gamma.contiguous().to(torch::kFloat32);
  auto bc = beta.contiguous().to(torch::kFloat32);
  const bool per_task = gamma.dim() == 2;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int rpb = 1024;
  dim3 gsums(T, (unsigned)((M + rpb - 1) / rpb));
  const long ptotal = (long)T * NB * Ho * Wo * (C / 8);
  const int pblocks = (int)std::min<long>((ptotal + 255) / 256, 4096);

#define LAUNCH_BNP(ST, PT)                                                     \
  do {                                                                         \
    if (!have_sums) {                                                          \
      const int nb_ = (int)((M + rpb - 1) / rpb);                              \
      auto partials = torch::empty({T, nb_, 2, C}, fopts);                     \
      hipLaunchKernelGGL((bn_sums_vec_kernel<ST>), gsums, dim3(256),           \
                         16384, stream.stream(),                               \
                         reinterpret_cast<const ST*>(x.data_ptr()),            \
                         partials.data_ptr<float>(), T, M, C, rpb);            \
      hipLaunchKernelGGL(bn_reduce2_kernel, dim3((T * C + 255) / 256),         \
                         dim3(256), 0, stream.stream(),                        \
                         partials.data_ptr<float>(),                           \
                         sums.data_ptr<float>(), T, nb_, C, (float*)nullptr,   \
                         (float*)nullptr);                                     \
    }                                                                          \
    const int fin_blocks = (T * C + 255) / 256;                                \
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(fin_blocks), dim3(256), 0,     \
                       stream.stream(), sums.data_ptr<float>(),                \
                       mean.data_ptr<float>(), var.data_ptr<float>(),          \
                       rstd.data_ptr<float>(), T, M, C, (float)eps);           \
    hipLaunchKernelGGL((bn_norm_act_pool_vec_kernel<ST, PT>), dim3(pblocks),   \
                       dim3(256), 0, stream.stream(),                          \
                       reinterpret_cast<const ST*>(x.data_ptr()),              \
                       reinterpret_cast<ST*>(y.data_ptr()),                    \
                       mask.data_ptr<unsigned char>(),                         \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                       gc.data_ptr<float>(), bc.data_ptr<float>(),             \
                       T, NB, H, W, C, Ho, Wo, (float)slope);                  \
  } while (0)

  if (x.scalar_type() == torch::kFloat32) {
    if (per_task) LAUNCH_BNP(float, true); else LAUNCH_BNP(float, false);
  } else if (x.scalar_type() == torch::kBFloat16) {
    if (per_task) LAUNCH_BNP(__hip_bfloat16, true);
    else LAUNCH_BNP(__hip_bfloat16, false);
  } else {
    TORCH_CHECK(false, "bn_act_pool_fwd: unsupported dtype");
  }
#undef LAUNCH_BNP
  return {y, mask, mean, var, rstd};
}

// Fused backward of BN+act+pool: dyp [T,NB,Ho,Wo,C], mask u8, x [T,NB,H,W,C]
// -> {dx [T,NB,H,W,C], dgamma_t [T,C], dbeta_t [T,C]}
std::vector<torch::Tensor> bn_act_pool_bwd(torch::Tensor dyp, torch::Tensor mask,
                                           torch::Tensor x, torch::Tensor mean,
                                           torch::Tensor rstd, torch::Tensor gamma,
                                           torch::Tensor beta, double slope) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  TORCH_CHECK(C % 8 == 0 && C <= 512);
  const long M = (long)NB * H * W;
  auto fopts = x.options().dtype(torch::kFloat32);
  auto bsums = torch::empty({T, 2, C}, fopts);
  auto dgamma_t = torch::empty({T, C}, fopts);
  auto dbeta_t = torch::empty({T, C}, fopts);
  auto dx = torch::empty_like(x);
  auto gc = gamma.contiguous().to(torch::kFloat32);
  auto bc = beta.contiguous().to(torch::kFloat32);
  auto dypc = dyp.contiguous();
  const bool per_task = gamma.dim() == 2;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int rpb = 1024;
  dim3 g(T, (unsigned)((M + rpb - 1) / rpb));

#define LAUNCH_BPB(ST, PT)                                                     \
  do {                                                                         \
    const int nb_ = (int)((M + rpb - 1) / rpb);                                \
    auto partials = torch::empty({T, nb_, 2, C}, fopts);                       \
    hipLaunchKernelGGL((bn_pool_bwd_sums_vec_kernel<ST, PT>), g, dim3(256),    \
                       16384, stream.stream(),                                 \
                       reinterpret_cast<const ST*>(dypc.data_ptr()),           \
                       mask.data_ptr<unsigned char>(),                         \
                       reinterpret_cast<const ST*>(x.data_ptr()),              \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                       gc.data_ptr<float>(), bc.data_ptr<float>(),             \
                       partials.data_ptr<float>(), T, NB, H, W, C,             \
                       (float)slope, rpb);                                     \
    hipLaunchKernelGGL(bn_reduce2_kernel, dim3((T * C + 255) / 256),           \
                       dim3(256), 0, stream.stream(),                          \
                       partials.data_ptr<float>(),                             \
                       bsums.data_ptr<float>(), T, nb_, C,                     \
                       dbeta_t.data_ptr<float>(),                              \
                       dgamma_t.data_ptr<float>());                            \
    hipLaunchKernelGGL((bn_pool_bwd_dx_vec_kernel<ST, PT>), g, dim3(256), 0,   \
                       stream.stream(),                                        \
                       reinterpret_cast<const ST*>(dypc.data_ptr()),           \
                       mask.data_ptr<unsigned char>(),                         \
                       reinterpret_cast<const ST*>(x.data_ptr()),              \
                       reinterpret_cast<ST*>(dx.data_ptr()),                   \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                       gc.data_ptr<float>(), bc.data_ptr<float>(),             \
                       bsums.data_ptr<float>(), T, NB, H, W, C, (float)slope,  \
                       rpb);                                                   \
  } while (0)

  if (x.scalar_type() == torch::kFloat32) {
    if (per_task) LAUNCH_BPB(float, true); else LAUNCH_BPB(float, false);
  } else if (x.scalar_type() == torch::kBFloat16) {
    if (per_task) LAUNCH_BPB(__hip_bfloat16, true);
    else LAUNCH_BPB(__hip_bfloat16, false);
  } else {
    TORCH_CHECK(false, "bn_act_pool_bwd: unsupported dtype");
  }
#undef LAUNCH_BPB
  // dbeta_t = bsums[:,0], dgamma_t = bsums[:,1], written by the reduce
  return {dx, dgamma_t, dbeta_t};
}
