// Task-batched STRIDE-2 3x3 convolution trio (fwd / dgrad / wgrad) as MFMA
// implicit GEMM on gfx950 — the conv of the max_pooling=False backbone
// (reference meta_neural_network_architectures.py:568-573: stride-2 convs,
// no pooling, global average pool before the head).
//
//   fwd   : Y[t]  = im2col_s2(X[t]) @ Wp[t]       M=NB*Ho*Wo, N=F, K=9*C
//           gather iy = 2*oy + ky - p; odd H with p=1 reads iy = H on the
//           last output row, so all four edges are predicated.
//   dgrad : dX[iy,ix,c] = sum dY[(iy+p-ky)/2, (ix+p-kx)/2, f] * W[f,c,ky,kx]
//           over the taps whose divisions are exact.  The output pixels are
//           split by the parity of (iy+p, ix+p) into four dense implicit
//           GEMMs over their own tap subsets (4, 2, 2, 1 taps; K = taps*F) —
//           one launch, parity in blockIdx.z.  No zero-dilated dY: that
//           would spend ~4x the MFMA work on zeros.  Pixels no output
//           touches (p=0 trailing row/column) see only out-of-range taps
//           and come out exactly zero.
//   wgrad : dW[t] = dY[t]^T @ im2col_s2(X[t])     split-K over NB*Ho*Wo,
//           bias grad fused (same structure as tconv_wgrad_kernel).
//
// Numerics contract = tconv.hip: bf16 NHWC activations, weights rounded
// to bf16 at repack, fp32 accumulate via v_mfma_f32_16x16x32_bf16, bf16
// out for fwd/dgrad, fp32 dw/db.  C <= 64, F <= 64.
// Schedule = the v1 stride-1 kernel: register staging between two
// barriers into XOR-swizzled LDS tiles, BM=256, 8 waves, BK=64.

#include "common.h"
#include "conv_host.h"
#include "wgrad_plan.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

using bf16 = __hip_bfloat16;
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

// same involution as tconv.hip: XOR row bits into the 16-byte-slot bits of
// a [rows][64] bf16 tile (index in shorts)
DEVINL int sswz64(int row, int col) {
  return (row * 64 + col) ^ ((row & 7) << 3);
}

#define SBM 256
#define SBK 64
#define SKMAX 576      // 9 * 64
#define SWBK 64        // wgrad K-step
#define SWGN 64        // wgrad output columns per block (4 waves x 16)
static_assert(SWBK == wgplan::kStep && SWGN == wgplan::kCols,
              "wgrad_plan.h cuts K-chunks for these tiles");

// ---------------------------------------------------------------------------
// Weight repack: W [T, F, C, 3, 3] fp32 -> Wp [T, 9, Ci, Co] bf16
//   fwd  : Wp[t][ky*3+kx][c][f] = W[t][f][c][ky][kx]   (Ci=C, Co=F)
//   dgrad: Wp[t][ky*3+kx][f][c] = W[t][f][c][ky][kx]   (Ci=F, Co=C)
// (no tap flip for dgrad: the parity kernels index taps directly)
// ---------------------------------------------------------------------------
__global__ void sconv_repack_kernel(const float* __restrict__ w,
                                    bf16* __restrict__ wp,
                                    int T, int F, int C, bool dgrad) {
  const long total = (long)T * F * C * 9;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    long r = i;
    const int kx = (int)(r % 3); r /= 3;
    const int ky = (int)(r % 3); r /= 3;
    const int c = (int)(r % C); r /= C;
    const int f = (int)(r % F); r /= F;
    const long t = r;
    long o;
    if (!dgrad) {
      o = (((t * 9 + (long)(ky * 3 + kx)) * C + c) * F) + f;
    } else {
      o = (((t * 9 + (long)(ky * 3 + kx)) * F + f) * C) + c;
    }
    wp[o] = __float2bfloat16(w[i]);
  }
}

// ---------------------------------------------------------------------------
// fwd / dgrad kernel: D[t] rows = gather(S[t]) @ Wp[t] rows.
//   S  [T, NB, Hs, Ws, Ci]  bf16  (fwd: X; dgrad: dY)
//   Wp [T, 9, Ci, Co]       bf16  (sconv_repack)
//   D  [T, NB, Hd, Wd, Co]  bf16  (fwd: Y; dgrad: dX)
// Every GEMM row m is an output pixel with a base source coordinate
// (row_h, row_w); every k is a (tap, channel) with a source offset
// (dh, dw) and a weight row.  fwd: base = 2*o - p, offset = +tap.
// dgrad (parity py,px in blockIdx.z): the rows are the pixels
// iy = h0 + 2j with h0 = py ^ p, base a = (iy + p - py)/2, and the taps
// ky = py ? {1} : {0, 2} read oy = a - (ky - py)/2.
// ---------------------------------------------------------------------------
template <bool DGRAD>
__global__ __launch_bounds__(512, 2)
void sconv_mm_kernel(const bf16* __restrict__ S, const bf16* __restrict__ Wp,
                     const float* __restrict__ bias, bf16* __restrict__ D,
                     int NB, int Hs, int Ws, int Ci,
                     int Hd, int Wd, int Co, int pad) {
  const int t = blockIdx.y;
  int py = 0, px = 0, h0 = 0, w0 = 0, ah = 0, aw = 0;
  int cntH = Hd, cntW = Wd, nkx = 3, ntaps = 9;
  if (DGRAD) {
    py = (int)blockIdx.z >> 1;
    px = (int)blockIdx.z & 1;
    h0 = py ^ pad;
    w0 = px ^ pad;
    cntH = Hd > h0 ? (Hd - h0 + 1) / 2 : 0;
    cntW = Wd > w0 ? (Wd - w0 + 1) / 2 : 0;
    ah = (h0 + pad - py) / 2;
    aw = (w0 + pad - px) / 2;
    nkx = px ? 1 : 2;
    ntaps = (py ? 1 : 2) * nkx;
  }
  const long Mtot = (long)NB * cntH * cntW;
  const long m0 = (long)blockIdx.x * SBM;
  if (m0 >= Mtot) return;   // block-uniform: smaller parity classes
  const int K = ntaps * Ci;
  const int ksteps = (K + SBK - 1) / SBK;
  const int ntiles = (Co + 15) / 16;

  __shared__ short lds_a[SBM * SBK];       // swizzled, see sswz64
  __shared__ short lds_bt[64 * SBK];       // B^T: [col][k], swizzled
  __shared__ int row_h[SBM], row_w[SBM], row_n[SBM], row_pix[SBM];
  __shared__ int ktab_dh[SKMAX + SBK], ktab_dw[SKMAX + SBK];
  __shared__ int ktab_c[SKMAX + SBK], ktab_wr[SKMAX + SBK];

  // per-block row decode (once)
  for (int m = threadIdx.x; m < SBM; m += blockDim.x) {
    const long mg = m0 + m;
    if (mg < Mtot) {
      const int jw = (int)(mg % cntW);
      const int jh = (int)((mg / cntW) % cntH);
      const int n = (int)(mg / ((long)cntW * cntH));
      row_n[m] = n;
      if (DGRAD) {
        row_h[m] = ah + jh;
        row_w[m] = aw + jw;
        row_pix[m] = (n * Hd + h0 + 2 * jh) * Wd + w0 + 2 * jw;
      } else {
        row_h[m] = 2 * jh - pad;
        row_w[m] = 2 * jw - pad;
        row_pix[m] = (int)mg;
      }
    } else {
      row_n[m] = -1;
    }
  }
  // k-table for the whole K range (K <= 576 since Ci <= 64)
  for (int k = threadIdx.x; k < ksteps * SBK; k += blockDim.x) {
    if (k < K) {
      const int tap = k / Ci;
      const int c = k - tap * Ci;
      ktab_c[k] = c;
      if (DGRAD) {
        const int tky = tap / nkx, tkx = tap - tky * nkx;
        const int ky = py ? 1 : 2 * tky;
        const int kx = px ? 1 : 2 * tkx;
        ktab_dh[k] = -tky;
        ktab_dw[k] = -tkx;
        ktab_wr[k] = (ky * 3 + kx) * Ci + c;
      } else {
        ktab_dh[k] = tap / 3;
        ktab_dw[k] = tap % 3;
        ktab_wr[k] = k;
      }
    } else {
      ktab_c[k] = -1;
      ktab_wr[k] = -1;
    }
  }

  const bf16* St = S + (long)t * NB * Hs * Ws * Ci;
  const bf16* Wt = Wp + (long)t * 9 * Ci * Co;

  const int wave = threadIdx.x / WAVE;          // 0..7: 32-row m-subtile
  const int lane = threadIdx.x % WAVE;
  const int fr = lane & 15;                      // fragment row/col
  const int fk = lane >> 4;                      // k-group 0..3

  f32x4 acc[2][4];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[hh][i] = {0.f, 0.f, 0.f, 0.f};

  __syncthreads();
  for (int ks = 0; ks < ksteps; ++ks) {
    const int k0 = ks * SBK;
    // stage A (gather): slot s -> (m, kk0), SBK/8 slots per row; vector
    // path when the 8-k run stays inside one tap
    for (int s = threadIdx.x; s < SBM * (SBK / 8); s += blockDim.x) {
      const int m = s / (SBK / 8);
      const int kk0 = (s % (SBK / 8)) * 8;
      const int n = row_n[m];
      const int c0 = ktab_c[k0 + kk0];
      const int c7 = ktab_c[k0 + kk0 + 7];
      if ((Ci % 8 == 0) && c0 >= 0 && c7 == c0 + 7) {
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n >= 0) {
          const int h = row_h[m] + ktab_dh[k0 + kk0];
          const int w = row_w[m] + ktab_dw[k0 + kk0];
          if (h >= 0 && h < Hs && w >= 0 && w < Ws) {
            v = *(const bf16x8*)&(
                (const short*)St)[(((long)n * Hs + h) * Ws + w) * Ci + c0];
          }
        }
        *(bf16x8*)&lds_a[sswz64(m, kk0)] = v;
      } else {
        for (int j = 0; j < 8; ++j) {
          const int kk = kk0 + j;
          const int c = ktab_c[k0 + kk];
          short v = 0;
          if (n >= 0 && c >= 0) {
            const int h = row_h[m] + ktab_dh[k0 + kk];
            const int w = row_w[m] + ktab_dw[k0 + kk];
            if (h >= 0 && h < Hs && w >= 0 && w < Ws) {
              v = ((const short*)St)[(((long)n * Hs + h) * Ws + w) * Ci + c];
            }
          }
          lds_a[sswz64(m, kk & ~7) + (kk & 7)] = v;
        }
      }
    }
    // stage B^T: slot s -> (kk = s>>3, f0 = (s&7)*8); the weight row comes
    // from the k-table (dgrad's taps are a subset of the 9)
    for (int s = threadIdx.x; s < SBK * 8; s += blockDim.x) {
      const int kk = s >> 3;           // 8 f-slots per k row (Co <= 64)
      const int f0 = (s & 7) * 8;
      const int wr = ktab_wr[k0 + kk];
      if ((Co % 8 == 0) && f0 + 8 <= Co) {
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (wr >= 0) {
          v = *(const bf16x8*)&((const short*)Wt)[(long)wr * Co + f0];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          lds_bt[sswz64(f0 + j, kk & ~7) + (kk & 7)] = v[j];
      } else {
        for (int j = 0; j < 8 && f0 + j < 64; ++j) {
          const int f = f0 + j;
          short v = 0;
          if (f < Co && wr >= 0) {
            v = ((const short*)Wt)[(long)wr * Co + f];
          }
          lds_bt[sswz64(f, kk & ~7) + (kk & 7)] = v;
        }
      }
    }
    __syncthreads();

    // fragments + MFMA (2 K-slices, 2 row-halves per wave)
#pragma unroll
    for (int ksl = 0; ksl < SBK / 32; ++ksl) {
      bf16x8 a0 = *(const bf16x8*)&lds_a[sswz64(wave * 32 + fr, ksl * 32 + fk * 8)];
      bf16x8 a1 = *(const bf16x8*)&lds_a[sswz64(wave * 32 + 16 + fr, ksl * 32 + fk * 8)];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (nt < ntiles) {
          bf16x8 b = *(const bf16x8*)&lds_bt[sswz64(nt * 16 + fr, ksl * 32 + fk * 8)];
          acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[0][nt], 0, 0, 0);
          acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[1][nt], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // all waves done reading before next-step staging
  }

  // epilogue: C/D layout col = lane&15, row = (lane>>4)*4 + j
  bf16* Dt = D + (long)t * NB * Hd * Wd * Co;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    if (nt >= ntiles) break;
    const int col = nt * 16 + fr;
    if (col >= Co) continue;
    const float bv = bias ? bias[(long)t * Co + col] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 32 + hh * 16 + fk * 4 + j;
      if (row_n[row] >= 0) {
        ((short*)Dt)[(long)row_pix[row] * Co + col] =
            (short)__bfloat16_as_short(__float2bfloat16(acc[hh][nt][j] + bv));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad kernel: dWacc[t][n=9C][f] += sum_k dY[t,k,f] * im2col_s2(X)[t,k,n]
// Block: 256 thr = 4 waves; wave w owns n-subtile w (16 cols), iterates
// m-tiles over F.  K-chunked grid.
//   dY [T, NB, Ho, Wo, F] bf16 ; X [T, NB, H, W, C] bf16
// DET=true: each (t, K-chunk) block writes a PRIVATE accumulator slice
// (plain stores, no atomics); DET=false: fp32 atomicAdd fast path.
// ---------------------------------------------------------------------------
template <bool DET>
__global__ __launch_bounds__(256, 2)
void sconv_wgrad_kernel(const bf16* __restrict__ dY, const bf16* __restrict__ X,
                        float* __restrict__ dWacc,  // [T, nsl, 9C, F]
                        float* __restrict__ dBacc,  // [T, nsl, F] or nullptr
                        int NB, int H, int W, int C,
                        int Ho, int Wo, int F, int pad, int kchunk) {
  const int t = blockIdx.z;
  const int n0 = blockIdx.x * SWGN;        // column block within 9C
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  const long kchunk0 = (long)blockIdx.y * kchunk;
  const long kchunk_end = min(kchunk0 + (long)kchunk, Ktot);
  const int mtiles = (F + 15) / 16;

  __shared__ short lds_at[64 * SWBK];    // dY^T tile: [f][k], swizzled
  __shared__ short lds_bt[SWGN * SWBK];  // im2col^T tile: [n][k], swizzled
  __shared__ int ntab_dy[SWGN], ntab_dx[SWGN], ntab_c[SWGN];
  __shared__ int ktab_n[SWBK], ktab_h[SWBK], ktab_w[SWBK];  // k -> input base
  __shared__ float db_lds[4][64];

  // n-table (once): n -> (ky, kx, c)
  for (int e = threadIdx.x; e < SWGN; e += blockDim.x) {
    const int n = n0 + e;
    if (n < N9) {
      const int kyx = n / C;
      ntab_c[e] = n - kyx * C;
      ntab_dy[e] = kyx / 3;
      ntab_dx[e] = kyx % 3;
    } else {
      ntab_c[e] = -1;
    }
  }

  const bf16* dYt = dY + (long)t * Ktot * F;
  const bf16* Xt = X + (long)t * NB * H * W * C;

  const int wave = threadIdx.x / WAVE;      // n-subtile
  const int lane = threadIdx.x % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;

  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};
  // fused bias-grad: only the n0==0 column block accumulates (the dY tile
  // is identical across column blocks)
  const bool do_bias = (dBacc != nullptr) && (blockIdx.x == 0);
  float db_acc = 0.f;
  const int db_f = threadIdx.x & 63;
  const int db_q = threadIdx.x >> 6;        // k-range slice (4 x 16)

  for (long k0 = kchunk0; k0 < kchunk_end; k0 += SWBK) {
    __syncthreads();
    // k-position table: output position -> stride-2 input base coordinate
    if (threadIdx.x < SWBK) {
      const long k = k0 + threadIdx.x;
      if (k < kchunk_end) {
        const int wo = (int)(k % Wo);
        const long r = k / Wo;
        ktab_w[threadIdx.x] = 2 * wo - pad;
        ktab_h[threadIdx.x] = 2 * (int)(r % Ho) - pad;
        ktab_n[threadIdx.x] = (int)(r / Ho);
      } else {
        ktab_n[threadIdx.x] = -1;
      }
    }
    __syncthreads();
    // stage dY^T: slot s -> (kk = s>>3, f0 = (s&7)*8); rows f >= F of the
    // fragment tiles are zero-filled
    for (int s = threadIdx.x; s < SWBK * 8; s += blockDim.x) {
      const int kk = s >> 3;
      const int f0 = (s & 7) * 8;
      if (f0 >= mtiles * 16) continue;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ktab_n[kk] >= 0) {
        if ((F % 8 == 0) && f0 + 8 <= F) {
          v = *(const bf16x8*)&((const short*)dYt)[(k0 + kk) * F + f0];
        } else {
          for (int j = 0; j < 8; ++j)
            if (f0 + j < F) v[j] = ((const short*)dYt)[(k0 + kk) * F + f0 + j];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        lds_at[sswz64(f0 + j, kk & ~7) + (kk & 7)] = v[j];
    }
    // stage im2col^T: vector fast path when the 8-column run stays inside
    // one (ky,kx) slice; scalar otherwise
    for (int s = threadIdx.x; s < SWBK * (SWGN / 8); s += blockDim.x) {
      const int kk = s / (SWGN / 8);
      const int n8 = (s % (SWGN / 8)) * 8;
      const int nimg = ktab_n[kk];
      const int c0 = ntab_c[n8];
      const int c7 = ntab_c[n8 + 7];
      const bool vec_ok = (C % 8 == 0) && c0 >= 0 && c7 == c0 + 7;
      if (vec_ok) {
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (nimg >= 0) {
          const int h = ktab_h[kk] + ntab_dy[n8];
          const int w = ktab_w[kk] + ntab_dx[n8];
          if (h >= 0 && h < H && w >= 0 && w < W) {
            v = *(const bf16x8*)&(
                (const short*)Xt)[(((long)nimg * H + h) * W + w) * C + c0];
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          lds_bt[sswz64(n8 + j, kk & ~7) + (kk & 7)] = v[j];
      } else {
        for (int j = 0; j < 8; ++j) {
          const int ncol = n8 + j;
          const int c = ntab_c[ncol];
          short v = 0;
          if (nimg >= 0 && c >= 0) {
            const int h = ktab_h[kk] + ntab_dy[ncol];
            const int w = ktab_w[kk] + ntab_dx[ncol];
            if (h >= 0 && h < H && w >= 0 && w < W) {
              v = ((const short*)Xt)[(((long)nimg * H + h) * W + w) * C + c];
            }
          }
          lds_bt[sswz64(ncol, kk & ~7) + (kk & 7)] = v;
        }
      }
    }
    __syncthreads();

#pragma unroll
    for (int ks = 0; ks < SWBK / 32; ++ks) {
      bf16x8 b = *(const bf16x8*)&lds_bt[sswz64(wave * 16 + fr, ks * 32 + fk * 8)];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        if (mt < mtiles) {
          bf16x8 a = *(const bf16x8*)&lds_at[sswz64(mt * 16 + fr, ks * 32 + fk * 8)];
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[mt], 0, 0, 0);
        }
      }
    }
    if (do_bias && db_f < F) {
#pragma unroll
      for (int kk = db_q * 16; kk < db_q * 16 + 16; ++kk) {
        db_acc += __bfloat162float(__hip_bfloat16(__hip_bfloat16_raw{
            (unsigned short)lds_at[sswz64(db_f, kk & ~7) + (kk & 7)]}));
      }
    }
  }
  if (do_bias) {
    db_lds[db_q][db_f] = db_acc;
    __syncthreads();
    if (db_q == 0 && db_f < F) {
      const float v = db_lds[0][db_f] + db_lds[1][db_f] + db_lds[2][db_f] +
                      db_lds[3][db_f];
      if (DET) {
        dBacc[((long)t * gridDim.y + blockIdx.y) * F + db_f] = v;
      } else {
        atomicAdd(&dBacc[(long)t * F + db_f], v);
      }
    }
  }

  // accumulate: C/D col = lane&15 (n within wave tile), row = fk*4+j (f);
  // n-columns are disjoint across blockIdx.x, so under DET the private
  // (t, K-chunk) slice needs no atomics at all
  float* dWt = DET ? dWacc + ((long)t * gridDim.y + blockIdx.y) * N9 * F
                   : dWacc + (long)t * N9 * F;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    if (mt >= mtiles) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = mt * 16 + fk * 4 + j;
      const int n = n0 + wave * 16 + fr;
      if (f < F && n < N9) {
        if (DET) {
          dWt[(long)n * F + f] = acc[mt][j];
        } else {
          atomicAdd(&dWt[(long)n * F + f], acc[mt][j]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
namespace {
long sconv_out_dim(long h, long pad) { return (h + 2 * pad - 3) / 2 + 1; }
}  // namespace

// w [T, F, C, 3, 3] -> [T, 9, C, F] (fwd) or [T, 9, F, C] (dgrad) bf16
torch::Tensor sconv_repack(torch::Tensor w, bool dgrad) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 5 && w.size(3) == 3 && w.size(4) == 3);
  auto wc = w.contiguous().to(torch::kFloat32);
  const int T = (int)w.size(0), F = (int)w.size(1), C = (int)w.size(2);
  auto wp = torch::empty({T, 9, dgrad ? F : C, dgrad ? C : F},
                         w.options().dtype(torch::kBFloat16));
  auto stream = at::cuda::getCurrentCUDAStream();
  const long total = (long)T * F * C * 9;
  hipLaunchKernelGGL(sconv_repack_kernel, dim3(ew_grid(total)), dim3(256),
                     0, stream.stream(), wc.data_ptr<float>(),
                     reinterpret_cast<bf16*>(wp.data_ptr()), T, F, C, dgrad);
  return wp;
}

// x [T, NB, H, W, C] bf16 ; wp [T, 9, C, F] ; bias [T, F] fp32 / undef
// -> y [T, NB, Ho, Wo, F] bf16
torch::Tensor sconv_fwd(torch::Tensor x, torch::Tensor wp,
                        c10::optional<torch::Tensor> bias, long pad) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "sconv_fwd needs bf16");
  TORCH_CHECK(wp.is_contiguous() && wp.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(pad == 0 || pad == 1, "sconv: pad must be 0 or 1");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int F = (int)wp.size(3);
  TORCH_CHECK(wp.size(0) == T && wp.size(1) == 9 && wp.size(2) == C);
  TORCH_CHECK(C <= 64 && F <= 64, "sconv: C, F must be <= 64");
  TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3, "sconv: input too small");
  const long Ho = sconv_out_dim(H, pad), Wo = sconv_out_dim(W, pad);
  auto y = torch::empty({T, NB, Ho, Wo, F}, x.options());
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous().to(torch::kFloat32);
    TORCH_CHECK(bc.numel() == (long)T * F);
    bptr = bc.data_ptr<float>();
  }
  const long Mtot = (long)NB * Ho * Wo;
  dim3 grid((unsigned)((Mtot + SBM - 1) / SBM), T, 1);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((sconv_mm_kernel<false>), grid, dim3(512), 0,
                     stream.stream(),
                     reinterpret_cast<const bf16*>(x.data_ptr()),
                     reinterpret_cast<const bf16*>(wp.data_ptr()), bptr,
                     reinterpret_cast<bf16*>(y.data_ptr()),
                     NB, H, W, C, (int)Ho, (int)Wo, F, (int)pad);
  return y;
}

// dy [T, NB, Ho, Wo, F] bf16 ; wp [T, 9, F, C] (sconv_repack dgrad)
// -> dx [T, NB, H, W, C] bf16.  H, W are explicit: two input sizes map to
// the same Ho under stride 2.
torch::Tensor sconv_dgrad(torch::Tensor dy, torch::Tensor wp, long pad,
                          long H, long W) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 5 && dy.is_contiguous());
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16, "sconv_dgrad needs bf16");
  TORCH_CHECK(wp.is_contiguous() && wp.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(pad == 0 || pad == 1, "sconv: pad must be 0 or 1");
  const int T = (int)dy.size(0), NB = (int)dy.size(1), Ho = (int)dy.size(2),
            Wo = (int)dy.size(3), F = (int)dy.size(4);
  const int C = (int)wp.size(3);
  TORCH_CHECK(wp.size(0) == T && wp.size(1) == 9 && wp.size(2) == F);
  TORCH_CHECK(C <= 64 && F <= 64, "sconv: C, F must be <= 64");
  TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3 &&
              sconv_out_dim(H, pad) == Ho && sconv_out_dim(W, pad) == Wo,
              "sconv_dgrad: (H, W) inconsistent with dy");
  auto dx = torch::empty({T, NB, H, W, C}, dy.options());
  // largest parity class: ceil(H/2) x ceil(W/2) pixels per image
  const long Msub = (long)NB * ((H + 1) / 2) * ((W + 1) / 2);
  dim3 grid((unsigned)((Msub + SBM - 1) / SBM), T, 4);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((sconv_mm_kernel<true>), grid, dim3(512), 0,
                     stream.stream(),
                     reinterpret_cast<const bf16*>(dy.data_ptr()),
                     reinterpret_cast<const bf16*>(wp.data_ptr()), nullptr,
                     reinterpret_cast<bf16*>(dx.data_ptr()),
                     NB, Ho, Wo, F, (int)H, (int)W, C, (int)pad);
  return dx;
}

// dy [T, NB, Ho, Wo, F] bf16 ; x [T, NB, H, W, C] bf16
// -> {dw [T, F, C, 3, 3] fp32, db [T, F] fp32}
std::vector<torch::Tensor> sconv_wgrad(torch::Tensor dy, torch::Tensor x,
                                       long pad, bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.dim() == 5 && x.dim() == 5);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
              x.scalar_type() == torch::kBFloat16, "sconv_wgrad needs bf16");
  TORCH_CHECK(pad == 0 || pad == 1, "sconv: pad must be 0 or 1");
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3), F = (int)dy.size(4);
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == NB);
  TORCH_CHECK(C <= 64 && F <= 64, "sconv: C, F must be <= 64");
  TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3 &&
              sconv_out_dim(H, pad) == Ho && sconv_out_dim(W, pad) == Wo,
              "sconv_wgrad: dy inconsistent with x");
  const bool det = deterministic_mode();
  // K-chunks sized so the grid has >= ~1024 blocks, as tconv_wgrad's.
  // MAML355_DETERMINISTIC: private per-(t, K-chunk) slices, summed in fixed
  // order by the finalize kernel -> bitwise reproducible
  const wgplan::Plan p = wgplan::sconv(T, NB, Ho, Wo, C, det);
  auto acc = torch::zeros({T, p.nslices, 9 * C, F},
                          x.options().dtype(torch::kFloat32));
  auto dbacc = torch::zeros({T, p.nslices, F},
                            x.options().dtype(torch::kFloat32));
  dim3 grid((unsigned)p.gridx, (unsigned)p.gridy, T);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_SWGRAD(DET_)                                                    \
  hipLaunchKernelGGL((sconv_wgrad_kernel<DET_>), grid, dim3(256), 0,           \
                     stream.stream(),                                          \
                     reinterpret_cast<const bf16*>(dyc.data_ptr()),            \
                     reinterpret_cast<const bf16*>(xc.data_ptr()),             \
                     acc.data_ptr<float>(),                                    \
                     with_bias ? dbacc.data_ptr<float>() : nullptr,            \
                     NB, H, W, C, Ho, Wo, F, (int)pad, p.kchunk)
  if (det) LAUNCH_SWGRAD(true); else LAUNCH_SWGRAD(false);
#undef LAUNCH_SWGRAD
  return finish_wgrad(acc, dbacc, T, F, C, p.nslices, stream.stream());
}
