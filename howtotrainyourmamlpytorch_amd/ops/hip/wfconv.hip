// Wide-channel fp32 task-batched stride-1 3x3 convolution trio (fwd / dgrad /
// wgrad) on v_mfma_f32_16x16x4_f32 — the backend that takes over where
// fconv.hip stops (64 channels), with fconv.hip's contract:
//
//   fwd   : Y[t]  = im2col(X[t])  @ Wp[t]       M=NB*Ho*Wo, N=Co, K=9*Ci
//   dgrad : dX[t] = im2col(dY[t]) @ Wp_flip[t]  (SAME kernel; weights
//           repacked flipped+transposed, im2col pad' = 2 - pad)
//   wgrad : dW[t] = dY[t]^T @ im2col(X[t])      split-K over positions,
//           private slice per K-chunk + ordered finalize, db fused
//
// Activations [T, NB, H, W, C] fp32, weights [T, F, C, 3, 3] fp32 used
// UNROUNDED, bias [T, F] fp32, all outputs fp32.  C and F are any value in
// 1..256 (the dispatch sends max(C, F) <= 64 to fconv.hip): nothing needs
// channel alignment, C % 4 == 0 and F % 4 == 0 only select 16-byte gathers
// over scalar ones, and the first layer's C in {1, 3} runs as it is stored.
// The weight repack is fconv_repack (a pure permutation, no channel cap).
//
// Why this is not wconv.hip with another element type.  The fp32 MFMA runs
// at 1/16 of the bf16 rate (fconv.hip's header), so an MFMA spent on padding
// is the first-order cost and staging traffic is not.  wconv.hip pays two
// such paddings: its K-step stays inside one tap (at Ci = 72 three steps of
// 32 per tap, a quarter of the MFMAs on zeros), and its column tile is a
// fixed 128 split 2 x 2 over the waves (at Co = 72 or 96 half or a quarter of
// the tile is empty, and the waves of the empty half idle).  Here
//   * K is flat, K9 = 9*Ci walked in 32-wide steps across tap boundaries;
//     only the last step has a tail (K9 = 648: 20.25 steps, 1.2 % padding),
//   * the waves split M only: wave w owns rows [32w, 32w+32) times ALL of the
//     block's columns, so a ragged column count costs every wave the same,
//   * the column blocks are even: nblk = ceil(Co/128) blocks of
//     16 * ceil(Co / (16*nblk)) columns (72 -> one block of 80, 136 -> two of
//     80, 256 -> two of 128), the tile count NT a template parameter.
// The pipelining is fconv.hip's plain one: both tiles go through registers
// between two barriers, bounds-checked loads that yield 0 outside the image,
// past the M and K tails and past Co, and the global loads of K-step k+1
// issued before the MFMAs of step k.  No floating-point atomics anywhere:
// every reduction order is fixed, so all three ops are bitwise run-to-run
// reproducible in every mode.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=
// kernel-resource-usage; VGPRs + AGPRs, LDS bytes, scratch bytes, waves/SIMD):
//   wfconv_mm_kernel<1>      96 +  0   20736   0   5
//   wfconv_mm_kernel<2>     120 +  0   23040   0   4
//   wfconv_mm_kernel<3>     148 +  0   25344   0   3
//   wfconv_mm_kernel<4>     148 +  0   27648   0   3
//   wfconv_mm_kernel<5>     164 +  0   29952   0   3
//   wfconv_mm_kernel<6>     212 +  0   32256   0   2
//   wfconv_mm_kernel<7>     228 +  0   34560   0   2
//   wfconv_mm_kernel<8>     252 +  0   36864   0   2
//   wfconv_wgrad_kernel<1>  117 +  0   37376   0   4
//   wfconv_wgrad_kernel<2>  125 +  0   37376   0   4
//   wfconv_wgrad_kernel<3>  134 +  0   37376   0   3
//   wfconv_wgrad_kernel<4>  141 +  0   37376   0   3
//   wfconv_wgrad_kernel<5>  149 +  0   37376   0   3
//   wfconv_wgrad_kernel<6>  157 +  0   37376   0   3
//   wfconv_wgrad_kernel<7>  166 +  0   37376   0   3
//   wfconv_wgrad_kernel<8>  172 +  0   37376   0   2
//   wfconv_wgrad_finalize    23 +  0       0   0   8
// No spills; the compile emits no packed-fp32 VALU instruction in this file.
// v_mfma_f32_32x32x2_f32 (same rate, fewer LDS reads per flop) is not used:
// its 32-wide tiles would bring back the column padding this design removes.

#include "common.h"
#include "wgrad_plan.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

// One plain v_add_f32.  The folds below add whole accumulators; written as
// vector adds the compiler pairs them into packed-fp32 adds, which this
// project does not emit.
DEVINL float add_f32(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// ---------------------------------------------------------------------------
// fwd / dgrad kernel.
//   X  [T, NB, H, W, Ci] ; Wp [T, 9, Ci, Co] ; bias [T, Co] or nullptr
//   Y  [T, NB, Ho, Wo, Co]            pad = im2col pad (fwd p, dgrad 2-p)
//
// Block = 256 threads = 4 waves, tile MM_M = 128 positions x 16*NT columns,
// K-step MM_K = 32 of the flat K9.  Grid (ceil(M/128), nblk, T).  Wave w owns
// rows [32w, 32w+32) as two 16-row halves times the NT column tiles: 2 x NT
// independent accumulators (64 registers at NT = 8), and as many again for
// the totals the chains are folded into every MM_FOLD K-steps.
//
// Operand layout (fconv.hip's): both tiles k-contiguous in LDS, A as [m][k]
// and B transposed as [col][k], row stride MM_LD = 36 floats.  Lane group
// g = lane>>4 reads the four consecutive k  16*kb + 4*g + {0..3}  of its row
// with one ds_read_b128 and feeds element j to MFMA j of that 16-wide K
// block — the same permutation of k on both sides, so the product is
// unchanged.  Stride 36 puts the 16 rows of a lane group on the 16 distinct
// multiples of 4 (36 r mod 64): one b128 read covers the 64 banks once per
// 16 lanes.  Per 16-k block 2 A reads and NT B reads feed 8*NT MFMAs.
//
// Staging.  A: thread -> fixed k-quad (tid & 7) and rows tid>>3 + 32*i; its
// four row decodes live in registers for the whole K loop.  B: Wp rows are
// [k][Co], so a thread loads a 4 x 4 patch — k-quad tid & 7, column quad cq
// — as four 16-byte row loads (Co % 4 == 0) or sixteen scalars, transposes
// it in registers and writes four ds_write_b128, one per column.  cq is
// tid>>3 with its two low bits swapped: lanes 0..7 then write one tile row
// (banks 0..31) and lanes 8..15 the row 8 further (36*8 mod 64 = 32: banks
// 32..63), so the 16-byte B stores are conflict-free, where fconv.hip's
// scalar B stores are 4-way conflicted.
// ---------------------------------------------------------------------------
#define MM_M 128
#define MM_K 32
#define MM_LD (MM_K + 4)
#define MM_FOLD 8   // K-steps per closed accumulation chain (256 terms)

template <int NT>   // 16-column tiles of the block, compile-time so the MFMA
                     // loop has no branches and its LDS reads batch
// two waves per SIMD: the two accumulator sets of NT = 8 are 128 registers
__global__ __launch_bounds__(256, 2)
void wfconv_mm_kernel(const float* __restrict__ X, const float* __restrict__ Wp,
                      const float* __restrict__ bias, float* __restrict__ Y,
                      int NB, int H, int W, int Ci, int Ho, int Wo, int Co,
                      int pad) {
  const int t = blockIdx.z;
  const long Mtot = (long)NB * Ho * Wo;
  const long m0 = (long)blockIdx.x * MM_M;
  const int co0 = blockIdx.y * (16 * NT);
  const int K9 = 9 * Ci;
  const bool vec = (Ci % 4) == 0;
  const bool vecb = (Co % 4) == 0;

  __shared__ __attribute__((aligned(16))) float lds_a[MM_M * MM_LD];
  __shared__ __attribute__((aligned(16))) float lds_bt[16 * NT * MM_LD];

  const float* Xt = X + (long)t * NB * H * W * Ci;
  const float* Wt = Wp + (long)t * 9 * Ci * Co;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;

  // this thread's k-quad (both tiles) and its four A rows, decoded once
  const int kq = (tid & 7) * 4;
  int r_n[4], r_h[4], r_w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long mg = m0 + (tid >> 3) + 32 * i;
    if (mg < Mtot) {
      r_w[i] = (int)(mg % Wo);
      r_h[i] = (int)((mg / Wo) % Ho);
      r_n[i] = (int)(mg / ((long)Wo * Ho));
    } else {
      r_n[i] = -1; r_h[i] = 0; r_w[i] = 0;
    }
  }
  // B staging: column quad with the two low bits of tid>>3 swapped
  const int bu = tid >> 3;
  const int b_c = 4 * ((bu & ~3) | ((bu & 1) << 1) | ((bu >> 1) & 1));
  const bool b_on = b_c < 16 * NT;   // = (tid >> 5) < NT: half-wave uniform

  f32x4 acc[2][NT], tot[2][NT];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      acc[hh][i] = {0.f, 0.f, 0.f, 0.f};
      tot[hh][i] = {0.f, 0.f, 0.f, 0.f};
    }
  int steps = 0;

  // global -> register half of the staging for the K-step at k0 (k >= K9
  // loads nothing and stages zeros)
  f32x4 va[4];
  f32x4 vb[4];   // vb[j] = column b_c + j, k = kq .. kq + 3
  auto load_step = [&](int k0) {
    // ---- A (im2col gather)
    if (vec) {
      // Ci % 4 == 0: the quad k..k+3 is 4 consecutive channels of one tap,
      // 16-byte aligned; K9 % 4 == 0, so the quad is valid as a whole
      const int k = k0 + kq;
      const int kyx = k / Ci;
      const int c0 = k - kyx * Ci;
      const int dy = kyx / 3 - pad, dx = kyx % 3 - pad;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int h = r_h[i] + dy, w = r_w[i] + dx;
        if (k < K9 && r_n[i] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
          v = *(const f32x4*)&Xt[(((long)r_n[i] * H + h) * W + w) * Ci + c0];
        }
        va[i] = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) va[i] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + kq + j;
        if (k < K9) {
          const int kyx = k / Ci;
          const int c = k - kyx * Ci;
          const int dy = kyx / 3 - pad, dx = kyx % 3 - pad;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int h = r_h[i] + dy, w = r_w[i] + dx;
            if (r_n[i] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
              va[i][j] = Xt[(((long)r_n[i] * H + h) * W + w) * Ci + c];
            }
          }
        }
      }
    }
    // ---- B: rows k of Wp are contiguous [Co]; 4 x 4 patch, transposed here
    if (b_on) {
      const int col = co0 + b_c;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int k = k0 + kq + jj;
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (k < K9) {
          const float* src = Wt + (long)k * Co + col;
          if (vecb) {
            // Co % 4 == 0: the four columns are valid together
            if (col < Co) r = *(const f32x4*)src;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (col + j < Co) r[j] = src[j];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) vb[j][jj] = r[j];
      }
    }
  };
  load_step(0);
  for (int k0 = 0; k0 < K9; k0 += MM_K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(f32x4*)&lds_a[((tid >> 3) + 32 * i) * MM_LD + kq] = va[i];
    }
    if (b_on) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *(f32x4*)&lds_bt[(b_c + j) * MM_LD + kq] = vb[j];
      }
    }
    __syncthreads();
    // prefetch: the next K-step's global loads fly under this step's MFMAs
    load_step(k0 + MM_K);

#pragma unroll
    for (int kb = 0; kb < MM_K / 16; ++kb) {
      const int kc = kb * 16 + fk * 4;
      const f32x4 a0 = *(const f32x4*)&lds_a[(wave * 32 + fr) * MM_LD + kc];
      const f32x4 a1 = *(const f32x4*)&lds_a[(wave * 32 + 16 + fr) * MM_LD + kc];
      // column tiles two at a time: 8 registers of B fragments live, 4
      // independent accumulators per group (4 MFMAs = 128 cycles between two
      // uses of one accumulator, against 40 of dependent latency); with all
      // NT fragments live NT = 8 spilled
#pragma unroll
      for (int n0 = 0; n0 < NT; n0 += 2) {
        constexpr int kGroup = 2;
        f32x4 b[kGroup];
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
          if (n0 + g < NT)
            b[g] = *(const f32x4*)&lds_bt[((n0 + g) * 16 + fr) * MM_LD + kc];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int g = 0; g < kGroup; ++g) {
            if (n0 + g < NT) {
              acc[0][n0 + g] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  a0[j], b[g][j], acc[0][n0 + g], 0, 0, 0);
              acc[1][n0 + g] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  a1[j], b[g][j], acc[1][n0 + g], 0, 0, 0);
            }
          }
        }
      }
    }
    // blocked accumulation: every MM_FOLD K-steps the chain is closed and
    // added to the total, so no fmaf chain is longer than 256 terms (one
    // chain over K9 = 864 measured 1.6 times the RMS error of the library
    // conv against float64; a fixed order all the same)
    if ((++steps & (MM_FOLD - 1)) == 0) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            tot[hh][nt][e] = add_f32(tot[hh][nt][e], acc[hh][nt][e]);
          acc[hh][nt] = {0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();  // all waves done reading before the next staging
  }
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        acc[hh][nt][e] = add_f32(tot[hh][nt][e], acc[hh][nt][e]);

  // epilogue: C/D layout col = lane&15, row = (lane>>4)*4 + j; bias added
  float* Yt = Y + (long)t * Mtot * Co;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = co0 + nt * 16 + fr;
      if (col >= Co) continue;
      const float bv = bias ? bias[(long)t * Co + col] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long mg = m0 + wave * 32 + hh * 16 + fk * 4 + j;
        if (mg < Mtot) Yt[mg * Co + col] = acc[hh][nt][j] + bv;
      }
    }
}

// ---------------------------------------------------------------------------
// wgrad kernel: slice[t][chunk][n = 9C][f] = sum over the chunk's positions
// k of dY[t,k,f] * im2col(X)[t,k,n];  dbslice[t][chunk][f] = sum_k dY.
//   dY [T, NB, Ho, Wo, F] ; X [T, NB, H, W, C]
// Block = 256 threads = 4 waves over a WG_N = 128-column block of 9C and an
// F block of 16*MT <= 128 rows (F blocks even, as the column blocks of the
// mm kernel: fblk = ceil(F/128) blocks of 16 * ceil(F / (16*fblk)) rows).
// The waves split the columns only: wave w owns columns [32w, 32w+32) as two
// 16-column tiles times the MT row tiles — MT x 2 accumulators, 64 registers
// at MT = 8 — so a ragged F costs every wave the same.  Column tiles past 9C
// (last column block only) are skipped per wave.  Grid (F blocks * column
// blocks, K-chunks, T), blockIdx.x = column block * fblk + F block, which is
// wgplan::wconv's grid; every (t, chunk) block stores a PRIVATE slice with
// plain stores and wfconv_wgrad_finalize_kernel sums the slices in chunk
// order — no atomics, one path in every mode.
//
// Both tiles are staged AS STORED, position-major: dY tile [k][f] and im2col
// tile [k][n], WG_K = 32 positions per K-step, 16-byte writes.  The
// reduction index is the LDS row, so each MFMA operand is one ds_read_b32
// (per 4-position block 2 B reads and MT A reads feed 2*MT MFMAs: 0.625
// reads per MFMA at MT = 8, against fconv_wgrad's 1.25).  Row stride: a read
// touches the four rows 4ks + (lane>>4) at 16 consecutive columns, banks
// (S*r + base + c) mod 64 for r = 0..3, c = 0..15; the 64 lanes cover the 64
// banks once iff S*r mod 64 runs over {0, 16, 32, 48}, i.e. S mod 64 is 16
// or 48.  The tile is 128 floats wide and 128 = 0 (mod 64) would be a 4-way
// conflict, so WG_LD = 128 + 16 = 144 (= 16 mod 64; 576-byte rows keep the
// 16-byte writes aligned).  LDS 2 x 32 x 144 x 4 B = 36 KB.
// Staging: thread -> fixed column quad (tid & 31) of both tiles, its (tap,
// channel) decode done once, and rows tid>>5 + 8*i, whose (wo, ho, image)
// advance by 32 positions per K-step with carries.  The global loads of
// K-step k+1 are issued before the MFMAs of step k.  The bias gradient is the
// ordered column sum of the staged dY tiles, from column block 0 only.
// ---------------------------------------------------------------------------
#define WG_N 128
#define WG_K 32
#define WG_LD 144
static_assert(WG_K == wgplan::kStepWide && WG_N == wgplan::kTileWide,
              "wgrad_plan.h cuts K-chunks for these tiles");

// the MFMAs of one K-step for NN live column tiles of this wave
template <int MT, int NN>
DEVINL void wfconv_wgrad_step(const float* lds_a, const float* lds_b,
                              f32x4 (&acc)[MT][2], int fk, int fr, int ncol) {
#pragma unroll
  for (int ks = 0; ks < WG_K / 4; ++ks) {
    const int row = (ks * 4 + fk) * WG_LD + fr;
    float b[NN];
#pragma unroll
    for (int nt = 0; nt < NN; ++nt) b[nt] = lds_b[row + ncol + nt * 16];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const float a = lds_a[row + mt * 16];
#pragma unroll
      for (int nt = 0; nt < NN; ++nt) {
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[nt], acc[mt][nt],
                                                           0, 0, 0);
      }
    }
  }
}

template <int MT>   // 16-row tiles of the F block, compile-time (as NT)
// two waves per SIMD: without the bound MT = 8 took 171 VGPRs + 92 AGPRs and
// one wave per SIMD; with it the accumulators stay in VGPRs (172, no AGPRs)
__global__ __launch_bounds__(256, 2)
void wfconv_wgrad_kernel(const float* __restrict__ dY,
                         const float* __restrict__ X,
                         float* __restrict__ dWsl,  // [T, nsl, 9C, F]
                         float* __restrict__ dBsl,  // [T, nsl, F] or nullptr
                         int NB, int H, int W, int C, int Ho, int Wo, int F,
                         int pad, int kchunk, int fblk) {
  const int t = blockIdx.z;
  const int fb = blockIdx.x % fblk;
  const int nb = blockIdx.x / fblk;
  const int f0 = fb * (16 * MT);
  const int n0 = nb * WG_N;
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  const long kc0 = (long)blockIdx.y * kchunk;
  const long kc_end = min(kc0 + (long)kchunk, Ktot);
  const bool vecx = (C % 4) == 0;
  const bool vecf = (F % 4) == 0;

  __shared__ __attribute__((aligned(16))) float lds_a[WG_K * WG_LD];  // dY  [k][f]
  __shared__ __attribute__((aligned(16))) float lds_b[WG_K * WG_LD];  // col [k][n]
  __shared__ float db_lds[WG_N];

  const float* dYt = dY + (long)t * Ktot * F;
  const float* Xt = X + (long)t * NB * H * W * C;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;
  // this wave's two column tiles (wave-uniform)
  const bool live0 = n0 + wave * 32 < N9;
  const bool live1 = n0 + wave * 32 + 16 < N9;

  // this thread's column quad of both tiles, decoded once: n -> (tap, c)
  const int q4 = (tid & 31) * 4;
  const int sr = tid >> 5;
  const bool a_on = q4 < 16 * MT;   // dY columns of this F block
  int q_dy[4], q_dx[4], q_c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + q4 + j;
    if (n < N9) {
      const int kyx = n / C;
      q_c[j] = n - kyx * C;
      q_dy[j] = kyx / 3 - pad;
      q_dx[j] = kyx % 3 - pad;
    } else {
      q_c[j] = -1; q_dy[j] = 0; q_dx[j] = 0;
    }
  }

  f32x4 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // fused bias grad: the dY tile is the same in every column block, so only
  // column block 0 sums it; thread -> column tid & 127, rows 16 * (tid>>7)..
  const bool do_bias = (dBsl != nullptr) && (nb == 0);
  float db_acc = 0.f, db_blk = 0.f;
  int db_steps = 0;
  const int db_f = tid & 127;
  const int db_h = tid >> 7;

  // The four staging rows of this thread advance by WG_K positions per
  // K-step: decode (wo, ho, img) once, then step it with carries.  dho < Ho
  // and one carry keep ho below 2 * Ho.
  const int s_dwo = WG_K % Wo;
  const int s_dho = (WG_K / Wo) % Ho;
  const int s_dimg = (WG_K / Wo) / Ho;
  int p_k[4], p_wo[4], p_ho[4], p_img[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = (int)kc0 + sr + 8 * i;
    p_k[i] = k;
    p_wo[i] = k % Wo;
    p_ho[i] = (k / Wo) % Ho;
    p_img[i] = (k / Wo) / Ho;
  }
  // global -> register half of the staging for the next K-step; rows past
  // the chunk end load nothing and stage zeros
  f32x4 vy[4], vx[4];
  auto load_step = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long k = p_k[i];
      f32x4 y4 = {0.f, 0.f, 0.f, 0.f}, x4 = {0.f, 0.f, 0.f, 0.f};
      if (k < kc_end) {
        if (a_on) {
          // dY row k, columns f0 + q4 .. + 3
          const int f = f0 + q4;
          const float* src = dYt + k * F + f;
          if (vecf) {
            if (f < F) y4 = *(const f32x4*)src;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (f + j < F) y4[j] = src[j];
          }
        }
        const int wo = p_wo[i], ho = p_ho[i];
        const long img = p_img[i];
        if (vecx) {
          // C % 4 == 0: the quad is 4 consecutive channels of one tap
          const int h = ho + q_dy[0], w = wo + q_dx[0];
          if (q_c[0] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
            x4 = *(const f32x4*)&Xt[((img * H + h) * W + w) * C + q_c[0]];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int h = ho + q_dy[j], w = wo + q_dx[j];
            if (q_c[j] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
              x4[j] = Xt[((img * H + h) * W + w) * C + q_c[j]];
            }
          }
        }
      }
      vy[i] = y4;
      vx[i] = x4;
      // advance this row to the next K-step
      p_k[i] += WG_K;
      p_wo[i] += s_dwo;
      const int cw = p_wo[i] >= Wo;
      p_wo[i] -= cw ? Wo : 0;
      p_ho[i] += s_dho + cw;
      const int ch = p_ho[i] >= Ho;
      p_ho[i] -= ch ? Ho : 0;
      p_img[i] += s_dimg + ch;
    }
  };

  load_step();
  for (long k0 = kc0; k0 < kc_end; k0 += WG_K) {
    __syncthreads();  // previous K-step's reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(f32x4*)&lds_a[(sr + 8 * i) * WG_LD + q4] = vy[i];
      *(f32x4*)&lds_b[(sr + 8 * i) * WG_LD + q4] = vx[i];
    }
    __syncthreads();
    // prefetch: the next K-step's global loads fly under this step's MFMAs
    load_step();

    if (live1) {
      wfconv_wgrad_step<MT, 2>(lds_a, lds_b, acc, fk, fr, wave * 32);
    } else if (live0) {
      wfconv_wgrad_step<MT, 1>(lds_a, lds_b, acc, fk, fr, wave * 32);
    }
    if (do_bias) {
      // blocked sum, fixed order: a pairwise tree over the step's 16 rows,
      // eight steps to a block, the blocks into db_acc.  db of a conv in
      // front of a batch norm is a sum that cancels to zero, so what comes
      // out is its rounding error: one serial chain over the chunk measured
      // 3 to 4 times the RMS error of a pairwise sum.
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = lds_a[(db_h * 16 + i) * WG_LD + db_f];
#pragma unroll
      for (int w = 8; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) v[i] = add_f32(v[2 * i], v[2 * i + 1]);
      db_blk += v[0];
      if ((++db_steps & 7) == 0) {
        db_acc += db_blk;
        db_blk = 0.f;
      }
    }
  }
  if (do_bias) {  // block-uniform
    db_acc += db_blk;
    if (db_h == 1) db_lds[db_f] = db_acc;
    __syncthreads();
    // columns past 16*MT belong to the next F block
    if (db_h == 0 && db_f < 16 * MT && f0 + db_f < F) {
      dBsl[((long)t * gridDim.y + blockIdx.y) * F + f0 + db_f] =
          db_acc + db_lds[db_f];
    }
  }

  // C/D: col = lane&15 (n within the tile), row = fk*4+j (f).  Tiles are
  // disjoint, so the (t, chunk) slice is written exactly once.
  float* dWt = dWsl + ((long)t * gridDim.y + blockIdx.y) * N9 * F;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = n0 + wave * 32 + nt * 16 + fr;
    if (n >= N9) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int f = f0 + mt * 16 + fk * 4;
      if (vecf) {
        // F % 4 == 0: the four rows stand together, one 16-byte store
        if (f < F) *(f32x4*)&dWt[(long)n * F + f] = acc[mt][nt];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (f + j < F) dWt[(long)n * F + f + j] = acc[mt][nt][j];
      }
    }
  }
}

// slices [T, nsl, 9C, F] -> dW [T, F, C, 3, 3]; dbsl [T, nsl, F] -> db [T, F].
// Slices are summed in chunk order: the one, fixed reduction order.
__global__ void wfconv_wgrad_finalize_kernel(const float* __restrict__ sl,
                                             const float* __restrict__ dbsl,
                                             float* __restrict__ dw,
                                             float* __restrict__ db,
                                             int T, int F, int C, int nsl) {
  const long total = (long)T * F * C * 9;
  const long ssz = (long)9 * C * F;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = first; i < total; i += grid_stride()) {
    long r = i;
    const int kx = (int)(r % 3); r /= 3;
    const int ky = (int)(r % 3); r /= 3;
    const int c = (int)(r % C); r /= C;
    const int f = (int)(r % F); r /= F;
    const long t = r;
    const long e = ((long)(ky * 3 + kx) * C + c) * F + f;
    float v = 0.f;
    for (int s = 0; s < nsl; ++s) v += sl[(t * nsl + s) * ssz + e];
    dw[i] = v;
  }
  if (dbsl) {
    for (long i = first; i < (long)T * F; i += grid_stride()) {
      const long t = i / F;
      const int f = (int)(i % F);
      float v = 0.f;
      for (int s = 0; s < nsl; ++s) v += dbsl[(t * nsl + s) * F + f];
      db[i] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
// even blocks: `n` channels in ceil(n/128) blocks of `tiles` 16-wide tiles
static int wfconv_tiles(int n) {
  const int nblk = (n + 127) / 128;
  return (n + 16 * nblk - 1) / (16 * nblk);
}

// x [T, NB, H, W, Ci] fp32 ; wp [T, 9, Ci, Co] fp32 (fconv_repack) ;
// bias [T, Co] fp32 / undef
torch::Tensor wfconv_mm(torch::Tensor x, torch::Tensor wp,
                        c10::optional<torch::Tensor> bias, long pad,
                        long Ho, long Wo) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kFloat32, "wfconv_mm needs fp32");
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.is_contiguous() &&
              wp.scalar_type() == torch::kFloat32 && wp.size(1) == 9 &&
              wp.device() == x.device());
  TORCH_CHECK(x.size(0) <= 65535, "wfconv_mm: at most 65535 tasks (grid.z)");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), Ci = (int)x.size(4);
  const int Co = (int)wp.size(3);
  TORCH_CHECK(wp.size(0) == T && wp.size(2) == Ci, "wp does not match x");
  TORCH_CHECK(Ci >= 1 && Ci <= 256 && Co >= 1 && Co <= 256,
              "wfconv_mm: channels must be in 1..256");
  TORCH_CHECK(pad >= 0 && pad <= 2 && Ho == H + 2 * pad - 2 &&
              Wo == W + 2 * pad - 2 && Ho >= 1 && Wo >= 1,
              "wfconv_mm: output size does not match the im2col pad");
  auto y = torch::empty({T, NB, Ho, Wo, Co}, x.options());
  const long Mtot = (long)NB * Ho * Wo;
  if (T == 0 || Mtot == 0) return y;
  // positions are decoded and the row grid is cut in 32 bits; every global
  // offset is carried as 64-bit
  TORCH_CHECK(Mtot < (1L << 30) && (long)NB * H * W < (1L << 30),
              "wfconv_mm: too many positions per task");
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == torch::kFloat32 &&
                bias->numel() == (long)T * Co);
    bc = bias->contiguous();
    bptr = bc.data_ptr<float>();
  }
  const int nt = wfconv_tiles(Co);
  dim3 grid((unsigned)((Mtot + MM_M - 1) / MM_M),
            (unsigned)((Co + 16 * nt - 1) / (16 * nt)), T);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_WFMM(NT_)                                                       \
  case NT_:                                                                    \
    hipLaunchKernelGGL((wfconv_mm_kernel<NT_>), grid, dim3(256), 0,            \
                       stream.stream(), x.data_ptr<float>(),                   \
                       wp.data_ptr<float>(), bptr, y.data_ptr<float>(), NB, H, \
                       W, Ci, (int)Ho, (int)Wo, Co, (int)pad);                 \
    break
  switch (nt) {
    LAUNCH_WFMM(1); LAUNCH_WFMM(2); LAUNCH_WFMM(3); LAUNCH_WFMM(4);
    LAUNCH_WFMM(5); LAUNCH_WFMM(6); LAUNCH_WFMM(7); LAUNCH_WFMM(8);
    default: TORCH_CHECK(false, "wfconv_mm: no instantiation for ", nt, " tiles");
  }
#undef LAUNCH_WFMM
  return y;
}

// The split-K plan wfconv_wgrad cuts for a shape: {kchunk, chunks}.
std::vector<long> wfconv_wgrad_plan(long T, long NB, long Ho, long Wo, long C,
                                    long F) {
  const wgplan::Plan p =
      wgplan::wconv((int)T, (int)NB, (int)Ho, (int)Wo, (int)C, (int)F);
  return {p.kchunk, p.gridy};
}

// dy [T, NB, Ho, Wo, F] fp32 ; x [T, NB, H, W, C] fp32
// -> {dw [T, F, C, 3, 3] fp32, db [T, F] fp32 (zeros unless with_bias)}
std::vector<torch::Tensor> wfconv_wgrad(torch::Tensor dy, torch::Tensor x,
                                        long pad, bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.dim() == 5 && x.dim() == 5 &&
              dy.device() == x.device());
  TORCH_CHECK(dy.scalar_type() == torch::kFloat32 &&
              x.scalar_type() == torch::kFloat32, "wfconv_wgrad needs fp32");
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  TORCH_CHECK(x.size(0) <= 65535, "wfconv_wgrad: at most 65535 tasks (grid.z)");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3), F = (int)dy.size(4);
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == NB, "dy does not match x");
  TORCH_CHECK(C >= 1 && C <= 256 && F >= 1 && F <= 256,
              "wfconv_wgrad: channels must be in 1..256");
  TORCH_CHECK(pad >= 0 && pad <= 2 && Ho == H + 2 * pad - 2 &&
              Wo == W + 2 * pad - 2 && Ho >= 1 && Wo >= 1,
              "wfconv_wgrad: dy size does not match the pad");
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  // positions are stepped in 32 bits; every global offset is 64-bit
  TORCH_CHECK(Ktot < (1L << 30) && (long)NB * H * W < (1L << 30),
              "wfconv_wgrad: too many positions per task");
  auto fopts = x.options();
  auto dw = torch::empty({T, F, C, 3, 3}, fopts);
  auto db = torch::zeros({T, F}, fopts);
  if (T == 0 || Ktot == 0) return {dw.zero_(), db};
  const wgplan::Plan p = wgplan::wconv(T, NB, Ho, Wo, C, F);
  const int nsl = p.nslices;
  const int mt = wfconv_tiles(F);
  const int fblk = (F + 16 * mt - 1) / (16 * mt);
  TORCH_CHECK(nsl >= 1 && nsl <= 65535 &&
                  p.gridx == fblk * ((N9 + WG_N - 1) / WG_N),
              "wfconv_wgrad: plan does not match the tiles");
  auto sl = torch::empty({T, nsl, N9, F}, fopts);
  auto dbsl = torch::empty({T, nsl, F}, fopts);
  dim3 grid((unsigned)p.gridx, (unsigned)nsl, T);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_WFWG(MT_)                                                       \
  case MT_:                                                                    \
    hipLaunchKernelGGL((wfconv_wgrad_kernel<MT_>), grid, dim3(256), 0,         \
                       stream.stream(), dyc.data_ptr<float>(),                 \
                       xc.data_ptr<float>(), sl.data_ptr<float>(),             \
                       with_bias ? dbsl.data_ptr<float>() : nullptr, NB, H, W, \
                       C, Ho, Wo, F, (int)pad, p.kchunk, fblk);                \
    break
  switch (mt) {
    LAUNCH_WFWG(1); LAUNCH_WFWG(2); LAUNCH_WFWG(3); LAUNCH_WFWG(4);
    LAUNCH_WFWG(5); LAUNCH_WFWG(6); LAUNCH_WFWG(7); LAUNCH_WFWG(8);
    default: TORCH_CHECK(false, "wfconv_wgrad: no instantiation for ", mt, " tiles");
  }
#undef LAUNCH_WFWG
  const long total = (long)T * F * C * 9;
  hipLaunchKernelGGL(wfconv_wgrad_finalize_kernel, dim3(ew_grid(total)),
                     dim3(256), 0, stream.stream(), sl.data_ptr<float>(),
                     with_bias ? dbsl.data_ptr<float>() : nullptr,
                     dw.data_ptr<float>(), db.data_ptr<float>(), T, F, C, nsl);
  return {dw, db};
}
