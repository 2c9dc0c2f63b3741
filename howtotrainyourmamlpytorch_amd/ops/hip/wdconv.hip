// First-layer forward for the wide backbones: bf16 3x3 conv of a C in {1, 3}
// image into 65..256 filters, stride 1 or 2, the whole reduction in ONE
// v_mfma_f32_16x16x32_bf16 per 16-position x 16-channel tile.
//
//   x    [T, NB, H, W, C] bf16, as stored (no channel pad)
//   w    [T, F, C, 3, 3] fp32, bias [T, F] fp32 (optional)
//   y    [T, NB, Ho, Wo, F] bf16;  stride 1: Ho = H + 2p - 2;  stride 2:
//        Ho = (H + 2p - 3) / 2 + 1 (swconv.hip's geometry: odd H with p = 1
//        reads iy = H on the last line, so all four edges are out of range)
//
// Numerics contract = wconv.hip: weights rounded to bf16 once by the repack,
// fp32 MFMA accumulation, bias added in fp32, one rounding at the store.  No
// atomics, no data-dependent order: bitwise repeatable.
//
// K = 9C <= 27 fits one 32-wide K-step.  wdconv_repack writes the weights as
// [T, 64*NG, 32] bf16 rows, k = (ky*3 + kx)*C + c, zeros for k >= 9C and for
// the rows past F.  With that k order the 3C values of one ky are one
// contiguous run of an NHWC image row, starting at (wo*stride)*C of the padded
// row.  C = 1 (K = 9) is zero-filled to 32 as well rather than sent to the
// 16-wide-K instruction: the kernel is bound by its stores (below), the MFMA
// pipe is by an estimate from instruction counts (no counter run) under a
// third busy at 32, and the 16-wide instruction has another
// operand layout (4 k per lane), i.e. a second fragment assembler and a
// second set of instantiations to save time nobody waits for.
//
// Work split: a block (4 waves) works on one task and walks chunks of R
// output lines (wdconv_addr.h).  The waves split the POSITIONS of a chunk
// (16-position tiles, wave w takes tiles w, w+4, ..); every wave holds the
// weight fragments of ALL F channels in registers for the block's lifetime:
// 4 VGPRs per 16-channel tile, 64 at F = 256 (the bias lies in LDS, 4 bytes a
// channel, staged once per block).  Splitting the columns instead
// would quarter that, but every wave would then assemble every position
// fragment (4x the LDS reads), and a wave's stores would be 64-channel
// slivers of many lines; with the positions split a wave's tile is one
// contiguous 16 * 2F-byte piece of y.  Only four accumulators (one 64-channel
// group) are live at a time.
//
// x goes through LDS.  A chunk's rows of the zero-padded images are staged
// once, halo as zeros (left/right columns, rows above/below an image, images
// past the task's last; stride 2 stages 2R + 1 rows for R lines).  The
// position fragment (lane: position lane&15, k = 8*(lane>>4) .. +7) is eight
// unpredicated ds_read_u16 at base(position) + k_off(k), packed in pairs and
// masked for k >= 9C.  The next chunk's rows are loaded to registers at the
// top of a chunk and written to the other buffer after the wave's first tile:
// the tile loop itself waits on no global load.  One barrier per chunk.
//
// The store is the floor, so it is built for whole lines.  The MFMA takes the
// weight fragment as its row operand: a lane holds 4 channels (rows 4*(lane>>4)
// + e) of one position (lane&15).  Plain tiles would give an 8-byte store, a
// wave instruction writing 16 lines x 32 bytes.  Two steps change that:
//   1. the weight rows are permuted (wdc::tile_channel): tiles 2h, 2h+1 of a
//      64-channel group leave lane group gq the 8 consecutive channels
//      32h + 8gq .. +7 — 16 bytes per lane, the four lanes of a position
//      64 contiguous bytes.  No data moves: only which weight row a lane loads.
//   2. one DPP row_ror:8 exchange per dword between positions p and p + 8:
//      lanes p < 8 give away their upper half (channels 32..63) and lanes
//      p >= 8 their lower one.  After it lane (p, gq) holds channels
//      32*(p>>3) + 8gq .. +7 of positions p&7 and (p&7) + 8.
// Each of the two global_store_dwordx4 of a group then writes, for 8
// positions, 8 lanes x 16 bytes = the position's whole 128-byte run of the
// group (aligned to 128 where F % 64 == 0).  4 + 4 v_cndmask and 4 DPP moves
// per 64 channels; no LDS round trip.
//
// Tails: rows past F are zero weights and their stores are masked per lane
// (F % 8 == 0: an 8-channel piece is whole or absent); a half group past F
// is skipped wave-uniformly (F = 72: group 1 runs two of its four MFMAs).
// Positions past the chunk read staged slot 0.. and store nothing.
//
// Resources (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage); LDS is
// the two 8 KB x buffers plus 256 * NG bytes of bias; <NG, STRIDE>,
// NG = ceil(F / 64):
//
//   kernel                      VGPRs  AGPRs  SGPRs  LDS bytes  waves/SIMD
//   wdconv_fwd_kernel<2, 1>      176      8     90      16896           2
//   wdconv_fwd_kernel<2, 2>      177      8     90      16896           2
//   wdconv_fwd_kernel<3, 1>      194      8     96      17152           2
//   wdconv_fwd_kernel<3, 2>      195      8     96      17152           2
//   wdconv_fwd_kernel<4, 1>      210      8    102      17408           2
//   wdconv_fwd_kernel<4, 2>      211      8    102      17408           2
//   wdconv_repack_kernel          24      0     38          0           8
//
// Scratch 0 bytes, no VGPR spill and no SGPR spill in any instantiation; two
// blocks share a CU at every F.  The bias is what made that so: held in
// registers in accumulator layout (16 per 64 channels, loaded with 16 * NG
// scattered scalar loads per thread) it took NG = 4 to 256 VGPRs + 46 AGPRs
// and one block per CU, with 2 and 6 SGPRs kept in VGPR lanes at NG = 3 and
// 4.  It now lies in LDS and is read per tile (the empty asm in the tile
// keeps the compiler from hoisting those reads back into 16 * NG registers).
// __launch_bounds__(256) is the block size: one wave per SIMD per block.
// The per-slot staging predicates are folded into one compare (slot_static /
// slot_dyn): held as 16 lane masks they alone spilled 60 SGPRs.

#include "common.h"
#include "wdconv_addr.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4;

// two floats -> one dword of two bf16 (lo: a, hi: b), round to nearest even
DEVINL unsigned pack_bf16(float a, float b) {
  const unsigned lo = __hip_bfloat16_raw(__float2bfloat16(a)).x;
  const unsigned hi = __hip_bfloat16_raw(__float2bfloat16(b)).x;
  return lo | (hi << 16);
}

// lane i of a 16-lane row reads lane (i + 8) % 16 of it
DEVINL unsigned row_ror8(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
}

}  // namespace

// w [T, F, C, 3, 3] fp32 -> wp [T, FP, 32] bf16, k = (ky*3 + kx)*C + c
__global__ void wdconv_repack_kernel(const float* __restrict__ w,
                                     short* __restrict__ wp, int T, int F,
                                     int C, int FP) {
  const long total = (long)T * FP * 32;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int k = (int)(i & 31);
    const int f = (int)((i >> 5) % FP);
    const long t = (i >> 5) / FP;
    float v = 0.f;
    if (f < F && k < 9 * C) {
      const int tap = k / C, c = k - tap * C;
      v = w[((t * F + f) * C + c) * 9 + tap];
    }
    wp[i] = (short)__hip_bfloat16_raw(__float2bfloat16(v)).x;
  }
}

template <int NG, int STRIDE>
__global__ __launch_bounds__(256)
void wdconv_fwd_kernel(const unsigned short* __restrict__ X,
                       const short* __restrict__ Wp,
                       const float* __restrict__ bias, short* __restrict__ Y,
                       const wdc::Geom geom, int F) {
  wdc::Geom g = geom;
  g.S = STRIDE;  // compile-time in the address arithmetic
  __shared__ unsigned short xs[2][wdc::kCap];
  __shared__ __attribute__((aligned(16))) float bs[64 * NG];
  const int t = blockIdx.y;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int lane = tid % WAVE;
  const int p = lane & 15;   // weights: row of a tile; x, D: position in tile
  const int gq = lane >> 4;  // weights, x: k / 8; D: 4-row group
  const long Mtot = (long)g.NL * g.Wo;

  const unsigned short* Xt = X + (long)t * g.NB * g.H * g.W * g.C;
  const short* Wt = Wp + (long)t * (64 * NG) * 32;
  short* Yt = Y + Mtot * F * t;

  // weight fragments: in registers for the block's lifetime.  The bias goes
  // to LDS once (one coalesced load per thread, zeros past F and without a
  // bias); the first barrier below publishes it
  bf16x8 wf[NG][4];
#pragma unroll
  for (int q = 0; q < NG; ++q)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      wf[q][nt] = *(const bf16x8*)&Wt[(64 * q + wdc::tile_channel(nt, p)) * 32 +
                                      8 * gq];
  if (tid < 64 * NG)
    bs[tid] = (bias != nullptr && tid < F) ? bias[(long)t * F + tid] : 0.f;

  // per-lane k decode (once): LDS offsets of this lane's 8 k, pair masks
  int koff[8];
  unsigned pm[4];
#pragma unroll
  for (int j = 0; j < 8; ++j) koff[j] = wdc::k_off(g, 8 * gq + j);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = 8 * gq + 2 * i;
    pm[i] = (k < 9 * g.C ? 0xffffu : 0u) | (k + 1 < 9 * g.C ? 0xffff0000u : 0u);
  }
  // after the exchange this lane stores channels chb .. +7 of each group
  const bool lowp = p < 8;
  const int chb = 32 * (p >> 3) + 8 * gq;

  // staging: slot j*256 + tid.  Branch-free: every load is issued (a zero
  // slot reads element 0 of the task's x and is written as 0)
  unsigned short xr[wdc::kNLD];
  unsigned okm = 0;
  int sst[wdc::kNLD];  // the chunk-independent half of each slot's source
#pragma unroll
  for (int j = 0; j < wdc::kNLD; ++j)
    sst[j] = wdc::slot_static(g, j * wdc::kThreads + tid);
  auto stage_load = [&](int img0, int ho0) {
    okm = 0;
#pragma unroll
    for (int j = 0; j < wdc::kNLD; ++j) {
      const int off = wdc::slot_dyn(g, img0, ho0, sst[j]);
      okm |= (off >= 0 ? 1u : 0u) << j;
      xr[j] = Xt[off >= 0 ? off : 0];
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int j = 0; j < wdc::kNLD; ++j) {
      xs[buf][j * wdc::kThreads + tid] =
          (okm >> j) & 1 ? xr[j] : (unsigned short)0;
    }
  };

  int ck = blockIdx.x;
  if (ck >= g.nchunks) return;  // block-uniform, before any barrier
  wdc::Chunk ch = wdc::chunk_at(g, ck);
  stage_load(ch.img0, ch.ho0);
  stage_write(0);
  __syncthreads();

  for (int it = 0; ck < g.nchunks; ++it) {
    const int buf = it & 1;
    const unsigned short* xc = xs[buf];
    const int nlines = min(g.R, g.NL - ch.L0);
    const int npos = nlines * g.Wo;
    const long m0 = (long)ch.L0 * g.Wo;
    const int ho0 = ch.ho0;
    // next chunk of this block: its rows fly under this chunk's first tile
    const int nck = ck + gridDim.x;
    const bool more = nck < g.nchunks;
    wdc::Chunk nch = ch;
    if (more) {
      nch = wdc::chunk_at(g, nck);
      stage_load(nch.img0, nch.ho0);
    }

    // one 16-position tile starting at chunk position tq (wave-uniform)
    auto tile = [&](int tq) {
      const int q = tq + p;
      const int ab = q < npos ? wdc::pos_base(g, ho0, q) : 0;
      unsigned short e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = xc[ab + koff[j]];
      u32x4 ad;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        ad[i] = ((unsigned)e[2 * i] | ((unsigned)e[2 * i + 1] << 16)) & pm[i];
      const bf16x8 af = __builtin_bit_cast(bf16x8, ad);
      // the two positions this lane stores after the exchange
      const int qa = tq + (p & 7), qb = qa + 8;
#pragma unroll
      for (int q4 = 0; q4 < NG; ++q4) {
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          acc[nt] = {0.f, 0.f, 0.f, 0.f};
          if (64 * q4 + 32 * (nt >> 1) < F) {  // wave-uniform
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[q4][nt], af, acc[nt], 0, 0, 0);
          }
        }
        // bias in fp32, one rounding.  Accumulator nt holds channels
        // tile_channel(nt, 4gq + e): 8gq + 4(nt&1) + e of half nt>>1, so the
        // lane's 16 biases are two 32-byte runs of bs (a broadcast read per
        // lane group).  lo = channels 8gq .. +7, hi = 32 + 8gq .. +7
        int bo = 8 * gq;
        asm volatile("" : "+v"(bo));  // read per tile: hoisted out of the tile
                                      // loop the biases cost 16 VGPRs a group
        const float* bq = &bs[64 * q4 + bo];
        f32x4 sb[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          sb[nt] = acc[nt] + *(const f32x4*)&bq[32 * (nt >> 1) + 4 * (nt & 1)];
        unsigned lo[4], hi[4];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          lo[d] = pack_bf16(sb[0][2 * d], sb[0][2 * d + 1]);
          lo[2 + d] = pack_bf16(sb[1][2 * d], sb[1][2 * d + 1]);
          hi[d] = pack_bf16(sb[2][2 * d], sb[2][2 * d + 1]);
          hi[2 + d] = pack_bf16(sb[3][2 * d], sb[3][2 * d + 1]);
        }
        u32x4 o1, o2;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const unsigned recv = row_ror8(lowp ? hi[d] : lo[d]);
          o1[d] = lowp ? lo[d] : recv;
          o2[d] = lowp ? recv : hi[d];
        }
        const int cb = 64 * q4 + chb;
        if (cb < F) {
          if (qa < npos) *(u32x4*)&Yt[(m0 + qa) * F + cb] = o1;
          if (qb < npos) *(u32x4*)&Yt[(m0 + qb) * F + cb] = o2;
        }
      }
    };

    bool pending = more;  // the staged rows go to LDS after the first tile
    for (int tq = wave * wdc::kTile; tq < npos; tq += wdc::kStep) {
      tile(tq);
      if (pending) {
        stage_write(buf ^ 1);
        pending = false;
      }
    }
    if (pending) stage_write(buf ^ 1);
    __syncthreads();
    ck = nck;
    ch = nch;
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
namespace {

bool wd_aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

int wd_groups(long F) { return (int)((F + 63) / 64); }

}  // namespace

// w [T, F, C, 3, 3] fp32 -> [T, 64 * ceil(F / 64), 32] bf16
torch::Tensor wdconv_repack(torch::Tensor w) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 5 && w.size(3) == 3 && w.size(4) == 3 &&
              w.scalar_type() == torch::kFloat32, "wdconv_repack: w [T,F,C,3,3] fp32");
  auto wc = w.contiguous();
  const long T = w.size(0), F = w.size(1), C = w.size(2);
  TORCH_CHECK(C == 1 || C == 3, "wdconv_repack: C must be 1 or 3");
  TORCH_CHECK(F % 8 == 0 && F > 64 && F <= 256,
              "wdconv_repack: F must be a multiple of 8 in 72..256");
  const long FP = 64 * wd_groups(F);
  auto wp = torch::empty({T, FP, 32}, w.options().dtype(torch::kBFloat16));
  if (T == 0) return wp;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(wdconv_repack_kernel, dim3(ew_grid(T * FP * 32)), dim3(256),
                     0, stream.stream(), wc.data_ptr<float>(),
                     reinterpret_cast<short*>(wp.data_ptr()), (int)T, (int)F,
                     (int)C, (int)FP);
  return wp;
}

// Whether an H x W x C image's staged rows fit the LDS buffer (one output
// line's three rows: 3 * (S*(Wo-1) + 3) * C <= kCap, i.e. up to 453 columns at
// C = 3 and stride 1).  The routing asks this; wider images keep the
// pad-to-8 route.
bool wdconv_fits(long H, long W, long C, long pad, long stride) {
  if (!((C == 1 || C == 3) && (pad == 0 || pad == 1) &&
        (stride == 1 || stride == 2) && H + 2 * pad >= 3 && W + 2 * pad >= 3 &&
        H < (1L << 20) && W < (1L << 20)))
    return false;
  const wdc::Geom g =
      wdc::make_geom(1, 1, (int)H, (int)W, (int)C, (int)pad, (int)stride);
  return g.R >= 1 && g.nslots <= wdc::kCap;
}

// x [T, NB, H, W, C] bf16 ; wp = wdconv_repack(w) ; bias [T, F] fp32 / undef
// -> y [T, NB, Ho, Wo, F] bf16
torch::Tensor wdconv_fwd(torch::Tensor x, torch::Tensor wp,
                         c10::optional<torch::Tensor> bias, long F, long pad,
                         long stride) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "wdconv_fwd needs bf16");
  TORCH_CHECK(F % 8 == 0 && F > 64 && F <= 256,
              "wdconv_fwd: F must be a multiple of 8 in 72..256");
  const int NG = wd_groups(F);
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 3 && wp.is_contiguous() &&
              wp.scalar_type() == torch::kBFloat16 && wp.size(1) == 64 * NG &&
              wp.size(2) == 32 && wp.device() == x.device(),
              "wdconv_fwd: wp is not wdconv_repack's image for F");
  TORCH_CHECK(x.size(0) <= 65535, "wdconv_fwd: at most 65535 tasks (grid.y)");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  TORCH_CHECK(wp.size(0) == T, "wp does not match x");
  TORCH_CHECK(C == 1 || C == 3, "wdconv_fwd: C must be 1 or 3");
  TORCH_CHECK(pad == 0 || pad == 1, "wdconv_fwd: pad must be 0 or 1");
  TORCH_CHECK(stride == 1 || stride == 2, "wdconv_fwd: stride must be 1 or 2");
  TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3, "wdconv_fwd: input too small");
  const long Ho = wdc::out_dim(H, (int)pad, (int)stride);
  const long Wo = wdc::out_dim(W, (int)pad, (int)stride);
  auto y = torch::empty({T, NB, Ho, Wo, F}, x.options());
  const long Mtot = (long)NB * Ho * Wo;
  if (T == 0 || Mtot == 0) return y;
  // positions and x elements are indexed in 32 bits inside a task; every
  // global offset is carried as 64-bit
  TORCH_CHECK(Mtot < (1L << 30) && (long)NB * H * W * C < (1L << 31) &&
                  (long)NB * Ho * Ho <= (1L << 32),
              "wdconv_fwd: too many positions per task");
  TORCH_CHECK(wd_aligned16(wp) && wd_aligned16(y), "wdconv_fwd: 16-byte alignment");
  const wdc::Geom g = wdc::make_geom(T, NB, H, W, C, (int)pad, (int)stride);
  TORCH_CHECK(g.R >= 1 && g.nslots <= wdc::kCap,
              "wdconv_fwd: an output line's input rows do not fit the LDS buffer");
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == torch::kFloat32 &&
                bias->numel() == (long)T * F);
    bc = bias->contiguous();
    bptr = bc.data_ptr<float>();
  }
  const int gridx = wdc::grid_x(g, T);
  auto stream = at::cuda::getCurrentCUDAStream();
#define WDCONV_LAUNCH(NG_, S_)                                                 \
  hipLaunchKernelGGL((wdconv_fwd_kernel<NG_, S_>), dim3(gridx, T), dim3(256),  \
                     0, stream.stream(),                                       \
                     reinterpret_cast<const unsigned short*>(x.data_ptr()),    \
                     reinterpret_cast<const short*>(wp.data_ptr()), bptr,      \
                     reinterpret_cast<short*>(y.data_ptr()), g, (int)F)
  if (stride == 1) {
    if (NG == 2) WDCONV_LAUNCH(2, 1);
    else if (NG == 3) WDCONV_LAUNCH(3, 1);
    else WDCONV_LAUNCH(4, 1);
  } else {
    if (NG == 2) WDCONV_LAUNCH(2, 2);
    else if (NG == 3) WDCONV_LAUNCH(3, 2);
    else WDCONV_LAUNCH(4, 2);
  }
#undef WDCONV_LAUNCH
  return y;
}
