// Split-K plan of the wgrad GEMM launchers (tconv.hip, wgrad_nt.hip,
// sconv.hip, fconv.hip): K-chunk length, grid, number of private slices and
// 64- or 128-column blocks.  Plain C++, no HIP and no torch, reads no
// environment: tests/host/wgrad_plan_check.cpp pins and sweeps it on the CPU.
//
// Per task the GEMM is dW[n][f] = sum_k im2col(X)[k][n] * dY[k][f] with
// n < 9C columns and k < NB*Ho*Wo positions.  blockIdx.x walks the columns,
// blockIdx.y the K-chunks, blockIdx.z the tasks.  On the atomic path every
// K-chunk adds into one accumulator (nslices == 1); on the ordered paths
// (MAML355_DETERMINISTIC=1, and fp32 always) each K-chunk owns a private
// slice and a finalize kernel sums the slices in chunk order.
#pragma once

namespace maml355 {
namespace wgplan {

constexpr int kCols = 64;            // columns per block and per NSUB
constexpr int kStep = 64;            // K-step of the bf16 kernels
constexpr int kStepF32 = 32;         // K-step of fconv_wgrad_kernel
constexpr long kBlocks = 1024;       // grid the chunks are sized for
constexpr long kBlocksF32 = 3072;
constexpr long kAtomicCap = 4096;    // longest K-chunk on the atomic path
constexpr long kNoCap = 0;

// v2's operand transposes are fixed cost: below this many positions per
// task the v1 gather kernel wins (hip_autograd.py routes on the same number)
constexpr long kV2MinPositions = 30000;
// 128-column blocks: v2 from this padded reduction length, v3 from this
// many positions over all tasks (profiles/README.md)
constexpr long kV2WideMinKr = 131072;
constexpr long kV3WideMinTK = 600000;

enum Bias { kBiasNone = 0, kBiasOnes = 1, kBiasColsum = 2 };

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }
inline long round_up(long a, long b) { return ceil_div(a, b) * b; }

struct Chunks { int kchunk, gridy, nslices; };

// Cut a reduction of `klen` positions into K-chunks, multiples of `kstep`,
// so that the grid has about `target` blocks; `blocks_xz` is the column
// grid times T.  A cap marks the atomic path (one shared accumulator);
// without one every chunk gets its own slice.
inline Chunks chunks(long klen, long blocks_xz, int kstep, long target,
                     long cap = kNoCap) {
  const long per_y = blocks_xz > 1 ? blocks_xz : 1;
  const long desired_y = target / per_y > 1 ? target / per_y : 1;
  long kchunk = round_up(ceil_div(klen, desired_y), kstep);
  if (kchunk < kstep) kchunk = kstep;
  if (cap != kNoCap && kchunk > cap) kchunk = cap;
  const int gridy = (int)ceil_div(klen, kchunk);
  return {(int)kchunk, gridy, cap != kNoCap ? 1 : gridy};
}

struct Plan {
  int nsub;       // 64-column sub-tiles per block: 1 or 2
  int gridx;      // column blocks
  int Wk;         // line width of the reduction index (Wo, or Wo padded to 8)
  long Kr;        // reduction length the K-chunks cover
  int bias;       // Bias; v3 only
  int kchunk, gridy, nslices;
};

inline Plan with_chunks(Plan p, const Chunks& c) {
  p.kchunk = c.kchunk; p.gridy = c.gridy; p.nslices = c.nslices;
  return p;
}

// 64 or 128 columns per block: `wide` is the measured default, 9C <= 64
// never goes wide, MAML355_WGRAD_NSUB (0 = unset, 1, 2) overrides for A/B.
inline int pick_nsub(int N9, bool wide, int nsub_override) {
  if (nsub_override == 1) return 1;
  if (nsub_override == 2) return N9 > kCols ? 2 : 1;
  return N9 > kCols && wide ? 2 : 1;
}

// tconv_wgrad (v1 gather kernel) and, with stride-2 Ho/Wo, sconv_wgrad:
// flat reduction index, 64-column blocks.
inline Plan v1(int T, int NB, int Ho, int Wo, int C, bool det) {
  Plan p{};
  p.nsub = 1;
  p.gridx = (int)ceil_div(9 * C, kCols);
  p.Wk = Wo;
  p.Kr = (long)NB * Ho * Wo;
  return with_chunks(p, chunks(p.Kr, (long)p.gridx * T, kStep, kBlocks,
                               det ? kNoCap : kAtomicCap));
}

inline Plan sconv(int T, int NB, int Ho, int Wo, int C, bool det) {
  return v1(T, NB, Ho, Wo, C, det);
}

// tconv_wgrad_v2: every line of the reduction index padded to 8 positions,
// the whole rounded up to the K-step.
inline Plan v2(int T, int NB, int Ho, int Wo, int C, bool det,
               int nsub_override) {
  Plan p{};
  p.Wk = (int)round_up(Wo, 8);
  p.Kr = round_up((long)NB * Ho * p.Wk, kStep);
  p.nsub = pick_nsub(9 * C, p.Kr >= kV2WideMinKr, nsub_override);
  p.gridx = (int)ceil_div(9 * C, kCols * p.nsub);
  return with_chunks(p, chunks(p.Kr, (long)p.gridx * T, kStep, kBlocks,
                               det ? kNoCap : kAtomicCap));
}

// tconv_wgrad_v3.  C is the stored channel count; the kernel sees the first
// layer's C in {1, 3} padded to 8.  Deterministic mode keeps, bit for bit,
// the sums of the routing v3 replaced — v2 from kV2MinPositions up (if v2 is
// on), v1 below — so it takes that plan's line width and its K-chunks.
inline Plan v3(int T, int NB, int Ho, int Wo, int C, bool with_bias, bool det,
               bool v2_on, int nsub_override) {
  const bool as_v2 = det && (long)NB * Ho * Wo >= kV2MinPositions && v2_on;
  Plan p{};
  p.Wk = as_v2 ? (int)round_up(Wo, 8) : Wo;
  p.Kr = round_up((long)NB * Ho * p.Wk, kStep);
  const int N9 = 9 * (C % 8 == 0 ? C : 8);
  p.nsub = pick_nsub(N9, (long)T * p.Kr >= kV3WideMinTK, nsub_override);
  p.gridx = (int)ceil_div(N9, kCols * p.nsub);
  // a spare column in the last block carries the bias as a column of ones;
  // the deterministic orders sum the dY tile's columns instead, as v2 and v1
  p.bias = !with_bias ? kBiasNone
           : (!det && p.gridx * kCols * p.nsub > N9) ? kBiasOnes
                                                     : kBiasColsum;
  if (det) {
    const Plan old = as_v2 ? v2(T, NB, Ho, Wo, C, true, nsub_override)
                           : v1(T, NB, Ho, Wo, C, true);
    return with_chunks(p, {old.kchunk, old.gridy, old.nslices});
  }
  return with_chunks(p, chunks(p.Kr, (long)p.gridx * T, kStep, kBlocks,
                               kAtomicCap));
}

// fconv_wgrad: always ordered private slices, no cap, sized for more blocks.
inline Plan fconv(int T, int NB, int Ho, int Wo, int C) {
  Plan p{};
  p.nsub = 1;
  p.gridx = (int)ceil_div(9 * C, kCols);
  p.Wk = Wo;
  p.Kr = (long)NB * Ho * Wo;
  return with_chunks(p, chunks(p.Kr, (long)p.gridx * T, kStepF32,
                               kBlocksF32));
}

}  // namespace wgplan
}  // namespace maml355
