// Address logic of the LDS-staged first-layer forward (dconv_fwd_v3_kernel
// in dconv.hip), shared between the kernel and a host-side checker
// (tests/host/dconv_fwd_v3_addr_check.cpp): everything here compiles as
// plain C++ so the index arithmetic is walked under ASan/UBSan on the CPU.
//
// Per task the output is NL = NB*Ho lines of Wo positions.  A chunk is R
// consecutive lines (the last chunk of a task may be shorter); it may cross
// image boundaries.  The chunk's input is staged in LDS as rows of the
// zero-PADDED images [Hp = H + 2 pad][Wp = W + 2 pad][C]: staged row 0 is
// padded row ho0 of image img0 (the chunk's first line), staged row r is
// padded row (ho0 + r) % Hp of image img0 + (ho0 + r) / Hp.  Output line
// (img, ho) reads padded rows ho .. ho+2 of its image, and Hp - Ho = 2, so
// line l of the chunk starts at staged row l + 2 * (images crossed).  The
// halo (left/right columns, rows above and below an image, images past the
// task's last) is written as zeros: a window read needs no predicate.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFV3_HD __host__ __device__ inline
#else
#define DFV3_HD inline
#endif

namespace maml355 {
namespace dfv3 {

constexpr int kThreads = 256;            // block size: 4 waves
constexpr int kTile = 16;                // positions per MFMA tile
constexpr int kStep = 4 * kTile;         // positions a wave advances per tile
constexpr int kNLD = 9;                  // staging loads per thread per chunk
constexpr int kCap = kNLD * kThreads;    // elements (2 bytes) per LDS buffer
constexpr int kChunkMin = 336;           // positions per chunk: at least about
constexpr int kChunkMax = 1024;          // 21 tiles, at most 64

struct Geom {
  int NB, H, W, C, pad;
  int Ho, Wo, Hp, RS;    // RS = Wp * C: elements per staged row
  int NL;                // NB * Ho output lines per task
  int R;                 // lines per chunk; 0: the shape does not fit
  int nchunks;           // per task
  int rows;              // staged rows per chunk
  unsigned mRS, mHp, mHo;  // multiply-high reciprocals
  // a wave's step of kStep positions: lines, columns, LDS base
  int dwo, dho, dA, wrapA;
};

// ceil(2^32 / d): umulhi(n, magic(d)) == n / d whenever n * d <= 2^32
DFV3_HD unsigned magic(int d) {
  return (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d);
}
DFV3_HD int udiv(int n, unsigned m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)__umulhi((unsigned)n, m);
#else
  return (int)(((unsigned long long)(unsigned)n * m) >> 32);
#endif
}

// staged rows R lines can need: R + 2, plus 2 per image boundary crossed
DFV3_HD int staged_rows(int R, int Ho) {
  return R + 2 + 2 * ((R - 1 + Ho - 1) / Ho);
}

// R is the most lines whose staged rows fit kCap, up to kChunkMax positions;
// where that leaves a task fewer than want_chunks chunks (a small launch)
// it comes down to as few as kChunkMin positions
DFV3_HD Geom make_geom(int NB, int H, int W, int C, int pad, int want_chunks) {
  Geom g;
  g.NB = NB; g.H = H; g.W = W; g.C = C; g.pad = pad;
  g.Ho = H + 2 * pad - 2; g.Wo = W + 2 * pad - 2;
  g.Hp = H + 2 * pad; g.RS = (W + 2 * pad) * C;
  g.NL = NB * g.Ho;
  int R = kChunkMax / g.Wo;
  if (R < 1) R = 1;
  if (R > g.NL) R = g.NL;
  while (R >= 1 && (long)staged_rows(R, g.Ho) * g.RS > kCap) --R;
  const int Rmin = (kChunkMin + g.Wo - 1) / g.Wo;
  while (R > Rmin && (g.NL + R - 1) / R < want_chunks) --R;
  g.R = R < 1 ? 0 : R;
  g.nchunks = g.R ? (g.NL + g.R - 1) / g.R : 0;
  g.rows = g.R ? staged_rows(g.R, g.Ho) : 0;
  g.mRS = magic(g.RS); g.mHp = magic(g.Hp); g.mHo = magic(g.Ho > 1 ? g.Ho : 2);
  const int dl = kStep / g.Wo;
  g.dwo = kStep - dl * g.Wo;
  const int dimg = dl / g.Ho;
  g.dho = dl - dimg * g.Ho;
  g.dA = (dl + 2 * dimg) * g.RS + g.dwo * C;
  g.wrapA = g.RS - g.Wo * C;
  return g;
}

// first line of chunk ck
struct Chunk { int L0, img0, ho0; };
DFV3_HD Chunk chunk_at(const Geom& g, int ck) {
  Chunk c;
  c.L0 = ck * g.R;
  c.img0 = c.L0 / g.Ho;
  c.ho0 = c.L0 - c.img0 * g.Ho;
  return c;
}

// Staging: LDS element slot s of a chunk that starts at (img0, ho0) ->
// element offset into the task's x, or -1 for a zero (halo, an image past
// the task's last, a slot past the staged rows).  img0 >= NB gives all zeros.
DFV3_HD int slot_src(const Geom& g, int img0, int ho0, int s) {
  const int row = udiv(s, g.mRS);
  const int col = s - row * g.RS;
  const int rel = ho0 + row;
  const int irel = udiv(rel, g.mHp);
  const int h = rel - irel * g.Hp - g.pad;
  const int img = img0 + irel;
  const int cw = col - g.pad * g.C;
  const bool ok = row < g.rows && img < g.NB && (unsigned)h < (unsigned)g.H &&
                  (unsigned)cw < (unsigned)(g.W * g.C);
  return ok ? ((img * g.H + h) * g.W) * g.C + cw : -1;
}

// Window reads: LDS element offset = base(position) + k_off(k).
// k = (ky*3 + kx)*C + c, the MFMA's reduction index.
DFV3_HD int k_off(const Geom& g, int k) {
  const int tap = k / g.C, c = k - tap * g.C;
  const int dy = tap / 3, dx = tap - dy * 3;
  return (dy * g.RS + dx * g.C) + c;
}

// a lane's position inside a chunk: column, line of its image, LDS base
struct LanePos { int wo, ho, ab; };

// position q = l * Wo + wo of a chunk whose first line is ho0 of its image;
// (l, wo) is a per-lane constant for q < kStep, so the kernel divides once
DFV3_HD LanePos lane_init(const Geom& g, int ho0, int l, int wo) {
  LanePos p;
  const int rel = ho0 + l;
  const int cross = g.Ho > 1 ? udiv(rel, g.mHo) : rel;
  p.wo = wo;
  p.ho = rel - cross * g.Ho;
  p.ab = (l + 2 * cross) * g.RS + wo * g.C;
  return p;
}

// advance by kStep positions with adds and compares: after the column carry
// ho <= Ho, plus dho <= Ho - 1, so one conditional subtract restores ho < Ho
DFV3_HD void lane_advance(const Geom& g, LanePos& p) {
  p.wo += g.dwo;
  p.ab += g.dA;
  if (p.wo >= g.Wo) { p.wo -= g.Wo; p.ho += 1; p.ab += g.wrapA; }
  p.ho += g.dho;
  if (p.ho >= g.Ho) { p.ho -= g.Ho; p.ab += 2 * g.RS; }
}

}  // namespace dfv3
}  // namespace maml355
