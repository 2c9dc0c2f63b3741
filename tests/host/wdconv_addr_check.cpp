// CPU check of the wide first-layer forward's address logic
// (howtotrainyourmamlpytorch_amd/ops/hip/wdconv_addr.h).  No GPU: built with
// -fsanitize=address,undefined and run by tests/test_wdconv_addr.py.
//
// Per shape and grid width it replays the kernel's walk: every block's
// chunks, every staging slot of every chunk, every wave's tiles, every window
// read, every store of the exchanged lane map.  It checks that
//  * the multiply-high divisions agree with the plain ones;
//  * every staged slot reads inside the task's x (really read from an array
//    of exactly that size, so ASan sees an overrun) or is a zero;
//  * every window read hits a slot this chunk wrote, and for a stored
//    position finds the value of the zero-padded strided 3x3 window, k in
//    (ky, kx, c) order; k >= 9C is masked;
//  * the permuted weight rows and the row_ror:8 exchange leave every
//    (position, channel < F) stored exactly once, each 16-byte store inside y,
//    and the 8 lanes of a position cover one contiguous 128-byte run.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wdconv_addr.h"

using namespace maml355::wdc;

static int g_fail = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__);      \
                         std::printf(__VA_ARGS__); std::printf("\n"); }        \
      ++g_fail;                                                                \
    }                                                                          \
  } while (0)

struct Shape { int T, NB, H, W, C, F, pad, S; };

// value of element e of the task's x: never 0, so a zero slot is told apart
static uint16_t xval(long e) { return (uint16_t)(1 + e % 65521); }

static void walk(const Shape& s, int gridx, bool range_only) {
  const Geom g = make_geom(s.T, s.NB, s.H, s.W, s.C, s.pad, s.S);
  CHECK(g.R >= 1 && g.nslots <= kCap, "shape does not fit");
  if (g.R < 1 || g.nslots > kCap) return;
  if (gridx <= 0) gridx = grid_x(g, s.T);
  gridx = std::min(gridx, g.nchunks);
  CHECK(gridx >= 1, "empty grid");
  CHECK(g.rows >= 3, "fewer than a window's rows");
  const long x_task = (long)s.NB * s.H * s.W * s.C;
  const long Mtot = (long)g.NL * g.Wo;
  CHECK(x_task < (1L << 31) && Mtot < (1L << 30), "launch checks");
  const int K = 9 * s.C, NG = (s.F + 63) / 64;
  std::vector<uint16_t> x(x_task);
  for (long e = 0; e < x_task; ++e) x[e] = xval(e);
  std::vector<uint8_t> stored(range_only ? 0 : Mtot * s.F, 0);

  std::vector<int> lds(2 * kCap);            // -2: never written; else value
  for (int bx = 0; bx < gridx; ++bx) {
    if (range_only && bx != 0 && bx != gridx - 1) continue;
    std::fill(lds.begin(), lds.end(), -2);
    auto stage = [&](const Chunk& c, int buf) {
      for (int j = 0; j < kNLD; ++j) {
        if (j * kThreads >= g.nslots) continue;
        for (int tid = 0; tid < kThreads; ++tid) {
          const int sl = j * kThreads + tid;
          CHECK(sl < kCap, "slot past the buffer");
          const int row = sl / g.RS, col = sl % g.RS;
          CHECK(udiv(sl, g.RS, g.mRS) == row, "udiv RS %d", sl);
          const int rel = s.S * c.ho0 + row;
          CHECK(udiv(rel, g.SR, g.mSR) == rel / g.SR, "udiv SR %d", rel);
          const int off = slot_src(g, c.img0, c.ho0, sl);
          const int img = c.img0 + rel / g.SR, hp = rel % g.SR;
          const int wp = col / s.C, ch = col % s.C;
          const bool inside = row < g.rows && img < s.NB && hp >= s.pad &&
                              hp < s.H + s.pad && wp >= s.pad && wp < s.W + s.pad;
          CHECK((off >= 0) == inside, "slot %d zero decision", sl);
          int v = 0;
          if (off >= 0) {
            const long want =
                (((long)img * s.H + (hp - s.pad)) * s.W + (wp - s.pad)) * s.C + ch;
            CHECK(off == want && off < x_task, "slot %d off %d want %ld", sl, off, want);
            v = x[off];                      // ASan: a real read
          } else {
            (void)x[0];                      // the kernel's clamped load
          }
          lds[buf * kCap + sl] = v;
        }
      }
    };
    stage(chunk_at(g, bx), 0);
    int it = 0;
    for (int ck = bx; ck < g.nchunks; ck += gridx, ++it) {
      const int buf = it & 1;
      const Chunk ch = chunk_at(g, ck);
      const int nlines = std::min(g.R, g.NL - ch.L0);
      const int npos = nlines * g.Wo;
      const long m0 = (long)ch.L0 * g.Wo;
      CHECK(nlines >= 1, "empty chunk %d", ck);
      if (ck + gridx < g.nchunks) stage(chunk_at(g, ck + gridx), buf ^ 1);
      if (range_only && it > 1 && ck + gridx < g.nchunks) continue;
      for (int wave = 0; wave < kWaves; ++wave)
        for (int tq = wave * kTile; tq < npos; tq += kStep)
          for (int lane = 0; lane < 64; ++lane) {
            const int p = lane & 15, gq = lane >> 4;
            const int q = tq + p;
            const bool mv = q < npos;
            if (mv) {
              CHECK(udiv(q, g.Wo, g.mWo) == q / g.Wo, "udiv Wo %d", q);
              CHECK(udiv(ch.ho0 + q / g.Wo, g.Ho, g.mHo) ==
                        (ch.ho0 + q / g.Wo) / g.Ho, "udiv Ho");
            }
            const int ab = mv ? pos_base(g, ch.ho0, q) : 0;
            const long m = m0 + q;
            const int img = (int)(m / ((long)g.Ho * g.Wo));
            const int ho = (int)(m / g.Wo % g.Ho), wo = (int)(m % g.Wo);
            for (int j = 0; j < 8; ++j) {
              const int k = 8 * gq + j;
              const int a = ab + k_off(g, k);
              CHECK(a >= 0 && a < g.nslots, "window read %d outside", a);
              if (a < 0 || a >= kCap) continue;
              const int got = lds[buf * kCap + a];
              CHECK(got != -2, "window read of an unwritten slot");
              if (!mv || k >= K) continue;
              const int tap = k / s.C, c = k % s.C;
              const int hi = s.S * ho + tap / 3 - s.pad;
              const int wi = s.S * wo + tap % 3 - s.pad;
              int ref = 0;
              if (hi >= 0 && hi < s.H && wi >= 0 && wi < s.W)
                ref = xval((((long)img * s.H + hi) * s.W + wi) * s.C + c);
              CHECK(got == ref, "window value m%ld k%d got %d want %d", m, k, got, ref);
            }
            // stores: after the exchange lane (p, gq) holds channels
            // 32*(p>>3) + 8gq .. +7 of positions tq + (p&7) and + 8
            if (range_only) continue;
            for (int q4 = 0; q4 < NG; ++q4) {
              const int cb = 64 * q4 + 32 * (p >> 3) + 8 * gq;
              if (cb >= s.F) continue;
              for (int h = 0; h < 2; ++h) {
                const int qs = tq + (p & 7) + 8 * h;
                if (qs >= npos) continue;
                const long e = (m0 + qs) * s.F + cb;
                CHECK(e % 8 == 0 && e + 8 <= Mtot * s.F, "store outside y");
                for (int i = 0; i < 8 && e + 8 <= Mtot * s.F; ++i) ++stored[e + i];
              }
            }
          }
    }
  }
  if (!range_only) {
    long bad = 0;
    for (long e = 0; e < Mtot * s.F; ++e) bad += stored[e] != 1;
    CHECK(bad == 0, "%ld outputs not stored exactly once", bad);
  }
  std::printf("walk T%d NB%d %dx%d C%d F%d pad%d s%d: R=%d rows=%d chunks=%d grid=%d %s\n",
              s.T, s.NB, s.H, s.W, s.C, s.F, s.pad, s.S, g.R, g.rows, g.nchunks,
              gridx, range_only ? "range" : "full");
}

// the four tiles of a group hold every one of its 64 channels once
static void check_weight_rows() {
  int seen[64] = {0};
  for (int nt = 0; nt < 4; ++nt)
    for (int r = 0; r < 16; ++r) {
      const int c = tile_channel(nt, r);
      CHECK(c >= 0 && c < 64, "tile channel range");
      if (c >= 0 && c < 64) ++seen[c];
    }
  for (int c = 0; c < 64; ++c) CHECK(seen[c] == 1, "channel %d held %d times", c, seen[c]);
}

int main() {
  check_weight_rows();
  const Shape full[] = {
      // tests/test_wdconv_gpu.py
      {2, 3, 7, 7, 3, 72, 1, 1},    {2, 5, 14, 14, 3, 128, 1, 1},
      {1, 2, 9, 8, 1, 96, 0, 1},    {1, 2, 5, 5, 3, 256, 1, 1},
      {2, 3, 3, 3, 3, 80, 0, 1},    {1, 7, 21, 20, 3, 72, 1, 1},
      {2, 3, 7, 7, 3, 72, 1, 2},    {1, 2, 8, 8, 1, 96, 0, 2},
      {1, 5, 28, 28, 1, 128, 1, 2}, {1, 3, 3, 3, 3, 80, 1, 2},
      {2, 2, 8, 8, 3, 136, 1, 1},   {2, 2, 9, 7, 1, 72, 0, 2},
      {2, 12, 14, 15, 1, 96, 1, 1}, {2, 12, 14, 15, 1, 96, 1, 2},
      // edges: one column, one line, a wide line, an image per chunk line
      {1, 1, 1, 1, 3, 72, 1, 1},    {1, 1, 1, 17, 1, 96, 1, 2},
      {1, 200, 3, 3, 3, 72, 1, 1},  {1, 40, 4, 4, 3, 72, 0, 2},
      {1, 3, 30, 200, 3, 72, 1, 1}, {1, 2, 5, 254, 3, 72, 0, 2},
      {1, 2, 9, 400, 3, 72, 1, 1},  {2, 3, 84, 84, 3, 96, 1, 1},
      {1, 1, 3, 453, 3, 72, 1, 1},  // the widest line that fits: 4095 slots
      {2, 3, 84, 84, 3, 96, 1, 2},  {2, 5, 28, 28, 1, 128, 1, 1},
  };
  for (const Shape& s : full) {
    walk(s, 0, false);   // the launcher's grid
    walk(s, 1, false);   // one block walks every chunk
    walk(s, 2, false);
  }
  const Shape range[] = {
      {128, 75, 84, 84, 3, 96, 1, 1}, {128, 5, 84, 84, 3, 128, 1, 2},
      {32, 100, 28, 28, 1, 96, 1, 1}, {128, 75, 84, 84, 3, 256, 1, 2},
  };
  for (const Shape& s : range) walk(s, 0, true);
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
