// CPU check of the LDS-staged first-layer forward's address logic
// (howtotrainyourmamlpytorch_amd/ops/hip/dconv_fwd_v3_addr.h).  No GPU:
// built with -fsanitize=address,undefined and run by
// tests/test_dconv_fwd_v3_addr.py.
//
// Per shape and grid width it replays the kernel's walk: every block's chunks
// with the incremental (img0, ho0) carry, every staging slot of every chunk,
// every wave's tiles with the incremental lane position, every window read.
// It checks that
//  * the multiply-high divisions and the incremental states agree with the
//    closed forms;
//  * every staged slot reads inside the task's x (the element is really read
//    from an array of exactly that size, so ASan sees an overrun) or is a
//    zero, and agrees with the definition of the zero-padded image;
//  * every window read of a stored position hits a slot that this chunk
//    wrote and finds there the value of the zero-padded 3x3 window; reads of
//    lanes past the chunk's end stay inside the written slots too;
//  * every output position is produced exactly once.
// `range` shapes (workload size) walk the first and the last task's first
// and last blocks only, and add the task base to every offset in 64 bits.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dconv_fwd_v3_addr.h"

using namespace maml355::dfv3;

static int g_fail = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__);      \
                         std::printf(__VA_ARGS__); std::printf("\n"); }        \
      ++g_fail;                                                                \
    }                                                                          \
  } while (0)

struct Shape { int T, NB, H, W, C, F, pad; };

// value of element e of the task's x: never 0, so a zero slot is told apart
static uint16_t xval(long e) { return (uint16_t)(1 + e % 65521); }

// the launcher's grid width (dconv.hip)
static int grid_for(const Geom& g, int T) {
  const long fill = (2048 + T - 1) / T;
  const long per_task = std::max<long>((g.nchunks + 11) / 12, fill);
  return (int)std::min<long>(g.nchunks, per_task);
}

static void walk(const Shape& s, int gridx, bool range_only) {
  const int fill = (2048 + s.T - 1) / s.T;
  const Geom g = make_geom(s.NB, s.H, s.W, s.C, s.pad, fill);
  CHECK(g.R >= 1, "shape does not fit");
  if (g.R < 1) return;
  if (gridx <= 0) gridx = grid_for(g, s.T);
  gridx = std::min(gridx, g.nchunks);
  CHECK(gridx >= 1 && gridx <= g.nchunks, "grid %d of %d chunks", gridx, g.nchunks);
  CHECK((long)g.rows * g.RS <= kCap, "staged rows exceed the LDS buffer");
  CHECK((long)(g.Ho + kCap) * std::max(g.Hp, g.RS) < (1L << 32), "magic range");
  const long x_task = (long)s.NB * s.H * s.W * s.C;
  const long x_total = x_task * s.T;
  const long Mtot = (long)g.NL * g.Wo;
  const int K = 9 * s.C, KS = (K + 3) / 4;
  std::vector<uint16_t> x(x_task);
  for (long e = 0; e < x_task; ++e) x[e] = xval(e);
  std::vector<uint8_t> produced(Mtot, 0);
  std::vector<int> koff(4 * KS);
  for (int k = 0; k < 4 * KS; ++k) koff[k] = k < K ? k_off(g, k) : 0;

  const int dL = gridx * g.R;
  const int sdimg = dL / g.Ho, sdho = dL - sdimg * g.Ho;
  std::vector<int> lds(2 * kCap);            // -2: never written; else value
  for (int bx = 0; bx < gridx; ++bx) {
    if (range_only && bx != 0 && bx != gridx - 1) continue;
    std::fill(lds.begin(), lds.end(), -2);
    Chunk ch = chunk_at(g, bx);
    auto stage = [&](int img0, int ho0, int buf) {
      for (int sl = 0; sl < kCap; ++sl) {
        // closed forms of the two multiply-high divisions
        CHECK(udiv(sl, g.mRS) == sl / g.RS, "udiv RS %d", sl);
        const int row = sl / g.RS, col = sl % g.RS;
        CHECK(udiv(ho0 + row, g.mHp) == (ho0 + row) / g.Hp, "udiv Hp");
        const int off = slot_src(g, img0, ho0, sl);
        // definition: padded row hp of image img, padded column wp, channel
        const int img = img0 + (ho0 + row) / g.Hp, hp = (ho0 + row) % g.Hp;
        const int wp = col / s.C, c = col % s.C;
        const bool inside = row < g.rows && img < s.NB && hp >= s.pad &&
                            hp < s.H + s.pad && wp >= s.pad && wp < s.W + s.pad;
        CHECK((off >= 0) == inside, "slot %d zero decision", sl);
        int v = 0;
        if (off >= 0) {
          const long want =
              (((long)img * s.H + (hp - s.pad)) * s.W + (wp - s.pad)) * s.C + c;
          CHECK(off == want, "slot %d off %d want %ld", sl, off, want);
          CHECK(off < x_task, "slot %d reads past the task's x", sl);
          const long full = (long)(s.T - 1) * x_task + off;
          CHECK(full < x_total && full >= off, "full range");
          v = x[off];                        // ASan: a real read
        } else {
          (void)x[0];                        // the kernel's clamped load
        }
        lds[buf * kCap + sl] = v;
      }
    };
    stage(ch.img0, ch.ho0, 0);
    int it = 0;
    for (int ck = bx; ck < g.nchunks; ck += gridx, ++it) {
      const int buf = it & 1;
      // incremental chunk origin against the closed form
      const Chunk want = chunk_at(g, ck);
      CHECK(ch.L0 == want.L0 && ch.img0 == want.img0 && ch.ho0 == want.ho0,
            "chunk %d origin", ck);
      const int nlines = std::min(g.R, g.NL - ch.L0);
      const int npos = nlines * g.Wo;
      const int m0 = ch.L0 * g.Wo;
      CHECK(nlines >= 1, "empty chunk %d", ck);
      const int nck = ck + gridx;
      int nho0 = ch.ho0 + sdho, nimg0 = ch.img0 + sdimg;
      if (nho0 >= g.Ho) { nho0 -= g.Ho; nimg0 += 1; }
      stage(nck < g.nchunks ? nimg0 : s.NB, nho0, buf ^ 1);
      const bool sample = range_only && it > 1 && nck < g.nchunks;
      for (int wave = 0; wave < 4 && !sample; ++wave)
        for (int li = 0; li < 16; ++li) {
          const int q0 = wave * kTile + li;
          LanePos p = lane_init(g, ch.ho0, q0 / g.Wo, q0 % g.Wo);
          int q = q0;
          for (int tq = wave * kTile; tq < npos; tq += kStep) {
            if (tq != wave * kTile) { q += kStep; lane_advance(g, p); }
            const bool mv = q < npos;
            // closed form of the lane position
            if (mv) {
              const int l = q / g.Wo, wo = q % g.Wo;
              const int cross = (ch.ho0 + l) / g.Ho;
              CHECK(p.wo == wo && p.ho == (ch.ho0 + l) % g.Ho &&
                        p.ab == (l + 2 * cross) * g.RS + wo * s.C,
                    "lane pos ck%d q%d", ck, q);
            }
            const int ab = mv ? p.ab : 0;
            const long m = (long)m0 + q;
            const int img = (int)(m / ((long)g.Ho * g.Wo));
            const int ho = (int)(m / g.Wo % g.Ho), wo = (int)(m % g.Wo);
            for (int k = 0; k < 4 * KS; ++k) {
              const int a = ab + koff[k];
              CHECK(a >= 0 && a < g.rows * g.RS, "window read %d outside", a);
              if (a < 0 || a >= kCap) continue;
              const int got = lds[buf * kCap + a];
              CHECK(got != -2, "window read of an unwritten slot");
              if (!mv || k >= K) continue;
              const int tap = k / s.C, c = k % s.C;
              const int hi = ho + tap / 3 - s.pad, wi = wo + tap % 3 - s.pad;
              int ref = 0;
              if (hi >= 0 && hi < s.H && wi >= 0 && wi < s.W)
                ref = xval((((long)img * s.H + hi) * s.W + wi) * s.C + c);
              CHECK(got == ref, "window value m%ld k%d got %d want %d", m, k,
                    got, ref);
            }
            if (mv && li == 0)
              for (int i = 0; i < kTile && q + i < npos; ++i) {
                CHECK(m + i < Mtot, "position past the task");
                if (m + i < Mtot) ++produced[m + i];
              }
          }
        }
      if (sample)
        for (int q = 0; q < npos; ++q) ++produced[m0 + q];
      ch.L0 += dL; ch.img0 = nimg0; ch.ho0 = nho0;
    }
  }
  if (!range_only) {
    long bad = 0;
    for (long m = 0; m < Mtot; ++m) bad += produced[m] != 1;
    CHECK(bad == 0, "%ld positions not produced exactly once", bad);
  }
  std::printf("walk T%d NB%d %dx%d C%d pad%d: R=%d rows=%d chunks=%d grid=%d %s\n",
              s.T, s.NB, s.H, s.W, s.C, s.pad, g.R, g.rows, g.nchunks, gridx,
              range_only ? "range" : "full");
}

int main() {
  const Shape full[] = {
      {1, 1, 1, 1, 3, 48, 1},    {1, 1, 3, 5, 3, 48, 1},
      {1, 1, 1, 17, 1, 64, 1},   {2, 3, 7, 5, 3, 16, 1},
      {2, 3, 9, 11, 1, 32, 0},   {2, 2, 3, 3, 3, 48, 0},
      {1, 200, 3, 3, 3, 16, 1},  {2, 5, 14, 14, 1, 64, 1},
      {2, 5, 14, 14, 3, 48, 1},  {3, 2, 20, 84, 3, 48, 1},
      {2, 2, 28, 28, 1, 64, 1},  {2, 3, 7, 7, 1, 16, 1},
      {2, 3, 7, 7, 3, 64, 1},    {1, 1, 14, 84, 3, 48, 1},
      {1, 5, 28, 28, 1, 64, 1},  {1, 3, 30, 200, 3, 48, 1},
      {1, 2, 5, 254, 3, 16, 0},  {1, 1, 1, 254, 3, 16, 1},
      // several chunks per block, ragged last chunk (tests/test_dconv_fwd_v3_gpu.py)
      {1, 2, 7, 84, 3, 48, 1},   {2, 2, 7, 84, 3, 16, 0},
      {1, 2, 20, 28, 1, 64, 1},  {2, 7, 9, 9, 1, 32, 1},
      {1, 40, 5, 5, 3, 64, 1},   {2, 3, 7, 84, 3, 48, 0},
      {2, 3, 9, 11, 1, 64, 1},   {2, 4, 3, 3, 3, 16, 0},
      {2, 4, 3, 3, 3, 16, 1},
  };
  for (const Shape& s : full) {
    walk(s, 0, false);   // the launcher's grid
    walk(s, 1, false);   // one block walks every chunk
    walk(s, 2, false);
  }
  const Shape range[] = {
      {128, 75, 84, 84, 3, 48, 1}, {128, 5, 84, 84, 3, 48, 1},
      {32, 100, 28, 28, 1, 64, 1},
  };
  for (const Shape& s : range) walk(s, 0, true);
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
