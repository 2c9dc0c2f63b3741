// CPU check of the wgrad launchers' split-K plan
// (howtotrainyourmamlpytorch_amd/ops/hip/wgrad_plan.h).  No GPU: built with
// -fsanitize=address,undefined and run by tests/test_wgrad_plan.py.
//
//  (a) pinned plans: what the launchers computed at the commit before the
//      plan moved into the header (each had its own copy of the arithmetic
//      then), at test shapes and at the workloads' layer shapes;
//  (b) invariants over a sweep of shapes, both modes and the
//      MAML355_WGRAD_NSUB override: the deterministic v3 plan cuts the
//      K-chunks of the v2 plan from 30 000 positions up and of the v1 plan
//      below, chunks are whole K-steps, cover the reduction and leave no
//      empty trailing slice, private slices exist exactly off the atomic
//      path, and the grid fits.

#include <cstdio>

#include "wgrad_plan.h"

using namespace maml355::wgplan;

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

static int out1(int h, int pad) { return h + 2 * pad - 2; }            // stride 1
static int out2(int h, int pad) { return (h + 2 * pad - 3) / 2 + 1; }  // stride 2

// ---- (a) pinned plans -----------------------------------------------------
struct Pinned {
  Shape s;
  bool det;
  int v1_gridx, v1_kchunk, v1_gridy;
  int v2_nsub; long v2_Kr; int v2_gridx, v2_kchunk, v2_gridy;
  int v3_Wk; long v3_Kr; int v3_nsub, v3_gridx, v3_bias, v3_kchunk, v3_gridy;
};

static const Pinned kPinned[] = {
  {{2, 3, 11, 9, 48, 48, 1}, false, 7, 64, 5, 1, 576, 7, 64, 9,
   9, 320, 1, 7, kBiasOnes, 64, 5},
  {{2, 3, 11, 9, 48, 48, 1}, true, 7, 64, 5, 1, 576, 7, 64, 9,
   9, 320, 1, 7, kBiasColsum, 64, 5},
  {{1, 1, 3, 3, 8, 8, 0}, true, 2, 64, 1, 1, 64, 2, 64, 1,
   1, 64, 1, 2, kBiasColsum, 64, 1},
  // mini-imagenet first layer, 128 tasks
  {{128, 75, 84, 84, 3, 48, 1}, false, 1, 4096, 130, 1, 554432, 1, 4096, 136,
   84, 529216, 2, 1, kBiasOnes, 4096, 130},
  {{128, 75, 84, 84, 3, 48, 1}, true, 1, 66176, 8, 1, 554432, 1, 69312, 8,
   88, 554432, 2, 1, kBiasColsum, 69312, 8},
  // ... second layer
  {{128, 75, 42, 42, 48, 48, 1}, false, 7, 4096, 33, 2, 151232, 4, 4096, 37,
   42, 132352, 2, 4, kBiasOnes, 4096, 33},
  {{128, 75, 42, 42, 48, 48, 1}, true, 7, 132352, 1, 2, 151232, 4, 75648, 2,
   48, 151232, 2, 4, kBiasColsum, 75648, 2},
  // omniglot first layer
  {{32, 20, 28, 28, 1, 64, 1}, false, 1, 512, 31, 1, 17920, 1, 576, 32,
   28, 15680, 1, 2, kBiasOnes, 1024, 16},
  {{32, 20, 28, 28, 1, 64, 1}, true, 1, 512, 31, 1, 17920, 1, 576, 32,
   28, 15680, 1, 2, kBiasColsum, 512, 31},
  // 33 075 positions: deterministic v3 takes v2's chunks
  {{4, 75, 21, 21, 48, 48, 1}, true, 7, 960, 35, 1, 37824, 7, 1088, 35,
   24, 37824, 1, 7, kBiasColsum, 1088, 35},
  {{2, 8, 64, 64, 16, 24, 1}, false, 3, 256, 128, 1, 32768, 3, 256, 128,
   64, 32768, 1, 3, kBiasOnes, 256, 128},
};

struct PinnedSmall { Shape s; bool det; int gridx, kchunk, gridy_or_nslices; };

static const PinnedSmall kPinnedStride2[] = {
  {{128, 75, 84, 84, 3, 48, 1}, false, 1, 4096, 33},
  {{128, 75, 84, 84, 3, 48, 1}, true, 1, 16576, 8},
  {{4, 75, 21, 21, 48, 48, 1}, false, 7, 256, 36},
  {{4, 75, 21, 21, 48, 48, 1}, true, 7, 256, 36},
};

static const PinnedSmall kPinnedF32[] = {
  {{2, 3, 11, 9, 48, 48, 1}, true, 7, 32, 10},
  {{128, 75, 84, 84, 3, 48, 1}, true, 1, 22080, 24},
  {{32, 20, 28, 28, 1, 64, 1}, true, 1, 192, 82},
};

static void check_pinned() {
  for (const Pinned& r : kPinned) {
    const Shape& s = r.s;
    const int Ho = out1(s.H, s.pad), Wo = out1(s.W, s.pad);
    const Plan a = v1(s.T, s.NB, Ho, Wo, s.C, r.det);
    const Plan b = v2(s.T, s.NB, Ho, Wo, s.C, r.det, 0);
    const Plan c = v3(s.T, s.NB, Ho, Wo, s.C, true, r.det, true, 0);
#define SAME(got, want)                                                        \
  CHECK((long)(got) == (long)(want), "%d,%d,%d,%d,%d,%d,%d det=%d: %s = %ld, "  \
        "pinned %ld", s.T, s.NB, s.H, s.W, s.C, s.F, s.pad, (int)r.det, #got,  \
        (long)(got), (long)(want))
    SAME(a.gridx, r.v1_gridx); SAME(a.kchunk, r.v1_kchunk);
    SAME(a.gridy, r.v1_gridy); SAME(a.nslices, r.det ? r.v1_gridy : 1);
    SAME(b.nsub, r.v2_nsub); SAME(b.Kr, r.v2_Kr); SAME(b.gridx, r.v2_gridx);
    SAME(b.kchunk, r.v2_kchunk); SAME(b.gridy, r.v2_gridy);
    SAME(b.nslices, r.det ? r.v2_gridy : 1);
    SAME(c.Wk, r.v3_Wk); SAME(c.Kr, r.v3_Kr); SAME(c.nsub, r.v3_nsub);
    SAME(c.gridx, r.v3_gridx); SAME(c.bias, r.v3_bias);
    SAME(c.kchunk, r.v3_kchunk); SAME(c.gridy, r.v3_gridy);
    SAME(c.nslices, r.det ? r.v3_gridy : 1);
  }
  for (const PinnedSmall& r : kPinnedStride2) {
    const Shape& s = r.s;
    const Plan a = sconv(s.T, s.NB, out2(s.H, s.pad), out2(s.W, s.pad), s.C,
                         r.det);
    SAME(a.gridx, r.gridx); SAME(a.kchunk, r.kchunk);
    SAME(a.gridy, r.gridy_or_nslices);
    SAME(a.nslices, r.det ? r.gridy_or_nslices : 1);
  }
  for (const PinnedSmall& r : kPinnedF32) {
    const Shape& s = r.s;
    const Plan a = fconv(s.T, s.NB, out1(s.H, s.pad), out1(s.W, s.pad), s.C);
    SAME(a.gridx, r.gridx); SAME(a.kchunk, r.kchunk);
    SAME(a.nslices, r.gridy_or_nslices); SAME(a.gridy, a.nslices);
  }
#undef SAME
  // without bias v3 carries no bias column in either mode
  CHECK(v3(2, 3, 11, 9, 48, false, false, true, 0).bias == kBiasNone, "bias");
  CHECK(v3(2, 3, 11, 9, 48, false, true, true, 0).bias == kBiasNone, "bias");
}

// ---- (b) invariants -------------------------------------------------------
// `atomic`: the plan shares one accumulator between its K-chunks
static void check_chunks(const char* what, const Plan& p, int kstep,
                         bool atomic, const Shape& s, int ovr) {
#define INV(cond)                                                              \
  CHECK(cond, "%s %d,%d,%d,%d,%d,%d,%d atomic=%d nsub=%d: %s (kchunk %d "      \
        "gridy %d nslices %d Kr %ld)", what, s.T, s.NB, s.H, s.W, s.C, s.F,    \
        s.pad, (int)atomic, ovr, #cond, p.kchunk, p.gridy, p.nslices, p.Kr)
  INV(p.kchunk > 0 && p.kchunk % kstep == 0);
  INV((long)p.gridy * p.kchunk >= p.Kr);
  INV((long)(p.gridy - 1) * p.kchunk < p.Kr);
  INV(p.nslices == (atomic ? 1 : p.gridy));
  INV(p.gridy >= 1 && p.gridy <= 65535);
  INV(p.gridx >= 1 && (p.nsub == 1 || p.nsub == 2));
  INV(p.gridx * kCols * p.nsub >= 9 * s.C);
#undef INV
}

static long check_sweep() {
  const int Ts[] = {1, 2, 32, 128}, NBs[] = {1, 5, 75};
  const int HWs[] = {3, 5, 10, 21, 28, 42, 84}, Cs[] = {1, 3, 8, 48, 64};
  const int Fs[] = {8, 48, 64};
  long cases = 0;
  for (int T : Ts) for (int NB : NBs) for (int HW : HWs) for (int C : Cs)
  for (int F : Fs) for (int pad = 0; pad <= 1; ++pad)
  for (int ovr = 0; ovr <= 2; ++ovr) for (int det = 0; det <= 1; ++det) {
    const Shape s = {T, NB, HW, HW, C, F, pad};
    const int Ho = out1(HW, pad), Wo = out1(HW, pad);
    const Plan a = v1(T, NB, Ho, Wo, C, det);
    const Plan b = v2(T, NB, Ho, Wo, C, det, ovr);
    check_chunks("v1", a, kStep, !det, s, ovr);
    check_chunks("v2", b, kStep, !det, s, ovr);
    CHECK(b.Wk % 8 == 0 && b.Wk >= Wo && b.Wk < Wo + 8, "v2 Wk %d", b.Wk);
    CHECK(b.Kr % kStep == 0 && b.Kr >= (long)NB * Ho * b.Wk, "v2 Kr");
    for (int v2_on = 0; v2_on <= 1; ++v2_on) {
      const Plan c = v3(T, NB, Ho, Wo, C, true, det, v2_on, ovr);
      check_chunks("v3", c, kStep, !det, s, ovr);
      CHECK(c.Kr % kStep == 0 && c.Kr >= (long)NB * Ho * c.Wk &&
            c.Kr < (long)NB * Ho * c.Wk + kStep, "v3 Kr");
      CHECK(det ? c.bias == kBiasColsum : c.bias != kBiasNone, "v3 bias %d",
            c.bias);
      if (!det) {
        CHECK(c.Wk == Wo, "atomic v3 pads no line");
        continue;
      }
      const bool as_v2 = (long)NB * Ho * Wo >= 30000 && v2_on;
      const Plan& old = as_v2 ? b : a;
      CHECK(c.kchunk == old.kchunk && c.gridy == old.gridy &&
            c.nslices == old.nslices && c.Wk == old.Wk,
            "det v3 %d,%d,%d,%d,%d pad %d nsub %d v2_on %d: kchunk %d gridy "
            "%d Wk %d, %s has %d %d %d", T, NB, HW, HW, C, pad, ovr, v2_on,
            c.kchunk, c.gridy, c.Wk, as_v2 ? "v2" : "v1", old.kchunk,
            old.gridy, old.Wk);
    }
    check_chunks("sconv", sconv(T, NB, out2(HW, pad), out2(HW, pad), C, det),
                 kStep, !det, s, ovr);
    check_chunks("fconv", fconv(T, NB, Ho, Wo, C), kStepF32, false, s, ovr);
    ++cases;
  }
  return cases;
}

int main() {
  check_pinned();
  const long cases = check_sweep();
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("%ld sweep cases; all checks passed\n", cases);
  return 0;
}
