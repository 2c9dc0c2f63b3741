// Host-side pieces the conv launchers share (tconv.hip, wgrad_nt.hip,
// sconv.hip, dconv.hip), each defined once.
#pragma once

#include <cstdlib>
#include <vector>

#include <hip/hip_bf16.h>
#include <torch/extension.h>

namespace maml355 {

// MAML355_DETERMINISTIC=1: ordered private-slice reductions instead of fp32
// atomics.  Read on every call: tests switch it inside one process.
inline bool deterministic_mode() {
  const char* e = getenv("MAML355_DETERMINISTIC");
  return e && e[0] == '1';
}

// MAML355_WGRAD_NSUB for wgrad_plan.h: 1 or 2, 0 when unset or anything else
inline int wgrad_nsub_override() {
  const char* e = getenv("MAML355_WGRAD_NSUB");
  return e && (e[0] == '1' || e[0] == '2') ? e[0] - '0' : 0;
}

// 16-byte-aligned zeros that tail and border lanes of the async staging read
// instead of predicating: one page of 128 bf16 per device, allocated and
// filled on first use and never written afterwards (a torch::zeros per call
// is a fill-kernel launch per call).  Defined in tconv.hip.
const __hip_bfloat16* conv_zero_page(const torch::Tensor& like);

// The tail of every bf16 wgrad launcher: wgrad_finalize_kernel sums the
// K-chunk slices of acc [T, nslices, 9C, F] in chunk order into
// dw [T, F, C, 3, 3]; db is dbacc [T, nslices, F] summed the same way.
// Returns {dw, db}.  Defined in tconv.hip, next to the kernel.
std::vector<torch::Tensor> finish_wgrad(const torch::Tensor& acc,
                                        const torch::Tensor& dbacc, int T,
                                        int F, int C, int nslices,
                                        hipStream_t stream);

}  // namespace maml355
