// Argument checks of the top-k gradient codec operators, one function per operator, called by both
// registrations (bindings.cpp, cpu_ref.cpp).  The kernels index with 32-bit integers and write
// through raw pointers, so sizes, dtypes and k are refused here before any launch.  What depends
// on the backend stays with it: is_cuda.
#pragma once

#include "data_checks.h"      // T

namespace ddlpc {
namespace checks {

inline void flat_f32(const char* op, const char* name, T t) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 1 && t.is_contiguous(), op, ": ", name,
              " must be a contiguous 1-D fp32 tensor");
}

// g, residual: n fp32 elements each; 1 <= k <= n < 2^31
inline void topk_encode(T g, T residual, int64_t k) {
  flat_f32("topk_encode", "g", g);
  flat_f32("topk_encode", "residual", residual);
  TORCH_CHECK(residual.numel() == g.numel() && residual.device() == g.device(),
              "topk_encode: residual must have g's size and device");
  TORCH_CHECK(g.numel() < (1LL << 31), "topk_encode: n must be below 2^31");
  TORCH_CHECK(k >= 1 && k <= g.numel(), "topk_encode: 1 <= k <= n, got k = ", k, ", n = ", g.numel());
}

// out fp32 [n]; idx int32 [W][k] (each row ascending, values in [0, n)); val fp32 [W][k]; w fp32 [W]
inline void topk_decode_sum(T out, T idx, T val, T w) {
  flat_f32("topk_decode_sum", "out", out);
  TORCH_CHECK(out.numel() >= 1 && out.numel() < (1LL << 31), "topk_decode_sum: 1 <= n < 2^31");
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 2 && idx.is_contiguous() && idx.size(0) >= 1 &&
              idx.size(1) >= 1 && idx.size(1) <= out.numel(),
              "topk_decode_sum: idx must be contiguous int32 [W][k] with 1 <= k <= n");
  TORCH_CHECK(val.scalar_type() == at::kFloat && val.is_contiguous() && val.sizes() == idx.sizes(),
              "topk_decode_sum: val must be contiguous fp32 of idx's shape");
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.is_contiguous() && w.numel() == idx.size(0),
              "topk_decode_sum: w must hold W fp32 weights");
  TORCH_CHECK(idx.device() == out.device() && val.device() == out.device() && w.device() == out.device(),
              "topk_decode_sum: tensors on different devices");
}

}  // namespace checks
}  // namespace ddlpc
