// Argument checks of the label operators (label_dist2, label_erode), called by both registrations
// (bindings.cpp, cpu_ref.cpp): dtype, rank, contiguity, ranges.  What depends on the backend stays
// with it: is_cuda, grid limits.
#pragma once

#include <ATen/ATen.h>

#include <cstdint>

namespace ddlpc {
namespace checks {

// labels: int64 [B, H, W] (a batch) or uint8 [H, W] / [B, H, W] (scene labels), contiguous
inline void label_dist2(const at::Tensor& labels, int64_t K, int64_t ignore_index) {
  const bool i64 = labels.scalar_type() == at::kLong, u8 = labels.scalar_type() == at::kByte;
  TORCH_CHECK((i64 && labels.dim() == 3) || (u8 && (labels.dim() == 2 || labels.dim() == 3)),
              "labels must be int64 [B, H, W] or uint8 [H, W] / [B, H, W]");
  TORCH_CHECK(labels.is_contiguous(), "labels must be contiguous");
  TORCH_CHECK(K >= 1 && K <= 16, "1 <= K <= 16");
  TORCH_CHECK(ignore_index >= INT32_MIN && ignore_index <= INT32_MAX, "ignore_index out of range");
  TORCH_CHECK(labels.size(-1) * labels.size(-2) < (1LL << 31), "H * W must be below 2^31");
}

inline void label_erode(const at::Tensor& labels, int64_t K, int64_t ignore_index, int64_t radius,
                        int64_t fill) {
  label_dist2(labels, K, ignore_index);
  TORCH_CHECK(radius >= 0 && radius <= 16, "0 <= radius <= 16");
  if (labels.scalar_type() == at::kByte) {
    TORCH_CHECK(fill >= K && fill <= 255, "uint8 labels: fill must lie in K..255");
  } else {
    TORCH_CHECK(fill < 0 || fill >= K || fill == ignore_index,
                "fill must not be a counted label (a class other than ignore_index)");
  }
}

}  // namespace checks
}  // namespace ddlpc
