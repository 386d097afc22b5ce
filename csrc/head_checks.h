// Argument checks of the evaluation head, called by both registrations (bindings.cpp,
// cpu_ref.cpp), as data_checks.h and tail_checks.h: dtype, shape relations, ranges, same device.
// What depends on the backend stays with it (is_cuda, the CPU twin's .contiguous()).
#pragma once

#include <ATen/ATen.h>

#include <cstdint>

namespace ddlpc {

bool head_supported(int C, int K);      // head_ce.hip: the (C, K) the head kernels are built for

namespace checks {

// head_eval: a bf16 [.., C], Wh fp32 [K][C], bh fp32 [K], int64 labels with one element per pixel,
// the accumulators sums fp64 [3] and cm int64 [K, K], bn4 fp32 [4][C] or None
inline void head_eval(const at::Tensor& a, const at::Tensor& Wh, const at::Tensor& bh,
                      const at::Tensor& labels, const at::Tensor& sums, const at::Tensor& cm,
                      const c10::optional<at::Tensor>& bn4) {
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && a.dim() >= 2 && a.is_contiguous(),
              "head_eval: a must be bf16, contiguous, [.., C]");
  TORCH_CHECK(Wh.scalar_type() == at::kFloat && bh.scalar_type() == at::kFloat && Wh.dim() >= 1,
              "head_eval: Wh and bh must be fp32");
  const int64_t C = a.size(-1), K = Wh.size(0);
  TORCH_CHECK(C >= 1 && K >= 1 && C <= 4096 && K <= 4096 && head_supported((int)C, (int)K),
              "head kernel: unsupported (C, K)");
  TORCH_CHECK(Wh.numel() == K * C && bh.numel() == K && Wh.is_contiguous() && bh.is_contiguous(),
              "head_eval: Wh [K][C] and bh [K], contiguous");
  const int64_t P = a.numel() / C;
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.numel() == P && labels.is_contiguous(),
              "head_eval: labels must be int64, contiguous, one per pixel");
  // (a workgroup's uint32 counter row cannot overflow)
  TORCH_CHECK(P < (1LL << 31), "head_eval: at most 2^31 - 1 pixels per call");
  TORCH_CHECK(sums.scalar_type() == at::kDouble && sums.dim() == 1 && sums.size(0) == 3 && sums.is_contiguous(),
              "head_eval: sums must be float64 [3] (loss sum, hits, counted pixels)");
  TORCH_CHECK(cm.scalar_type() == at::kLong && cm.dim() == 2 && cm.size(0) == K && cm.size(1) == K &&
              cm.is_contiguous(), "head_eval: cm must be int64 [K, K], contiguous");
  TORCH_CHECK(Wh.device() == a.device() && bh.device() == a.device() && labels.device() == a.device() &&
              sums.device() == a.device() && cm.device() == a.device(), "head_eval: tensors on different devices");
  if (bn4.has_value() && bn4->defined())
    TORCH_CHECK(bn4->scalar_type() == at::kFloat && bn4->numel() == 4 * C && bn4->is_contiguous() &&
                bn4->device() == a.device(), "bn4 must be fp32 [4][C] (mean, invstd, scale, shift)");
}

}  // namespace checks
}  // namespace ddlpc
