// Argument checks of lamb_step, called by both registrations (bindings.cpp, cpu_ref.cpp).  The
// kernels walk raw pointers with float4 loads at the addresses the chunk table names, so the
// buffers, the tables' shapes and — lamb_tables — every table entry are refused here before any
// launch.  What depends on the backend stays with it: is_cuda, and how the table's values reach
// the host (the GPU binding copies them once per table).
#pragma once

#include "codec_checks.h"     // T, flat_f32
#include "lamb_math.h"

namespace ddlpc {
namespace checks {

// -> C, the number of chunks (T = tensors.size(0))
inline int64_t lamb_step(T p, T g, T m, T v, T scal, T chunks, T tensors, T partial, T ratio, T norms,
                         int64_t sched_kind, int64_t warmup, int64_t total) {
  const char* names[4] = {"p", "g", "m", "v"};
  const at::Tensor* bufs[4] = {&p, &g, &m, &v};
  for (int i = 0; i < 4; ++i) {
    flat_f32("lamb_step", names[i], *bufs[i]);
    TORCH_CHECK(bufs[i]->numel() == p.numel() && bufs[i]->device() == p.device(), "lamb_step: ", names[i],
                " must have p's size and device");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(bufs[i]->data_ptr()) % 16 == 0, "lamb_step: ", names[i],
                " must be 16-byte aligned");
  }
  TORCH_CHECK(scal.scalar_type() == at::kFloat && scal.numel() == 8 && scal.is_contiguous(),
              "lamb_step: scal must be float[8]");
  TORCH_CHECK(chunks.scalar_type() == at::kLong && chunks.dim() == 2 && chunks.size(1) == 3 &&
              chunks.is_contiguous(), "lamb_step: chunks must be contiguous int64 [C][3]");
  TORCH_CHECK(tensors.scalar_type() == at::kLong && tensors.dim() == 2 && tensors.size(1) == 3 &&
              tensors.is_contiguous(), "lamb_step: tensors must be contiguous int64 [T][3]");
  const int64_t C = chunks.size(0), Tn = tensors.size(0);
  TORCH_CHECK(C < (1LL << 31) && Tn < (1LL << 31), "lamb_step: at most 2^31 - 1 chunks and tensors");
  TORCH_CHECK(partial.scalar_type() == at::kDouble && partial.is_contiguous() && partial.numel() >= 3 * C,
              "lamb_step: partial must be double[>= 3 C]");
  TORCH_CHECK(ratio.scalar_type() == at::kFloat && ratio.is_contiguous() && ratio.numel() >= Tn,
              "lamb_step: ratio must be float[>= T]");
  TORCH_CHECK(norms.scalar_type() == at::kFloat && norms.is_contiguous() && norms.numel() >= 2 * Tn,
              "lamb_step: norms must be float[>= 2 T]");
  for (const at::Tensor* t : {&scal, &chunks, &tensors, &partial, &ratio, &norms})
    TORCH_CHECK(t->device() == p.device(), "lamb_step: every tensor must be on p's device");
  TORCH_CHECK(sched_kind >= 0 && sched_kind <= 2, "sched_kind: 0 constant, 1 poly, 2 cosine");
  TORCH_CHECK(warmup >= 0 && total >= 0, "warmup and total must be >= 0");
  return C;
}

// the table's values (host pointers) against a buffer of n floats: the tensors own consecutive
// chunk ranges that cover [0, C); a tensor's chunks are consecutive pieces of kLambChunk floats,
// the last one shorter; tensors ascend in the buffer without overlap
inline void lamb_tables(const int64_t* ch, int64_t C, const int64_t* tn, int64_t Tn, int64_t n) {
  int64_t next = 0, end = 0;            // the next chunk to be owned, the end of the tensor before
  for (int64_t t = 0; t < Tn; ++t) {
    const int64_t first = tn[3 * t], count = tn[3 * t + 1], adapted = tn[3 * t + 2];
    TORCH_CHECK(first == next && count >= 1 && count <= C - first && (adapted == 0 || adapted == 1),
                "lamb_step: tensor ", t, " must own chunks [", next, ", ...) and carry a 0 / 1 flag");
    for (int64_t j = 0; j < count; ++j) {
      const int64_t* c = ch + 3 * (first + j);
      const bool last = j == count - 1;
      TORCH_CHECK(c[0] == t, "lamb_step: chunk ", first + j, " is not tensor ", t, "'s");
      TORCH_CHECK(c[2] >= 1 && (last ? c[2] <= kLambChunk : c[2] == kLambChunk), "lamb_step: chunk ", first + j,
                  " must hold ", kLambChunk, " floats (a tensor's last: 1 .. ", kLambChunk, ")");
      TORCH_CHECK(c[1] >= end && c[1] % 4 == 0 && c[1] <= n - c[2] &&
                  (j == 0 || c[1] == c[-2] + kLambChunk),
                  "lamb_step: chunk ", first + j, " leaves its tensor's span or the buffer");
    }
    const int64_t* c = ch + 3 * (first + count - 1);
    end = c[1] + c[2];
    next = first + count;
  }
  TORCH_CHECK(next == C, "lamb_step: ", C - next, " chunks belong to no tensor");
}

}  // namespace checks
}  // namespace ddlpc
