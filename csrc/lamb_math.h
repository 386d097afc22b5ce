// Arithmetic of the LAMB step (You et al. 2020), shared by the gfx950 kernels (lamb.hip) and their
// CPU twin (cpu_ref.cpp): one text.  The fp32 element functions round every operation on its own
// (no contraction), so the moments kernel and the apply kernel form the same u bit for bit, and so
// do the two kernel sets; the scalars and the trust ratio are formed in double.
//
// Per element i of tensor t, with c = scal[5], ibc1 = scal[1], isb2 = scal[2], lr_t = scal[3]:
//     gc = g c
//     m' = m + (1 - b1) (gc - m)            v' = b2 v + ((1 - b2) gc) gc
//     r  = (m' ibc1) / (sqrtf(v') isb2 + eps)
//     u  = r + wd p   (an adapted tensor with wd != 0),   u = r   (otherwise)
//     ratio_t = ||p_t|| / ||u_t||  if both norms are positive and finite, else 1 (excluded: 1)
//     p' = p - (lr_t ratio_t) u
//
// Tables (int64, built once from the flat layout; lamb_checks.h refuses any other form):
//     chunks  [C][3] = (tensor, begin, length): consecutive pieces of 1 024 floats of one tensor,
//                      the tensor's last piece shorter; begin is a multiple of 4; no chunk
//                      straddles two tensors, and the alignment gaps between tensors belong to none
//     tensors [T][3] = (first chunk, chunk count, adapted flag)
// Scalar table `scal`, float[8], written by lamb_scalars from scal[0] (the steps taken):
//     [0] t   [1] 1 / (1 - b1^t)   [2] 1 / sqrt(1 - b2^t)   [3] lr_t (sched_lr of optim_math.h)
//     [4] gradient norm over the chunks (0: clipping off)   [5] clip coefficient (1: off)
//     [6] 0   [7] 0
// Sums: thread k of the 256 of a chunk adds its elements 4k .. 4k + 3 and then, for the short last
// piece, element 4 (len / 4) + k (k < len % 4); a halving tree combines the 256 sums.  A tensor's
// chunk sums: thread k adds those of chunks k, k + 256, ... and the same tree combines them.
#pragma once

#include <cmath>

#include "hd.h"
#include "optim_math.h"

namespace ddlpc {

constexpr int kLambChunk = 1024;       // floats per chunk: one float4 per thread of a workgroup
constexpr int kLambThreads = 256;

struct LambHyper { float b1, b2, eps, wd; };

DDLPC_HD inline void lamb_scalars(float* s, const SchedArgs& a, double sq) {
#pragma clang fp contract(off)
  const double t = (double)s[0] + 1.0;
  double norm = 0.0, coef = 1.0;
  if (a.max_norm > 0.0) {                 // as sched_scalars: torch.nn.utils.clip_grad_norm_
    norm = sqrt(sq);
    coef = a.max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  s[0] = (float)t;
  s[1] = (float)(1.0 / (1.0 - pow(a.b1, t)));
  s[2] = (float)(1.0 / sqrt(1.0 - pow(a.b2, t)));
  s[3] = (float)sched_lr(a, t);
  s[4] = (float)norm;
  s[5] = (float)coef;
  s[6] = 0.f;
  s[7] = 0.f;
}

// m, v <- m', v' from the clipped gradient
DDLPC_HDI void lamb_moments(float g, float coef, const LambHyper& h, float& m, float& v) {
#pragma clang fp contract(off)
  const float gc = g * coef;
  m = m + (1.f - h.b1) * (gc - m);
  v = h.b2 * v + ((1.f - h.b2) * gc) * gc;
}

// u from p and the new moments; wdt = wd for an adapted tensor, 0 for an excluded one
DDLPC_HDI float lamb_u(float p, float m, float v, float ibc1, float isb2, float eps, float wdt) {
#pragma clang fp contract(off)
  const float r = div_rn(m * ibc1, sqrtf(v) * isb2 + eps);
  return wdt != 0.f ? r + wdt * p : r;
}

// p' with step = lr_t ratio_t (formed once per chunk by mul_rn)
DDLPC_HDI float lamb_apply(float p, float u, float step) {
#pragma clang fp contract(off)
  return p - step * u;
}

// the trust ratio and the two norms of a tensor from its sums of p^2 and u^2
DDLPC_HD inline void lamb_ratio(double sp, double su, bool adapted, float* ratio, float* norms) {
  const double np = sqrt(sp), nu = sqrt(su);
  const bool ok = adapted && np > 0.0 && nu > 0.0 && np < HUGE_VAL && nu < HUGE_VAL;   // (NaN: no)
  *ratio = ok ? (float)(np / nu) : 1.f;
  norms[0] = (float)np;
  norms[1] = (float)nu;
}

}  // namespace ddlpc
