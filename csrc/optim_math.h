// Scalar arithmetic of the scheduled optimizer step, shared by the gfx950 scalars kernel
// (optim.hip) and its CPU twin (cpu_ref.cpp): one text, all in double, no contraction (the
// Python twin FlatAdam.lr_at evaluates the same operations one rounding each).
#pragma once

#include <cmath>

#include "hd.h"

namespace ddlpc {

enum SchedKind { SCHED_CONSTANT = 0, SCHED_POLY = 1, SCHED_COSINE = 2 };

struct SchedArgs {
  double lr, b1, b2, wd, max_norm, lr_min, power;
  long long warmup, total;
  int kind;          // SchedKind
  int decoupled;     // 1: scal[6] = lr_t * wd (AdamW), 0: scal[6] = 0 (wd goes into the gradient)
};

// lr at optimizer step t (1-based); s = t - 1 steps already taken, W = warmup, T = total:
//   s < W:  lr (s + 1) / W
//   else    u = clamp((s - W) / max(1, T - W), 0, 1),  lr_min + (lr - lr_min) f(u)
//           constant f = 1 | poly f = (1 - u)^power (power 1: 1 - u, no pow) | cosine
//           f = 0.5 (1 + cos(pi u));  poly and cosine: u = 1 (every step after T) is lr_min exactly
DDLPC_HD inline double sched_lr(const SchedArgs& a, double t) {
#pragma clang fp contract(off)
  const double s = t - 1.0, W = (double)a.warmup, T = (double)a.total;
  if (s < W) return a.lr * (s + 1.0) / W;
  const double span = T - W > 1.0 ? T - W : 1.0;
  double u = (s - W) / span;
  u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
  double f = 1.0;
  if (a.kind == SCHED_POLY) f = a.power == 1.0 ? 1.0 - u : pow(1.0 - u, a.power);
  else if (a.kind == SCHED_COSINE) f = 0.5 * (1.0 + cos(3.141592653589793 * u));
  if (a.kind != SCHED_CONSTANT && u >= 1.0) f = 0.0;     // (whatever cos(pi) rounds to)
  const double d = (a.lr - a.lr_min) * f;
  return a.lr_min + d;
}

// the float[8] table of one step from s[0] (the steps taken) and the gradient's squared norm
// (sq < 0: clipping off):  t, lr_t / (1 - b1^t), 1 / sqrt(1 - b2^t), lr_t, norm, coef,
// lr_t wd | 0, 0.  coef = min(max_norm / (norm + 1e-6), 1) as torch.nn.utils.clip_grad_norm_; a
// NaN / Inf norm propagates into coef (and so into every parameter), as there
DDLPC_HD inline void sched_scalars(float* s, const SchedArgs& a, double sq) {
#pragma clang fp contract(off)
  const double t = (double)s[0] + 1.0;
  const double lr_t = sched_lr(a, t);
  double norm = 0.0, coef = 1.0;
  if (a.max_norm > 0.0) {
    norm = sqrt(sq);
    coef = a.max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  s[0] = (float)t;
  s[1] = (float)(lr_t / (1.0 - pow(a.b1, t)));
  s[2] = (float)(1.0 / sqrt(1.0 - pow(a.b2, t)));
  s[3] = (float)lr_t;
  s[4] = (float)norm;
  s[5] = (float)coef;
  s[6] = a.decoupled ? (float)(lr_t * a.wd) : 0.f;
  s[7] = 0.f;
}

}  // namespace ddlpc
