// The scheduled optimizer step (adam_step_sched): learning-rate schedule, global gradient-norm
// clipping and coupled / decoupled weight decay on the device, next to the Adam of misc.hip.
//   * grad_sqnorm:   per-workgroup fp64 partial sums of g^2 (one extra read of g)
//   * sched_scalars: one workgroup — sums the partials, norm, clip coefficient, t += 1, lr_t
//                    and the bias corrections into the float[8] table `scal` (optim_math.h)
//   * adam_sched:    the Adam update reading that table
// Three launches, no host round trip, nothing step-dependent in a kernel argument: a captured
// step replays correctly.  No atomics and a fixed summation order: the same buffer gives the
// same bits on every call and on every device count.
#include "common.h"
#include "ops.h"
#include "optim_math.h"

namespace ddlpc {

namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_MAX_BLOCKS = 1024;     // one trip of the capped grid = 1024 x 256 float4

// partial[b] = sum over workgroup b's elements of (double)g * (double)g (each product exact).
// Order: a thread adds its float4s x, y, z, w trip by trip, then its tail element; the 256
// thread sums are combined by a halving tree in LDS.
__global__ __launch_bounds__(SQ_THREADS) void grad_sqnorm_kernel(const float* __restrict__ g,
                                                                 long long n,
                                                                 double* __restrict__ partial) {
  __shared__ double red[SQ_THREADS];
  const long long n4 = n / 4;
  double acc = 0.0;
  for (long long i = blockIdx.x * (long long)SQ_THREADS + threadIdx.x; i < n4;
       i += (long long)gridDim.x * SQ_THREADS) {
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    acc += (double)gg.x * (double)gg.x;
    acc += (double)gg.y * (double)gg.y;
    acc += (double)gg.z * (double)gg.z;
    acc += (double)gg.w * (double)gg.w;
  }
  for (long long i = n4 * 4 + blockIdx.x * (long long)SQ_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * SQ_THREADS)
    acc += (double)g[i] * (double)g[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = SQ_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one workgroup of 64: thread k adds partial[k], partial[k + 64], ... in that order, a halving
// tree combines the 64 sums, thread 0 writes the table (nb = 0: clipping off)
__global__ __launch_bounds__(64) void sched_scalars_kernel(float* __restrict__ s,
                                                           const double* __restrict__ partial,
                                                           int nb, SchedArgs a) {
  __shared__ double red[64];
  double acc = 0.0;
  for (int k = threadIdx.x; k < nb; k += 64) acc += partial[k];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) sched_scalars(s, a, red[0]);
}

// The Adam update of misc.hip's adam_kernel with a clipped gradient and either weight decay.
// Per element, with c = scal[5], ss = scal[1], inv = scal[2], dec = scal[6]:
//     gc = g c                                  (one rounding; c = 1 leaves g as it is)
//     coupled:    gr = gc + wd p   (wd != 0)    p0 = p
//     decoupled:  gr = gc                       p0 = p (1 - dec)   (1 - dec formed in fp32)
//     m' = m + (1 - b1) (gr - m)                lerp, as torch.optim.Adam
//     v' = b2 v + (1 - b2) gr gr
//     p' = p0 - ss m' / (sqrtf(v') inv + eps)
// Everything after gc / p0 is adam_kernel's text, so with c = 1 and coupled decay the results
// are adam_step_dev's bit for bit.  gc + wd p is written as the FMA that adam_kernel's g + wd p
// compiles to: left to the compiler, the tail loop pairs g c and wd p into one packed multiply
// and rounds wd p on its own.
template <bool DECOUPLED>
__global__ void adam_sched_kernel(float* __restrict__ p, const float* __restrict__ g,
                                  float* __restrict__ m, float* __restrict__ v, long long n,
                                  float b1, float b2, float eps, float wd,
                                  const float* __restrict__ scal) {
  const float step_size = scal[1], inv_sqrt_bc2 = scal[2], coef = scal[5];
  const float keep = 1.f - scal[6];
  const long long n4 = n / 4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4;
       i += (long long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gc = mul_rn(G[j], coef);
      float gr;
      if (DECOUPLED) { gr = gc; P[j] = mul_rn(P[j], keep); }
      else gr = wd != 0.f ? __builtin_fmaf(wd, P[j], gc) : gc;
      M[j] = M[j] + (1.f - b1) * (gr - M[j]);
      V[j] = b2 * V[j] + (1.f - b2) * gr * gr;
      const float denom = sqrtf(V[j]) * inv_sqrt_bc2 + eps;
      P[j] = P[j] - step_size * M[j] / denom;
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  // tail
  for (long long i = n4 * 4 + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float gc = mul_rn(g[i], coef);
    float gr, p0 = p[i];
    if (DECOUPLED) { gr = gc; p0 = mul_rn(p0, keep); }
    else gr = wd != 0.f ? __builtin_fmaf(wd, p0, gc) : gc;
    m[i] = m[i] + (1.f - b1) * (gr - m[i]);
    v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
    p[i] = p0 - step_size * m[i] / (sqrtf(v[i]) * inv_sqrt_bc2 + eps);
  }
}

}  // namespace

// workgroups (= partial sums) of grad_sqnorm for n elements: a function of n alone — not of
// the CU count, a CU reservation or a knob — so the partials, their order and the norm's bits
// are the same on every machine.  One per 1 024 elements, at most 1 024 (then each walks
// n / 2^20 trips of the grid-stride loop); 0 for an empty buffer.
int grad_sqnorm_blocks(long long n) {
  if (n <= 0) return 0;
  const long long nb = (n / 4 + SQ_THREADS - 1) / SQ_THREADS;     // (the tail rides on block 0)
  return (int)std::min<long long>(std::max<long long>(nb, 1), SQ_MAX_BLOCKS);
}

void grad_sqnorm_launch(const float* g, long long n, double* partial, hipStream_t st) {
  const int nb = grad_sqnorm_blocks(n);
  if (nb == 0) return;
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(nb), dim3(SQ_THREADS), 0, st, g, n, partial);
}

void sched_scalars_launch(float* scal, const double* partial, int nb, const SchedArgs& a,
                          hipStream_t st) {
  hipLaunchKernelGGL(sched_scalars_kernel, dim3(1), dim3(64), 0, st, scal, partial, nb, a);
}

void adam_sched_launch(float* p, const float* g, float* m, float* v, long long n, float b1,
                       float b2, float eps, float wd, bool decoupled, const float* scal,
                       hipStream_t st) {
  const int grid = (int)std::min<long long>((n / 4 + 255) / 256 + 1, 2048);   // as adam_launch
  if (decoupled)
    hipLaunchKernelGGL(adam_sched_kernel<true>, dim3(grid), dim3(256), 0, st, p, g, m, v, n, b1,
                       b2, eps, wd, scal);
  else
    hipLaunchKernelGGL(adam_sched_kernel<false>, dim3(grid), dim3(256), 0, st, p, g, m, v, n, b1,
                       b2, eps, wd, scal);
}

}  // namespace ddlpc
