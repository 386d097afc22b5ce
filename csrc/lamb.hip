// The LAMB step (lamb_step): Adam moments with a per-tensor trust ratio ||p_t|| / ||u_t|| on the
// device, next to the scheduled Adam of optim.hip and with the same per-step scalars (schedule,
// gradient-norm clipping).  The work is cut by a chunk table built once from the flat layout
// (lamb_math.h): pieces of 1 024 floats of one tensor, one 256-thread workgroup and one float4
// per thread each; a tensor's last piece is short and ends with scalar loads.
//   * lamb_gradnorm: per-chunk fp64 sums of g^2 (clipping on only; one extra read of g)
//   * lamb_scalars:  one workgroup — the gradient norm, clip coefficient, t += 1, lr_t and the
//                    bias corrections into the float[8] table `scal`
//   * lamb_moments:  per chunk: m', v' written, u formed in registers, {sum p^2, sum u^2} in fp64
//   * lamb_ratios:   per tensor: its chunks' sums -> ratio_t and the two norms
//   * lamb_apply:    per chunk: u again from p, m', v' (the same function, the same bits),
//                    p' = p - (lr_t ratio_t) u
// 10 model-sized streams (6 + 4), 11 with clipping; no scratch buffer of the model's size.  No
// host round trip and nothing step-dependent in a kernel argument: a captured step replays
// correctly.  No atomics; grids, partial sums and their order follow from the layout alone, so
// the same buffers give the same bits on every call, machine and rank.  The alignment gaps
// between tensors belong to no chunk: they are neither read nor written.
#include "common.h"
#include "lamb_math.h"
#include "ops.h"

namespace ddlpc {

namespace {

constexpr int LT = kLambThreads;
static_assert(kLambChunk == 4 * LT, "one float4 per thread covers a chunk");

struct Chunk {
  long long tensor, begin;
  int quads, rem;            // float4s of the chunk (256 unless it is a tensor's last), 0..3 more floats
};

DDLPC_DEVICE Chunk chunk_of(const long long* __restrict__ chunks) {
  const long long* c = chunks + 3 * (long long)blockIdx.x;
  const int len = (int)c[2];
  return Chunk{c[0], c[1], len >> 2, len & 3};
}

// The halving tree over the 256 thread sums of N quantities: thread k adds the sum of thread
// k + s for s = 128, 64 through LDS, then wave 0 for s = 32 .. 1 by lane shifts (the same
// additions in the same order as a tree all in LDS).  The result is thread 0's acc.
template <int N>
DDLPC_DEVICE void tree_sum(double (&acc)[N], double (*red)[LT]) {
  const int k = threadIdx.x;
#pragma unroll
  for (int q = 0; q < N; ++q) red[q][k] = acc[q];
  __syncthreads();
  if (k < 128) {
#pragma unroll
    for (int q = 0; q < N; ++q) red[q][k] += red[q][k + 128];
  }
  __syncthreads();
  if (k < 64) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      double a = red[q][k] + red[q][k + 64];
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) a += __shfl_down(a, s, 64);
      acc[q] = a;
    }
  }
}

__global__ __launch_bounds__(LT) void lamb_gradnorm_kernel(const float* __restrict__ g,
                                                           const long long* __restrict__ chunks,
                                                           double* __restrict__ gpartial) {
  __shared__ double red[1][LT];
  const Chunk c = chunk_of(chunks);
  const int k = threadIdx.x;
  double acc[1] = {0.0};
  if (k < c.quads) {
    const float4 gg = reinterpret_cast<const float4*>(g + c.begin)[k];
    acc[0] += (double)gg.x * (double)gg.x;
    acc[0] += (double)gg.y * (double)gg.y;
    acc[0] += (double)gg.z * (double)gg.z;
    acc[0] += (double)gg.w * (double)gg.w;
  }
  if (k < c.rem) {
    const float x = g[c.begin + 4 * c.quads + k];
    acc[0] += (double)x * (double)x;
  }
  tree_sum(acc, red);
  if (k == 0) gpartial[blockIdx.x] = acc[0];
}

// one workgroup: thread k adds gpartial[k], gpartial[k + 256], ... in that order, the tree
// combines the 256 sums, thread 0 writes the table (nc = 0: clipping off)
__global__ __launch_bounds__(LT) void lamb_scalars_kernel(float* __restrict__ s,
                                                          const double* __restrict__ gpartial, int nc,
                                                          SchedArgs a) {
  __shared__ double red[1][LT];
  double acc[1] = {0.0};
  for (int k = threadIdx.x; k < nc; k += LT) acc[0] += gpartial[k];
  tree_sum(acc, red);
  if (threadIdx.x == 0) lamb_scalars(s, a, acc[0]);
}

__global__ __launch_bounds__(LT) void lamb_moments_kernel(const float* __restrict__ p,
                                                          const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          const long long* __restrict__ chunks,
                                                          const long long* __restrict__ tensors,
                                                          const float* __restrict__ scal,
                                                          double* __restrict__ partial, LambHyper h) {
  __shared__ double red[2][LT];
  const Chunk c = chunk_of(chunks);
  const float ibc1 = scal[1], isb2 = scal[2], coef = scal[5];
  const float wdt = tensors[3 * c.tensor + 2] != 0 ? h.wd : 0.f;
  const int k = threadIdx.x;
  double acc[2] = {0.0, 0.0};           // sum p^2, sum u^2
  if (k < c.quads) {
    const float4 pp = reinterpret_cast<const float4*>(p + c.begin)[k];
    const float4 gg = reinterpret_cast<const float4*>(g + c.begin)[k];
    float4 mm = reinterpret_cast<float4*>(m + c.begin)[k];
    float4 vv = reinterpret_cast<float4*>(v + c.begin)[k];
    const float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lamb_moments(G[j], coef, h, M[j], V[j]);
      const float u = lamb_u(P[j], M[j], V[j], ibc1, isb2, h.eps, wdt);
      acc[0] += (double)P[j] * (double)P[j];
      acc[1] += (double)u * (double)u;
    }
    reinterpret_cast<float4*>(m + c.begin)[k] = mm;
    reinterpret_cast<float4*>(v + c.begin)[k] = vv;
  }
  if (k < c.rem) {
    const long long i = c.begin + 4 * c.quads + k;
    const float pi = p[i];
    float mi = m[i], vi = v[i];
    lamb_moments(g[i], coef, h, mi, vi);
    const float u = lamb_u(pi, mi, vi, ibc1, isb2, h.eps, wdt);
    acc[0] += (double)pi * (double)pi;
    acc[1] += (double)u * (double)u;
    m[i] = mi;
    v[i] = vi;
  }
  tree_sum(acc, red);
  if (k == 0) {
    partial[2 * (long long)blockIdx.x] = acc[0];
    partial[2 * (long long)blockIdx.x + 1] = acc[1];
  }
}

// one workgroup per tensor: thread k adds the sums of the tensor's chunks k, k + 256, ...
__global__ __launch_bounds__(LT) void lamb_ratios_kernel(const long long* __restrict__ tensors,
                                                         const double* __restrict__ partial,
                                                         float* __restrict__ ratio,
                                                         float* __restrict__ norms) {
  __shared__ double red[2][LT];
  const long long* t = tensors + 3 * (long long)blockIdx.x;
  const long long first = t[0], count = t[1];
  double acc[2] = {0.0, 0.0};
  for (long long j = threadIdx.x; j < count; j += LT) {
    acc[0] += partial[2 * (first + j)];
    acc[1] += partial[2 * (first + j) + 1];
  }
  tree_sum(acc, red);
  if (threadIdx.x == 0) lamb_ratio(acc[0], acc[1], t[2] != 0, ratio + blockIdx.x, norms + 2 * blockIdx.x);
}

__global__ __launch_bounds__(LT) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                        const float* __restrict__ v,
                                                        const long long* __restrict__ chunks,
                                                        const long long* __restrict__ tensors,
                                                        const float* __restrict__ scal,
                                                        const float* __restrict__ ratio, LambHyper h) {
  const Chunk c = chunk_of(chunks);
  const float ibc1 = scal[1], isb2 = scal[2];
  const float wdt = tensors[3 * c.tensor + 2] != 0 ? h.wd : 0.f;
  const float step = mul_rn(scal[3], ratio[c.tensor]);
  const int k = threadIdx.x;
  if (k < c.quads) {
    float4 pp = reinterpret_cast<float4*>(p + c.begin)[k];
    const float4 mm = reinterpret_cast<const float4*>(m + c.begin)[k];
    const float4 vv = reinterpret_cast<const float4*>(v + c.begin)[k];
    float* P = &pp.x; const float* M = &mm.x; const float* V = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      P[j] = lamb_apply(P[j], lamb_u(P[j], M[j], V[j], ibc1, isb2, h.eps, wdt), step);
    reinterpret_cast<float4*>(p + c.begin)[k] = pp;
  }
  if (k < c.rem) {
    const long long i = c.begin + 4 * c.quads + k;
    p[i] = lamb_apply(p[i], lamb_u(p[i], m[i], v[i], ibc1, isb2, h.eps, wdt), step);
  }
}

}  // namespace

void lamb_step_launch(float* p, const float* g, float* m, float* v, float* scal, const long long* chunks,
                      int nchunks, const long long* tensors, int ntensors, double* partial, float* ratio,
                      float* norms, const SchedArgs& a, const LambHyper& h, hipStream_t st) {
  double* gpartial = partial + 2 * (long long)nchunks;
  const bool clip = a.max_norm > 0.0 && nchunks > 0;
  if (clip)
    hipLaunchKernelGGL(lamb_gradnorm_kernel, dim3(nchunks), dim3(LT), 0, st, g, chunks, gpartial);
  hipLaunchKernelGGL(lamb_scalars_kernel, dim3(1), dim3(LT), 0, st, scal, gpartial, clip ? nchunks : 0, a);
  if (nchunks == 0) return;             // (the step counter advances, as in adam_step_sched)
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(nchunks), dim3(LT), 0, st, p, g, m, v, chunks, tensors, scal,
                     partial, h);
  hipLaunchKernelGGL(lamb_ratios_kernel, dim3(ntensors), dim3(LT), 0, st, tensors, partial, ratio, norms);
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(nchunks), dim3(LT), 0, st, p, m, v, chunks, tensors, scal, ratio,
                     h);
}

}  // namespace ddlpc
