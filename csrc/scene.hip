// Whole-scene prediction (overlap-tile inference): the two kernels around the network.
//
// The reference only dumps the arg-max of a few training tiles (ref.py:785-790); a scene is
// predicted here from overlapping windows whose class probabilities are blended in an fp32
// accumulator (ddlpc/infer.py holds the window plan, head_ce.hip the accumulating head):
//
//   * window_gather_kernel: the scene is uploaded ONCE as uint8 [H, W, Cin]; a batch of
//     windows (origins may be negative / overhang: the scene is mirrored at its borders,
//     edge pixel not repeated) is cut out directly in the first conv's input layout —
//     channel-last bf16, /255 by IEEE division as tile_gather_kernel, channels zero-padded to
//     cpad (8 = one 16-byte store per pixel).
//   * scene_finalize_kernel: accumulator [H, W, KA] -> uint8 class map (arg-max over the K
//     class channels, lowest class on ties) and, with labels, the K x K confusion matrix:
//     counted per workgroup in LDS, then added to HBM with integer atomics (integer sums do
//     not depend on their order: reproducible).
#include "common.h"
#include "ops.h"

namespace ddlpc {

namespace {

__global__ __launch_bounds__(256) void window_gather_kernel(
    const uint8_t* __restrict__ scene, const int* __restrict__ origins, int B, int H, int W,
    int in_ch, int tile, int cpad, bf16_t* __restrict__ x) {
  const long long S = (long long)tile * tile;
  const long long total = (long long)B * S;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(e / S);
    const int p = (int)(e - (long long)b * S);
    const int wy = p / tile, wx = p - wy * tile;
    const int sy = reflect_index(origins[2 * b] + wy, H);
    const int sx = reflect_index(origins[2 * b + 1] + wx, W);
    const uint8_t* sp = scene + ((long long)sy * W + sx) * in_ch;
    float f[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = c < in_ch ? __fdiv_rn((float)sp[c], 255.0f) : 0.f;
    if (cpad == 8) {
      reinterpret_cast<uint4*>(x)[e] = pack8(f);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < cpad) x[e * cpad + c] = f2bf(f[c]);
    }
  }
}

constexpr int kMaxK = 16;

__global__ __launch_bounds__(256) void scene_finalize_kernel(
    const float* __restrict__ acc, long long P, int K, int KA, const uint8_t* __restrict__ labels,
    int ignore_index, uint8_t* __restrict__ pred, unsigned long long* __restrict__ cm) {
  __shared__ unsigned int hist[kMaxK * kMaxK];
  if (labels != nullptr) {
    for (int i = threadIdx.x; i < K * K; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
  }
  const int nq = (K + 3) / 4;
  for (long long px = blockIdx.x * (long long)blockDim.x + threadIdx.x; px < P;
       px += (long long)gridDim.x * blockDim.x) {
    const float4* ap = reinterpret_cast<const float4*>(acc + px * KA);
    float m = 0.f;
    int am = 0;
    for (int q = 0; q < nq; ++q) {
      const float4 v = ap[q];
      const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j;
        if (k < K && (k == 0 || f[j] > m)) { m = f[j]; am = k; }
      }
    }
    pred[px] = (uint8_t)am;
    if (labels != nullptr) {
      const int l = labels[px];
      if (l < K && l != ignore_index) atomicAdd(&hist[l * K + am], 1u);
    }
  }
  if (labels != nullptr) {
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += blockDim.x)
      if (hist[i] != 0u) atomicAdd(&cm[i], (unsigned long long)hist[i]);
  }
}

int scene_grid(long long total) {
  return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 4096));
}

}  // namespace

void window_gather_launch(const uint8_t* scene, const int* origins, int B, int H, int W, int in_ch,
                          int tile, int cpad, bf16_t* x, hipStream_t st) {
  hipLaunchKernelGGL(window_gather_kernel, dim3(scene_grid((long long)B * tile * tile)), dim3(256),
                     0, st, scene, origins, B, H, W, in_ch, tile, cpad, x);
}

void scene_finalize_launch(const float* acc, long long P, int K, int KA, const uint8_t* labels,
                           int ignore_index, uint8_t* pred, int64_t* cm, hipStream_t st) {
  hipLaunchKernelGGL(scene_finalize_kernel, dim3(scene_grid(P)), dim3(256), 0, st, acc, P, K, KA,
                     labels, ignore_index, pred, reinterpret_cast<unsigned long long*>(cm));
}

}  // namespace ddlpc
