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
//     cpad (8 = one 16-byte store per pixel).  With a list of symmetry codes (test-time
//     augmentation) it cuts S views per window, window-major, read through crop_gather's
//     index map; a call without codes is the list {0}.
//   * scene_finalize_kernel: accumulator [H, W, KA] -> uint8 class map (arg-max over the K
//     class channels, lowest class on ties) and, with labels, the K x K confusion matrix:
//     counted per workgroup in LDS, then added to HBM with integer atomics (integer sums do
//     not depend on their order: reproducible).
#include "common.h"
#include "data_math.h"
#include "ops.h"

namespace ddlpc {

namespace {

// Window b under symmetry code c (test-time augmentation): network-side pixel (oy, ox) reads
// scene pixel (y0 + a, x0 + b), (a, b) = d4_forward (data_math.h; spelled out below), mirrored.
// Output [B * S, tile, tile, cpad], window-major: row b * S + j is window b under code j of
// `codes` (3 bits per code, code j at bits 3 j; a kernel argument, no device read).  Work split and
// LDS staging are crop_gather_kernel's (data.hip); LDS_T's A/B: scripts/predict_micro.py.
constexpr int kWinBS = 32;

template <bool LDS_T>
__global__ __launch_bounds__(256) void window_gather_kernel(
    const uint8_t* __restrict__ scene, const int* __restrict__ origins, int S, uint32_t codes, int H,
    int W, int nb, int in_ch, int tile, int cpad, bf16_t* __restrict__ x) {
  __shared__ uint2 s_px[kWinBS][kWinBS + 1];
  const int blk = blockIdx.x;
  const int v = blk / (nb * nb);             // view = b * S + j
  const int rem = blk - v * nb * nb;
  const int by = rem / nb, bx = rem - by * nb;
  const int b = v / S, j = v - b * S;
  const int code = (int)((codes >> (3 * j)) & 7u);
  const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
  const int lx = threadIdx.x & (kWinBS - 1), ly0 = threadIdx.x / kWinBS;
  constexpr int kRows = 256 / kWinBS;
  auto load = [&](int sy, int sx) {
    const uint8_t* sp = scene + ((long long)sy * W + sx) * in_ch;
    uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
    for (int ch = 0; ch < 8; ++ch)
      if (ch < in_ch) (ch < 4 ? w0 : w1) |= (uint32_t)sp[ch] << (8 * (ch & 3));
    return make_uint2(w0, w1);
  };
  const bool staged = LDS_T && (code & 4);
  if (staged) {
    // load role: r = ox - block origin (scene row), lanes along oy - block origin (scene column)
    for (int r = ly0; r < kWinBS; r += kRows) {
      const int ox = bx * kWinBS + r, oy = by * kWinBS + lx;
      if (ox < tile && oy < tile) {
        const int a = (code & 2) ? tile - 1 - ox : ox;
        const int c = (code & 1) ? tile - 1 - oy : oy;
        s_px[r][lx] = load(reflect_fast(y0 + a, H), reflect_fast(x0 + c, W));
      }
    }
    __syncthreads();
  }
  for (int ly = ly0; ly < kWinBS; ly += kRows) {
    const int oy = by * kWinBS + ly, ox = bx * kWinBS + lx;
    if (oy >= tile || ox >= tile) continue;
    uint2 px;
    if (staged) {
      px = s_px[lx][ly];
    } else {
      int a = (code & 4) ? ox : oy, c = (code & 4) ? oy : ox;
      if (code & 2) a = tile - 1 - a;
      if (code & 1) c = tile - 1 - c;
      px = load(reflect_fast(y0 + a, H), reflect_fast(x0 + c, W));
    }
    const uint32_t w[2] = {px.x, px.y};
    float f[8];
#pragma unroll
    for (int ch = 0; ch < 8; ++ch)
      f[ch] = ch < in_ch ? u8_unit((w[ch >> 2] >> (8 * (ch & 3))) & 0xffu) : 0.f;
    const long long e = ((long long)v * tile + oy) * tile + ox;
    if (cpad == 8) {
      reinterpret_cast<uint4*>(x)[e] = pack8(f);
    } else {
#pragma unroll
      for (int ch = 0; ch < 8; ++ch)
        if (ch < cpad) x[e * cpad + ch] = f2bf(f[ch]);
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

int window_gather_blocks(int tile) { return (tile + kWinBS - 1) / kWinBS; }

void window_gather_launch(const uint8_t* scene, const int* origins, int B, int S, uint32_t codes,
                          int H, int W, int in_ch, int tile, int cpad, bool lds_transpose, bf16_t* x,
                          hipStream_t st) {
  const int nb = window_gather_blocks(tile);
  const dim3 grid((unsigned)((long long)B * S * nb * nb));
  // a list without a transposing code never stages: the direct kernel runs the same
  // instructions without the LDS allocation (3% faster, docs/PERF.md)
  bool transposing = false;
  for (int j = 0; j < S; ++j) transposing |= ((codes >> (3 * j)) & 4u) != 0;
  if (lds_transpose && transposing)
    hipLaunchKernelGGL(window_gather_kernel<true>, grid, dim3(256), 0, st, scene, origins, S,
                       codes, H, W, nb, in_ch, tile, cpad, x);
  else
    hipLaunchKernelGGL(window_gather_kernel<false>, grid, dim3(256), 0, st, scene, origins, S,
                       codes, H, W, nb, in_ch, tile, cpad, x);
}

void scene_finalize_launch(const float* acc, long long P, int K, int KA, const uint8_t* labels,
                           int ignore_index, uint8_t* pred, int64_t* cm, hipStream_t st) {
  hipLaunchKernelGGL(scene_finalize_kernel, dim3(scene_grid(P)), dim3(256), 0, st, acc, P, K, KA,
                     labels, ignore_index, pred, reinterpret_cast<unsigned long long*>(cm));
}

}  // namespace ddlpc
