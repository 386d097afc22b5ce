// Label distance transform and boundary erosion (label_dist2, label_erode): one kernel template,
// two epilogues.  The recipe is label_math.h; this file is its gfx950 work split.
//
// The ISPRS "eroded boundaries" score sheet leaves out every pixel within 3 px of a class border.
// The labels at hand are cut (and resampled) on the device, so the band is computed on the device,
// in front of the unchanged head / scene kernels, which already skip ignored pixels.
//
//   * Work split.  A 256-thread workgroup owns a 32 x 32 output tile of one image; the grid is
//     ceil(W / 32) x ceil(H / 32) x B, a function of the shape alone.  No atomics: results are
//     bit-identical on every call.
//   * Staging.  The tile and a 16-pixel halo on each side are 64 rows x 64 columns, so a staged row
//     is one wave-wide read with lane = column (one coalesced 512-byte read per int64 row) and one
//     64-bit word per class.  Each lane classifies its pixel (label_class; outside the image =
//     invalid), five wave ballots give the row's validity word and the four bit planes of the class
//     codes, and lane k < 16 forms ne[row][k] = valid & ~(class == k) from them (other_mask) and
//     writes it to LDS: ne[64][16] uint64 = 8 KB.  Labels never sit in LDS as bytes.
//   * Distance phase.  A thread owns 4 output pixels (column tid & 31, rows tid >> 5 + 8 j), whose
//     own labels it read during staging (class code, and the value an un-eroded pixel keeps); it
//     makes no global read.  Per pixel and dy: one LDS word ne[row + dy][class], the nearest set
//     bit on either side by shifts, a count-trailing-zeros and a count-leading-zeros, and a
//     multiply-add (nearest_dx, pixel_dist2): no inner x loop.  Lanes of a row that share a class
//     read the same LDS word (broadcast).
//   * Epilogues.  DIST stores d2 (int32); ERODE stores `fill` where a valid pixel has d2 <= r^2 and
//     the label itself elsewhere, and never materialises d2.
//
// Where this departs from the first sketch of the design, and why:
//   * 5 ballots per row (validity + 4 bit planes) instead of one per class: the count does not
//     grow with K, and lane k rebuilds its class's word with four 64-bit selects.
//   * LDS holds ne = valid & ~eq per class instead of eq per class and a validity word per row:
//     the distance phase reads one word per step instead of two.
//   * ERODE walks |dy| <= r only, not 33 rows: a pixel with d2 <= r^2 has its witness within r
//     rows, so the decision is exact (label_math.h, pixel_dist2) at 2 r + 1 steps, 7 for r = 3.
//   * The 4 own labels are read from global memory (a second, L2-resident read of the tile's
//     centre) rather than decoded from the LDS words: an invalid pixel's value cannot be decoded,
//     and the erosion copies it through.
//
// Build figures (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): 42 VGPRs
// for the int64 instantiations, 38 for the uint8 ones (DIST and ERODE alike), 35-37 SGPRs, LDS
// 8192 bytes per workgroup, scratch 0 bytes (no spill), occupancy 8 waves per SIMD.
#include <type_traits>

#include "common.h"
#include "label_math.h"
#include "ops.h"

namespace ddlpc {

namespace {

constexpr int kRowsPerWave = kLabelStage / 4;     // 4 waves stage 16 rows each
constexpr int kOwn = kLabelTile * kLabelTile / 256;   // output pixels per thread
static_assert(kLabelStage == kWave, "a staged row is one wave-wide read");

template <typename T, bool ERODE>
__global__ __launch_bounds__(256) void label_boundary_kernel(
    const T* __restrict__ labels, int H, int W, int K, int ignore_index, int radius, int fill,
    typename std::conditional<ERODE, T, int>::type* __restrict__ out) {
  __shared__ uint64_t s_ne[kLabelStage * kLabelMaxK];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int x0 = blockIdx.x * kLabelTile, y0 = blockIdx.y * kLabelTile;
  const long long img = (long long)blockIdx.z * H * W;
  const T* __restrict__ lp = labels + img;

  // own pixels: column lx, rows ly0 + 8 j of the tile
  const int lx = tid & (kLabelTile - 1), ly0 = tid / kLabelTile;
  const int ox = x0 + lx;
  T own[kOwn];
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int oy = y0 + ly0 + 8 * j;
    own[j] = (oy < H && ox < W) ? lp[(long long)oy * W + ox] : (T)0;
  }

  // staging: wave w rows 16 w .. 16 w + 15 of the stage, lane = column
  const int sx = x0 - kLabelR + lane;
  const bool col_in = sx >= 0 && sx < W;
  int code[kRowsPerWave];
#pragma unroll
  for (int i = 0; i < kRowsPerWave; ++i) {
    const int sy = y0 - kLabelR + wave * kRowsPerWave + i;
    code[i] = -1;
    if (col_in && sy >= 0 && sy < H) code[i] = label_class((long long)lp[(long long)sy * W + sx], K, ignore_index);
  }
#pragma unroll
  for (int i = 0; i < kRowsPerWave; ++i) {
    const uint64_t valid = __ballot(code[i] >= 0);
    uint64_t plane[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) plane[j] = __ballot((code[i] >> j) & 1);
    if (lane < kLabelMaxK) s_ne[(wave * kRowsPerWave + i) * kLabelMaxK + lane] = other_mask(valid, plane, lane);
  }
  __syncthreads();

  const int reach = ERODE ? radius : kLabelR;
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int ly = ly0 + 8 * j, oy = y0 + ly;
    if (oy >= H || ox >= W) continue;
    const int cls = label_class((long long)own[j], K, ignore_index);
    const int d2 = label_dist2_at(s_ne, ly + kLabelR, lx + kLabelR, cls, reach);
    const long long e = img + (long long)oy * W + ox;
    if constexpr (ERODE)
      out[e] = label_eroded(cls, d2, radius) ? (T)fill : own[j];
    else
      out[e] = d2;
  }
}

template <typename T>
void launch_t(const T* labels, int B, int H, int W, int K, int ignore_index, int radius, int fill,
              void* out, hipStream_t st) {
  const dim3 grid((unsigned)label_tiles(W), (unsigned)label_tiles(H), (unsigned)B);
  if (radius < 0)
    hipLaunchKernelGGL((label_boundary_kernel<T, false>), grid, dim3(256), 0, st, labels, H, W, K,
                       ignore_index, 0, 0, static_cast<int*>(out));
  else
    hipLaunchKernelGGL((label_boundary_kernel<T, true>), grid, dim3(256), 0, st, labels, H, W, K,
                       ignore_index, radius, fill, static_cast<T*>(out));
}

}  // namespace

int label_tiles(int n) { return (n + kLabelTile - 1) / kLabelTile; }

void label_boundary_launch(const void* labels, bool u8, int B, int H, int W, int K, int ignore_index,
                           int radius, int fill, void* out, hipStream_t st) {
  if (u8)
    launch_t(static_cast<const uint8_t*>(labels), B, H, W, K, ignore_index, radius, fill, out, st);
  else
    launch_t(static_cast<const int64_t*>(labels), B, H, W, K, ignore_index, radius, fill, out, st);
}

}  // namespace ddlpc
