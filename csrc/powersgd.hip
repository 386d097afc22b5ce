// Low-rank gradient codec with error feedback (PowerSGD): per bucket every weight gradient, viewed
// as an n x m matrix A = residual + gradient, is sent as two thin factors P (n x r) and Q (m x r)
// that are summed by plain all-reduces; what the factors do not carry stays in the residual.
// parallel/codec.py holds the contract, powersgd_math.h the tables, the item geometry and the
// element function shared with the CPU twins.
//
// Five kernels, each ONE launch per bucket driven by the tables: blockIdx.x is a work item, the
// workgroup finds its (tensor, block) by walking the table (ten or so rows), so the grid is a
// function of the table alone, every output element has one fixed owner, there are no float
// atomics and nothing depends on the CU count.  256 threads = 4 waves everywhere.
//
//   project        item = (tensor, 16-row block).  A 16 x K strip of A against q_prev on
//                  v_mfma_f32_16x16x4_f32, r padded to the 16-wide N tile with zero columns.  Lane l
//                  loads one float4 of row l & 15 at k-quad l >> 4 of a 16-wide K step (16-byte
//                  loads where the address allows, guarded scalars otherwise), adds e + g, stores e,
//                  and feeds element t of the quad to MFMA t — the k permutation is free inside a
//                  sum, the B fragment applies the same one.  K moves in chunks of 256: the chunk's
//                  q_prev rows sit in LDS as [k][16] (zero padded; a B read takes 16 consecutive floats
//                  per k-quad, the four quads of a wave 64 floats apart: they share banks, a 2-way
//                  conflict per half-wave), wave w owns the chunk's k range
//                  [64 w, 64 w + 64) — four consecutive steps, so a row's 256 bytes are one run of
//                  loads.  The four accumulators are combined through LDS in wave order.
//   orthonormalize item = tensor.  Modified Gram-Schmidt over the r columns.  Thread k owns rows k,
//                  k + 256, ... of P for the whole kernel, so P itself needs no exchange: only the
//                  fp64 sums are shared (a shuffle butterfly per wave, the four waves in order).
//   backproject    item = (tensor, 64-column block), lane = column, so a row's loads are coalesced.
//                  P-hat moves through LDS in chunks of 256 rows ([row][16], zero padded, read as
//                  broadcasts); wave w takes the chunk's rows w, w + 4, ... in ascending order
//                  with 16 accumulators in registers; the waves are combined in wave order.
//   residual /     item = (tensor, 16-row x 256-column tile).  The tile's P-hat rows and (transposed)
//   decode         Q rows sit in LDS; a thread forms 4 rows x 4 consecutive columns with psgd_dot and
//                  stores 16 bytes where the address allows.
// The raw spans (biases, BatchNorm weights) ride in the project and decode launches as extra items.
#include "common.h"
#include "ops.h"
#include "powersgd_math.h"

namespace ddlpc {

namespace {

constexpr int NT = 256, RK = kPsgdMaxRank;
static_assert(kPsgdRows == 16 && kPsgdCols == NT && kPsgdBpCols == 64 && kPsgdRawChunk == 4 * NT, "item geometry");

struct Low { int off, n, m, p_off, q_off; };

DDLPC_DEVICE Low low_row(const int* __restrict__ low, int t) {
  return Low{low[5 * t], low[5 * t + 1], low[5 * t + 2], low[5 * t + 3], low[5 * t + 4]};
}

// the tensor that owns work item `item` when tensor t holds cnt(n, m) items; item becomes the index
// inside that tensor.  -> T with item reduced by every tensor's count when it lies past them
template <class F>
DDLPC_DEVICE int find_item(const int* __restrict__ low, int T, int& item, F cnt) {
  int t = 0;
  for (; t < T; ++t) {
    const int c = cnt(low[5 * t + 1], low[5 * t + 2]);
    if (item < c) break;
    item -= c;
  }
  return t;
}

DDLPC_DEVICE bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// raw chunk `item` of the raw table: dst[wire_off + i] = scale * src[off + i] (TO_WIRE), or
// dst[off + i] = src[wire_off + i]
template <bool TO_WIRE>
DDLPC_DEVICE void raw_item(const int* __restrict__ raw, int R, int item, const float* __restrict__ src,
                           float* __restrict__ dst, float scale) {
  int s = 0;
  for (; s < R; ++s) {
    const int c = (raw[3 * s + 1] + kPsgdRawChunk - 1) / kPsgdRawChunk;
    if (item < c) break;
    item -= c;
  }
  if (s == R) return;
  const long long off = raw[3 * s], wire = raw[3 * s + 2];
  const int len = raw[3 * s + 1];
  const long long i0 = (long long)item * kPsgdRawChunk;           // (len may lie within a chunk of 2^31)
  for (long long i = i0 + threadIdx.x; i < min((long long)len, i0 + kPsgdRawChunk); i += NT) {
    if (TO_WIRE) dst[wire + i] = mul_rn(scale, src[off + i]);
    else dst[off + i] = src[wire + i];
  }
}

__global__ __launch_bounds__(NT) void psgd_project_kernel(const float* __restrict__ g, float* e,
                                                         const float* __restrict__ q, float* __restrict__ wire_p,
                                                         const int* __restrict__ low, int T,
                                                         const int* __restrict__ raw, int R, int r, float w) {
  __shared__ __attribute__((aligned(16))) float qs[kPsgdCols * RK];      // [k][16]; then the 4 accumulators
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int item = blockIdx.x;
  const int t = find_item(low, T, item, [](int n, int) { return (n + kPsgdRows - 1) / kPsgdRows; });
  if (t == T) {
    raw_item<true>(raw, R, item, g, wire_p, w);
    return;
  }
  const Low L = low_row(low, t);
  const int row0 = item * kPsgdRows, row = row0 + (lane & 15), kq = lane >> 4;
  const long long rbase = (long long)L.off + (long long)row * L.m;       // (used where row < n)
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < L.m; kb += kPsgdCols) {
    __syncthreads();                                 // the chunk before has been read
    for (int i = tid; i < kPsgdCols * RK; i += NT) {
      const int k = kb + (i >> 4), j = i & 15;
      qs[i] = (j < r && k < L.m) ? q[(long long)L.q_off + (long long)k * r + j] : 0.f;
    }
    __syncthreads();
    const int kw = kb + wave * 64;
    if (kw >= L.m) continue;                         // (wave-uniform; the barriers stand above)
    float a[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k0 = kw + s * 16 + kq * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) a[s][j] = 0.f;     // rows past n, k past m: zeros
      if (row < L.n && k0 < L.m) {
        float* pe = e + rbase + k0;
        const float* pg = g + rbase + k0;
        if (k0 + 4 <= L.m && aligned16(pe) && aligned16(pg)) {
          const f32x4_t ve = *reinterpret_cast<const f32x4_t*>(pe), vg = *reinterpret_cast<const f32x4_t*>(pg);
          const f32x4_t va = {add_rn(ve.x, vg.x), add_rn(ve.y, vg.y), add_rn(ve.z, vg.z), add_rn(ve.w, vg.w)};
          *reinterpret_cast<f32x4_t*>(pe) = va;
          a[s][0] = va.x; a[s][1] = va.y; a[s][2] = va.z; a[s][3] = va.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k0 + j < L.m) {
              a[s][j] = add_rn(pe[j], pg[j]);
              pe[j] = a[s][j];
            }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][j], qs[((wave * 64 + s * 16 + kq * 4 + j) << 4) + (lane & 15)],
                                                   acc, 0, 0, 0);
  }
  __syncthreads();                                   // qs is free: the accumulators take its place
  float* red = qs;                                   // [wave][16 rows][16 columns]
#pragma unroll
  for (int v = 0; v < 4; ++v) red[wave * 256 + (4 * kq + v) * 16 + (lane & 15)] = acc[v];
  __syncthreads();
  const int i = tid >> 4, j = tid & 15;
  const float sum = add_rn(add_rn(add_rn(red[tid], red[256 + tid]), red[512 + tid]), red[768 + tid]);
  if (row0 + i < L.n && j < r) wire_p[(long long)L.p_off + (long long)(row0 + i) * r + j] = mul_rn(w, sum);
}

__global__ __launch_bounds__(NT) void psgd_orth_kernel(float* wire_p, const int* __restrict__ low, int r) {
  __shared__ double red[RK][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Low L = low_row(low, blockIdx.x);
  float* P = wire_p + L.p_off;
  for (int i = 0; i < r; ++i) {
    double s2 = 0.0;
    for (int row = tid; row < L.n; row += NT) {
      const double v = P[(long long)row * r + i];
      s2 = fma(v, v, s2);
    }
    s2 = wave_sum_d(s2);
    if (lane == 0) red[0][wave] = s2;
    __syncthreads();
    const double tot = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const float s = psgd_inv_norm(tot);
    double acc[RK];
#pragma unroll
    for (int k = 0; k < RK; ++k) acc[k] = 0.0;
    for (int row = tid; row < L.n; row += NT) {
      float* pr = P + (long long)row * r;
      const float qi = tot == 0.0 ? 0.f : mul_rn(pr[i], s);
      pr[i] = qi;
#pragma unroll
      for (int k = 1; k < RK; ++k)
        if (k > i && k < r) acc[k] = fma((double)qi, (double)pr[k], acc[k]);
    }
    __syncthreads();                                 // red[0] has been read by every thread
#pragma unroll
    for (int k = 1; k < RK; ++k)
      if (k > i && k < r) {                          // (workgroup-uniform)
        const double v = wave_sum_d(acc[k]);
        if (lane == 0) red[k][wave] = v;
      }
    __syncthreads();
    float d[RK];
#pragma unroll
    for (int k = 1; k < RK; ++k)
      d[k] = (k > i && k < r) ? (float)(((red[k][0] + red[k][1]) + red[k][2]) + red[k][3]) : 0.f;
    for (int row = tid; row < L.n; row += NT) {
      float* pr = P + (long long)row * r;
      const float qi = pr[i];
#pragma unroll
      for (int k = 1; k < RK; ++k)
        if (k > i && k < r) pr[k] = __builtin_fmaf(-d[k], qi, pr[k]);
    }
    __syncthreads();                                 // red is free for the next column
  }
}

__global__ __launch_bounds__(NT) void psgd_backproject_kernel(const float* __restrict__ e,
                                                             const float* __restrict__ wire_p,
                                                             float* __restrict__ q_loc, float* __restrict__ wire_q,
                                                             const int* __restrict__ low, int T, int r, float w) {
  __shared__ __attribute__((aligned(16))) float ph[NT * RK];             // P-hat rows of the chunk, [row][16]
  __shared__ float red[4 * RK * kPsgdBpCols];                            // [wave][j][column]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int item = blockIdx.x;
  const int t = find_item(low, T, item, [](int, int m) { return (m + kPsgdBpCols - 1) / kPsgdBpCols; });
  if (t == T) return;
  const Low L = low_row(low, t);
  const int c0 = item * kPsgdBpCols, c = c0 + lane;
  float acc[RK];
#pragma unroll
  for (int j = 0; j < RK; ++j) acc[j] = 0.f;
  for (int rb = 0; rb < L.n; rb += NT) {
    __syncthreads();
    for (int i = tid; i < NT * RK; i += NT) {
      const int row = rb + (i >> 4), j = i & 15;
      ph[i] = (row < L.n && j < r) ? wire_p[(long long)L.p_off + (long long)row * r + j] : 0.f;
    }
    __syncthreads();
    const int rows = min(NT, L.n - rb);
    if (c < L.m) {
      const float* col = e + (long long)L.off + (long long)rb * L.m + c;
#pragma unroll 4
      for (int i = wave; i < rows; i += 4) {
        const float a = col[(long long)i * L.m];
#pragma unroll
        for (int j = 0; j < RK; ++j) acc[j] = __builtin_fmaf(a, ph[i * RK + j], acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RK; ++j) red[(wave * RK + j) * kPsgdBpCols + lane] = acc[j];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = tid + NT * u, cc = o >> 4, j = o & 15;
    const float sum = add_rn(add_rn(add_rn(red[j * kPsgdBpCols + cc], red[(RK + j) * kPsgdBpCols + cc]),
                                    red[(2 * RK + j) * kPsgdBpCols + cc]), red[(3 * RK + j) * kPsgdBpCols + cc]);
    if (c0 + cc < L.m && j < r) {
      const long long at = (long long)L.q_off + (long long)(c0 + cc) * r + j;
      q_loc[at] = sum;
      wire_q[at] = mul_rn(w, sum);
    }
  }
}

// RESID: out = e, e <- e - P-hat Q_loc^T.  Else: out = g, g <- P-hat Q^T and the raw spans from wire_p.
template <bool RESID>
__global__ __launch_bounds__(NT) void psgd_tile_kernel(float* out, const float* __restrict__ wire_p,
                                                      const float* __restrict__ qv, const int* __restrict__ low,
                                                      int T, const int* __restrict__ raw, int R, int r) {
  __shared__ float ps[kPsgdRows * RK];               // [row][16]
  __shared__ float qs[RK * kPsgdCols];               // [j][column]
  const int tid = threadIdx.x;
  int item = blockIdx.x;
  const int t = find_item(low, T, item, [](int n, int m) {
    return ((n + kPsgdRows - 1) / kPsgdRows) * ((m + kPsgdCols - 1) / kPsgdCols);
  });
  if (t == T) {
    if (!RESID) raw_item<false>(raw, R, item, wire_p, out, 1.f);
    return;
  }
  const Low L = low_row(low, t);
  const int ctiles = (L.m + kPsgdCols - 1) / kPsgdCols;
  const int row0 = (item / ctiles) * kPsgdRows, c0 = (item % ctiles) * kPsgdCols;
  {
    const int i = tid >> 4, j = tid & 15;
    ps[tid] = (row0 + i < L.n && j < r) ? wire_p[(long long)L.p_off + (long long)(row0 + i) * r + j] : 0.f;
  }
  for (int i = tid; i < kPsgdCols * r; i += NT) {
    const int cc = i / r, j = i - cc * r;
    qs[j * kPsgdCols + cc] = (c0 + cc < L.m) ? qv[(long long)L.q_off + (long long)c0 * r + i] : 0.f;
  }
  __syncthreads();
  const int cq = (tid & 63) * 4, rg = (tid >> 6) * 4;
  if (c0 + cq >= L.m) return;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int row = row0 + rg + rr;
    if (row >= L.n) break;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = psgd_dot(ps + (rg + rr) * RK, 1, qs + cq + u, kPsgdCols, r);
    float* po = out + (long long)L.off + (long long)row * L.m + c0 + cq;
    if (c0 + cq + 4 <= L.m && aligned16(po)) {
      f32x4_t x = {v[0], v[1], v[2], v[3]};
      if (RESID) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(po);
        x = f32x4_t{sub_rn(a.x, v[0]), sub_rn(a.y, v[1]), sub_rn(a.z, v[2]), sub_rn(a.w, v[3])};
      }
      *reinterpret_cast<f32x4_t*>(po) = x;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c0 + cq + u < L.m) po[u] = RESID ? sub_rn(po[u], v[u]) : v[u];
    }
  }
}

}  // namespace

void psgd_project_launch(const float* g, float* e, const float* q, float* wire_p, const int* low, int T,
                         const int* raw, int R, int r, float w, const PsgdCounts& c, hipStream_t st) {
  const long long grid = c.rowblocks + c.rawchunks;
  if (grid == 0) return;
  hipLaunchKernelGGL(psgd_project_kernel, dim3((unsigned)grid), dim3(NT), 0, st, g, e, q, wire_p, low, T, raw, R, r, w);
}

void psgd_orthonormalize_launch(float* wire_p, const int* low, int T, int r, hipStream_t st) {
  if (T == 0) return;
  hipLaunchKernelGGL(psgd_orth_kernel, dim3(T), dim3(NT), 0, st, wire_p, low, r);
}

void psgd_backproject_launch(const float* e, const float* wire_p, float* q_loc, float* wire_q, const int* low,
                             int T, int r, float w, const PsgdCounts& c, hipStream_t st) {
  if (c.colblocks == 0) return;
  hipLaunchKernelGGL(psgd_backproject_kernel, dim3((unsigned)c.colblocks), dim3(NT), 0, st, e, wire_p, q_loc, wire_q,
                     low, T, r, w);
}

void psgd_residual_launch(float* e, const float* wire_p, const float* q_loc, const int* low, int T, int r,
                          const PsgdCounts& c, hipStream_t st) {
  if (c.tiles == 0) return;
  hipLaunchKernelGGL(psgd_tile_kernel<true>, dim3((unsigned)c.tiles), dim3(NT), 0, st, e, wire_p, q_loc, low, T,
                     (const int*)nullptr, 0, r);
}

void psgd_decode_launch(float* g, const float* wire_p, const float* wire_q, const int* low, int T, const int* raw,
                        int R, int r, const PsgdCounts& c, hipStream_t st) {
  const long long grid = c.tiles + c.rawchunks;
  if (grid == 0) return;
  hipLaunchKernelGGL(psgd_tile_kernel<false>, dim3((unsigned)grid), dim3(NT), 0, st, g, wire_p, wire_q, low, T, raw, R, r);
}

}  // namespace ddlpc
