// Top-k gradient codec with error feedback (Deep Gradient Compression / memory SGD): per bucket
// segment every rank sends the k largest-magnitude entries of a = residual + gradient as
// (index, value) pairs and keeps the rest in the residual.  parallel/codec.py holds the contract
// (topk_encode / topk_decode_sum); these kernels are bit-exact against it.
//
//   key(i) = bits(a[i]) & 0x7fffffff, compared as an unsigned integer: non-negative floats order
//   like their bit patterns, +Inf lies above every finite value and every NaN pattern above +Inf
//   (the argument of codec_absmax_kernel in misc.hip), so non-finite entries rank first and are sent.
//   Ranking: key descending, then index ascending.  With the threshold key T (the k-th largest) and
//   m = k - #{key > T}, the selected set is every key > T plus the first m indices with key == T.
//
// Work split: a workgroup (256 threads, 4 waves) owns a FIXED chunk of kTopkChunk elements, the
// grid is ceil(n / kTopkChunk) — nothing depends on the CU count.  A chunk is walked in quads that
// start on a 16-byte boundary of the residual pointer: whole quads move as one 16-byte access, the
// quads cut by the chunk's (or the segment's) ends fall back to guarded scalar accesses.
//
// Encode = 9 plain launches on the caller's stream, no host read (state in an int32 scratch):
//   init                          state / bin tables <- 0, remaining k <- k
//   hist<0>, pick<0>              a = e + g written over e; histogram of key bits 30..20 (11 bits)
//   hist<1>, pick<1>              bits 19..10 of the keys whose top 11 bits equal the chosen prefix
//   hist<2>, pick<2>              bits  9..0  of the keys whose top 21 bits equal the prefix -> T, m
//   count                         (#key > T, #key == T) per chunk
//   compact                       ordered compaction + residual[selected] <- +0.0
// Three passes with a wide first digit instead of four 8-bit passes: one pass less over the segment,
// and 11 bits = the exponent and 3 mantissa bits, which already splits a gradient's few populated
// binades eight ways each; the price is 4 x 2048 counters (32 KB) of LDS per workgroup.
// Histograms: one copy per wave in LDS (ds_add_u32), merged by the workgroup, added to the
// segment's bin table with integer atomicAdd — integer counts do not depend on the order.
//
// Decode: a workgroup owns one tile of kTopkTile output floats in LDS; for each rank in order it
// binary-searches that rank's ascending index row for the tile's sub-range, its threads apply the
// (unique) indices with two separately rounded operations (mul, add), a barrier separates the
// ranks; the tile is stored with 16-byte stores.  No float atomics: rank-ordered by construction.
#include "common.h"
#include "ops.h"

namespace ddlpc {

namespace {

constexpr int CH = kTopkChunk, TL = kTopkTile, NB = kTopkBins, NT = 256;
constexpr int kStep = NT * 4;                       // elements of one workgroup step (a quad per thread)
static_assert(CH <= 16384 && CH % kStep == 0 && TL % kStep == 0, "chunk / tile geometry");

// int32 scratch: [0] prefix (key bits chosen so far), [1] remaining k, [2] T, [3] m,
// bins[kTopkPasses][NB], counts[chunks][2]
enum { S_PREFIX = 0, S_KREM = 1, S_T = 2, S_M = 3, S_BINS = 4, S_COUNTS = S_BINS + kTopkPasses * NB };

__host__ __device__ constexpr int digit_shift(int p) { return p == 0 ? 20 : p == 1 ? 10 : 0; }
__host__ __device__ constexpr int digit_bits(int p) { return p == 0 ? 11 : 10; }
static_assert(digit_shift(0) + digit_bits(0) == 31 && (1 << digit_bits(0)) == NB, "31-bit key");

// elements by which p lies past a 16-byte boundary
DDLPC_DEVICE int misalign4(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

struct Quad { uint32_t v[4]; };

// the 4 elements [i0, i0 + 4) of p as bit patterns, those outside [lo, hi) as 0; vec: p + i0 is
// 16-byte aligned (every quad start of a walk anchored on p's own alignment)
DDLPC_DEVICE Quad load_quad(const float* p, long long i0, long long lo, long long hi, bool vec) {
  Quad q;
  if (vec && i0 >= lo && i0 + 4 <= hi) {
    const u32x4_t t = *reinterpret_cast<const u32x4_t*>(p + i0);
    q.v[0] = t.x; q.v[1] = t.y; q.v[2] = t.z; q.v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = (i0 + j >= lo && i0 + j < hi) ? __float_as_uint(p[i0 + j]) : 0u;
  }
  return q;
}

DDLPC_DEVICE void store_quad(float* p, long long i0, long long lo, long long hi, const Quad& q) {
  if (i0 >= lo && i0 + 4 <= hi) {
    *reinterpret_cast<u32x4_t*>(p + i0) = u32x4_t{q.v[0], q.v[1], q.v[2], q.v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j >= lo && i0 + j < hi) p[i0 + j] = __uint_as_float(q.v[j]);
  }
}

DDLPC_DEVICE int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// set bits of a wave mask below this lane
DDLPC_DEVICE int lanes_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32),
                                        __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
}

__global__ __launch_bounds__(NT) void topk_init_kernel(int* __restrict__ scratch, int k) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < S_COUNTS) scratch[i] = i == S_KREM ? k : 0;
}

// PASS 0: a = e + g (one fp32 add) written over e, histogram of the top digit.
// PASS 1, 2: histogram of the next digit of the keys whose higher digits equal the prefix.
template <int PASS>
__global__ __launch_bounds__(NT) void topk_hist_kernel(const float* __restrict__ g, float* e, long long n,
                                                      int* __restrict__ scratch) {
  constexpr int SH = digit_shift(PASS), BITS = digit_bits(PASS);
  __shared__ unsigned int hist[4][NB];
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int i = tid; i < 4 * NB; i += NT) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const long long c0 = (long long)blockIdx.x * CH, c1 = min(n, c0 + (long long)CH);
  const int mis = misalign4(e);
  // g moves in 16-byte quads too where it shares e's alignment (slices of two flat buffers at
  // one offset do), else in scalars
  const bool gvec = ((reinterpret_cast<uintptr_t>(g) ^ reinterpret_cast<uintptr_t>(e)) & 15) == 0;
  const unsigned int prefix = PASS == 0 ? 0u : (unsigned int)scratch[S_PREFIX];
  for (long long i0 = c0 - mis + tid * 4; i0 < c1; i0 += kStep) {
    Quad a = load_quad(e, i0, c0, c1, true);
    if (PASS == 0) {
      const Quad gg = load_quad(g, i0, c0, c1, gvec);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        a.v[j] = __float_as_uint(__fadd_rn(__uint_as_float(a.v[j]), __uint_as_float(gg.v[j])));
      store_quad(e, i0, c0, c1, a);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned int key = a.v[j] & 0x7fffffffu;
      if (i0 + j >= c0 && i0 + j < c1 && (PASS == 0 || (key >> (SH + BITS)) == prefix))
        atomicAdd(&hist[wave][(key >> SH) & ((1u << BITS) - 1u)], 1u);
    }
  }
  __syncthreads();
  unsigned int* bins = reinterpret_cast<unsigned int*>(scratch) + S_BINS + PASS * NB;
  for (int b = tid; b < (1 << BITS); b += NT) {
    const unsigned int s = hist[0][b] + hist[1][b] + hist[2][b] + hist[3][b];
    if (s != 0u) atomicAdd(&bins[b], s);
  }
}

// one workgroup: walk the pass's bins from the top to the digit where the running count crosses
// the remaining k; prefix <- (prefix, digit), remaining k -= count above; last pass: T, m
template <int PASS>
__global__ __launch_bounds__(NT) void topk_pick_kernel(int* scratch) {
  constexpr int BITS = digit_bits(PASS), PER = (1 << BITS) / NT;
  __shared__ unsigned int wtot[4];
  const unsigned int* bins = reinterpret_cast<const unsigned int*>(scratch) + S_BINS + PASS * NB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned int c[PER], s = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) { c[j] = bins[tid * PER + j]; s += c[j]; }
  // suffix sums of the threads' totals: a shuffle scan inside the wave (after the step at
  // distance o a lane holds the sum of its next 2 o lanes), the waves above through LDS
  unsigned int suf = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int v = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += v;
  }
  if (lane == 0) wtot[wave] = suf;
  const unsigned int krem = (unsigned int)scratch[S_KREM], prefix = (unsigned int)scratch[S_PREFIX];
  __syncthreads();                                   // (every thread has read the state)
  unsigned int run = suf - s;                        // keys in the bins above this thread's
  for (int w = wave + 1; w < 4; ++w) run += wtot[w];
#pragma unroll
  for (int j = PER - 1; j >= 0; --j) {
    if (run < krem && run + c[j] >= krem) {          // true for exactly one bin
      const unsigned int p = (prefix << BITS) | (unsigned int)(tid * PER + j);
      scratch[S_PREFIX] = (int)p;
      scratch[S_KREM] = (int)(krem - run);
      if (PASS == kTopkPasses - 1) { scratch[S_T] = (int)p; scratch[S_M] = (int)(krem - run); }
    }
    run += c[j];
  }
}

__global__ __launch_bounds__(NT) void topk_count_kernel(const float* __restrict__ e, long long n,
                                                       int* __restrict__ scratch) {
  __shared__ int red[4][2];
  const int tid = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * CH, c1 = min(n, c0 + (long long)CH);
  const int mis = misalign4(e);
  const unsigned int T = (unsigned int)scratch[S_T];
  int ngt = 0, neq = 0;
  for (long long i0 = c0 - mis + tid * 4; i0 < c1; i0 += kStep) {
    const Quad a = load_quad(e, i0, c0, c1, true);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned int key = a.v[j] & 0x7fffffffu;
      const bool valid = i0 + j >= c0 && i0 + j < c1;
      ngt += valid && key > T;
      neq += valid && key == T;
    }
  }
  ngt = wave_sum_i(ngt); neq = wave_sum_i(neq);
  if ((tid & 63) == 0) { red[tid >> 6][0] = ngt; red[tid >> 6][1] = neq; }
  __syncthreads();
  if (tid < 2) scratch[S_COUNTS + 2 * blockIdx.x + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// Ordered compaction.  An element is selected iff key > T, or key == T and fewer than m equal keys
// precede it in the segment; its slot is (#key > T before it) + min(#key == T before it, m), so idx
// comes out ascending.  "Before it" = the preceding chunks' counts + the workgroup's running counts
// + the lower waves of this step (LDS) + the lower lanes (ballot + mbcnt) + the lane's own quad.
__global__ __launch_bounds__(NT) void topk_compact_kernel(float* e, long long n, int k,
                                                         const int* __restrict__ scratch,
                                                         int* __restrict__ idx, uint32_t* __restrict__ val) {
  __shared__ int red[2][4][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long c0 = (long long)blockIdx.x * CH, c1 = min(n, c0 + (long long)CH);
  const int mis = misalign4(e);
  const unsigned int T = (unsigned int)scratch[S_T];
  const int m = scratch[S_M];
  const int* counts = scratch + S_COUNTS;
  int sg = 0, se = 0;
  for (int b = tid; b < (int)blockIdx.x; b += NT) { sg += counts[2 * b]; se += counts[2 * b + 1]; }
  sg = wave_sum_i(sg); se = wave_sum_i(se);
  if (lane == 0) { red[1][wave][0] = sg; red[1][wave][1] = se; }
  __syncthreads();
  int gt_run = red[1][0][0] + red[1][1][0] + red[1][2][0] + red[1][3][0];
  int eq_run = red[1][0][1] + red[1][1][1] + red[1][2][1] + red[1][3][1];
  int par = 0;                                       // red[par]: this step's wave totals
  for (long long s0 = c0 - mis; s0 < c1; s0 += kStep, par ^= 1) {
    const long long i0 = s0 + tid * 4;
    const Quad a = load_quad(e, i0, c0, c1, true);
    bool gt[4], eq[4];
    int pg = 0, pe = 0, tg = 0, te = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned int key = a.v[j] & 0x7fffffffu;
      const bool valid = i0 + j >= c0 && i0 + j < c1;
      gt[j] = valid && key > T;
      eq[j] = valid && key == T;
      const unsigned long long bg = __ballot(gt[j]), be = __ballot(eq[j]);
      pg += lanes_below(bg); pe += lanes_below(be);
      tg += __popcll(bg); te += __popcll(be);
    }
    // the buffer of the step before last is free again: every thread passed the last barrier
    if (lane == 0) { red[par][wave][0] = tg; red[par][wave][1] = te; }
    __syncthreads();
    int stepg = 0, stepe = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int wg = red[par][w][0], we = red[par][w][1];
      if (w < wave) { pg += wg; pe += we; }
      stepg += wg; stepe += we;
    }
    int gb = gt_run + pg, eb = eq_run + pe;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (gt[j] || eq[j]) {
        const int slot = gb + min(eb, m);
        if ((gt[j] || eb < m) && slot < k) {
          idx[slot] = (int)(i0 + j);
          val[slot] = a.v[j];
          e[i0 + j] = 0.f;                           // sent: nothing left in the residual
        }
        gb += gt[j]; eb += eq[j];
      }
    }
    gt_run += stepg; eq_run += stepe;
  }
}

// first position of the ascending row whose value is >= target
DDLPC_DEVICE int lower_bound_i(const int* __restrict__ row, int k, long long target) {
  int a = 0, b = k;
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (row[mid] < target) a = mid + 1; else b = mid;
  }
  return a;
}

__global__ __launch_bounds__(NT) void topk_scatter_sum_kernel(float* __restrict__ out, long long n,
                                                             const int* __restrict__ idx,
                                                             const float* __restrict__ val,
                                                             const float* __restrict__ w, int world, int k) {
  __shared__ __attribute__((aligned(16))) float tile[TL];
  const int tid = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * TL - misalign4(out);     // out + t0: 16-byte aligned
  const long long lo = max(t0, 0LL), hi = min(n, t0 + (long long)TL);
  for (int i = tid; i < TL; i += NT) tile[i] = 0.f;
  __syncthreads();
  for (int r = 0; r < world; ++r) {
    const int* ir = idx + (long long)r * k;
    const float* vr = val + (long long)r * k;
    const float wr = w[r];
    const int ja = lower_bound_i(ir, k, lo), jb = lower_bound_i(ir, k, hi);
    for (int j = ja + tid; j < jb; j += NT) {
      const long long o = (long long)ir[j] - t0;
      if (o >= 0 && o < TL) {                        // (always, for an ascending row)
        // two roundings as the oracle's out[idx] += val * w.  __fmul_rn / __fadd_rn inline to
        // operators that keep their header's contraction flag (the pair still came out as one
        // v_fmac_f32), so the operators stand here with contraction switched off
#pragma clang fp contract(off)
        const float prod = wr * vr[j];
        tile[o] = tile[o] + prod;
      }
    }
    __syncthreads();                                 // rank r is in the tile before rank r + 1
  }
  for (int q = tid; q < TL / 4; q += NT) {
    const long long i0 = t0 + 4 * q;
    if (i0 >= 0 && i0 + 4 <= n) {
      *reinterpret_cast<f32x4_t*>(out + i0) = *reinterpret_cast<const f32x4_t*>(tile + 4 * q);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j >= 0 && i0 + j < n) out[i0 + j] = tile[4 * q + j];
    }
  }
}

}  // namespace

TopkPlan topk_plan(long long n) {
  TopkPlan p;
  p.chunks = (int)((n + CH - 1) / CH);
  p.scratch_ints = (long long)S_COUNTS + 2LL * p.chunks;
  return p;
}

int topk_tiles(long long n, int mis) { return (int)((n + mis + TL - 1) / TL); }

void topk_encode_launch(const float* g, float* residual, long long n, int k, int* idx, float* val,
                        int* scratch, hipStream_t st) {
  const dim3 grid(topk_plan(n).chunks), one(1), blk(NT);
  hipLaunchKernelGGL(topk_init_kernel, dim3((S_COUNTS + NT - 1) / NT), blk, 0, st, scratch, k);
  hipLaunchKernelGGL(topk_hist_kernel<0>, grid, blk, 0, st, g, residual, n, scratch);
  hipLaunchKernelGGL(topk_pick_kernel<0>, one, blk, 0, st, scratch);
  hipLaunchKernelGGL(topk_hist_kernel<1>, grid, blk, 0, st, g, residual, n, scratch);
  hipLaunchKernelGGL(topk_pick_kernel<1>, one, blk, 0, st, scratch);
  hipLaunchKernelGGL(topk_hist_kernel<2>, grid, blk, 0, st, g, residual, n, scratch);
  hipLaunchKernelGGL(topk_pick_kernel<2>, one, blk, 0, st, scratch);
  hipLaunchKernelGGL(topk_count_kernel, grid, blk, 0, st, (const float*)residual, n, scratch);
  hipLaunchKernelGGL(topk_compact_kernel, grid, blk, 0, st, residual, n, k, (const int*)scratch, idx,
                     reinterpret_cast<uint32_t*>(val));
}

void topk_decode_sum_launch(float* out, long long n, const int* idx, const float* val,
                            const float* w, int world, int k, hipStream_t st) {
  const int mis = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);
  hipLaunchKernelGGL(topk_scatter_sum_kernel, dim3(topk_tiles(n, mis)), dim3(NT), 0, st, out, n, idx, val,
                     w, world, k);
}

}  // namespace ddlpc
